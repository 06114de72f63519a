"""CPU pins of tests/geo_embedding_f64.py, the float64 restatement tests/test_gpu_geo_embedding_f64.py compares the three
evaluations of gaussreg_amd/csrc/geo_embedding.hip with, and of the case table tests/geo_embedding_cases.py:

  * the restatement against the reference module's own outputs in tests/golden/rpe.npz, and against the reference's own
    GeometricStructureEmbedding run in torch float64 in a child interpreter on the dyadic cases (skipped where the
    reference tree is absent: nothing of it is copied), 1e-12 of the scale.  torch.topk does not promise an order among
    equal distances, so a row whose neighbour SET differs from the stable-sort rule must be a row with an exact tie at the
    cut, and only such rows are left out of the comparison;
  * the admission rule for every dyadic case: fp32 squared distances equal the float64 ones, identical neighbour lists,
    |ref32 - f64| <= 1.25e-6 of the scale over the whole tensor on unmarked cases, and the marking itself;
  * the function tables of embedding.py: 4-point Lagrange interpolation in float64 against the direct function, within
    0.024 h^4 max|F''''| (the remainder |(t+1) t (t-1) (t-2)| / 24 <= 9 / 384 on [0, 1]), plus, for the fp32 rows the module
    stores, 1.25 * 2^-24 max|F| (Lebesgue constant of the rule on its middle cell times the rounding of a row).
"""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import geo_embedding_cases as GC
import geo_embedding_f64 as F
from helpers import load_golden

REF = "/root/reference"

CHILD = textwrap.dedent('''
    import sys, types
    import numpy as np
    import torch
    REF, fin, fout = sys.argv[1:4]
    sys.path.insert(0, REF)
    for name in ("ipdb", "IPython", "open3d", "coloredlogs", "easydict", "plyfile", "fpsample", "cv2"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["IPython"].embed = lambda *a, **k: None
    sys.modules["geotransformer.ext"] = types.ModuleType("geotransformer.ext")
    torch.set_default_dtype(torch.float64)
    torch.set_num_threads(4)
    from geotransformer.modules.geotransformer.geotransformer import GeometricStructureEmbedding
    import geotransformer
    assert geotransformer.__file__.startswith(REF), geotransformer.__file__
    data, out = dict(np.load(fin)), {}
    for key in [k[:-7] for k in data if k.endswith("/points")]:
        g = lambda n: data[key + "/" + n]
        C, k, mean = (int(v) for v in g("cfg"))
        m = GeometricStructureEmbedding(C, float(g("sigma")[0]), float(g("sigma")[1]), k, "mean" if mean else "max")
        m.load_state_dict({"embedding.div_term": torch.from_numpy(g("div")), "proj_d.weight": torch.from_numpy(g("w_d")),
                           "proj_d.bias": torch.from_numpy(g("b_d")), "proj_a.weight": torch.from_numpy(g("w_a")),
                           "proj_a.bias": torch.from_numpy(g("b_a"))})
        assert m.proj_d.weight.dtype == torch.float64 and m.embedding.div_term.dtype == torch.float32
        pts = torch.from_numpy(g("points"))[None]
        with torch.no_grad():
            out[key + "/out"] = m(pts)[0].numpy()
            d_idx, a_idx = m.get_embedding_indices(pts)
        out[key + "/d_idx"], out[key + "/a_idx"] = d_idx[0].numpy(), a_idx[0].numpy()
    np.savez(fout, **out)
''')


def _f64(params):
    return {k: np.asarray(v, np.float64) for k, v in params.items()}


# ------------------------------------------------------------------------------------------------------------ pins
@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_restatement_matches_reference_golden(tag):
    """gse_a/b/c of tests/golden/rpe.npz are outputs of the reference module in fp32: off the diagonal at rtol = atol =
    2e-5, on it at atol = 2e-2 (the tolerances tests/test_gpu_next.py holds the kernels to on the same vectors)."""
    g = load_golden("rpe.npz")
    c, k, mean = (int(x) for x in g[f"gse_{tag}_cfg"])
    params = {"w_d": g[f"gse_{tag}_w_d"], "b_d": g[f"gse_{tag}_b_d"], "w_a": g[f"gse_{tag}_w_a"], "b_a": g[f"gse_{tag}_b_a"],
              "div": g[f"gse_{tag}_div"]}
    pts, ref = g[f"gse_{tag}_points"][0], g[f"gse_{tag}_out"][0]
    off = ~np.eye(ref.shape[0], dtype=bool)
    for dtype in (np.float32, np.float64):
        out = F.embedding(pts, params, 0.2, 15, k, "mean" if mean else "max", dtype)
        assert out.dtype == dtype and out.shape == ref.shape
        np.testing.assert_allclose(out[off], ref[off], rtol=2e-5, atol=2e-5)
        np.testing.assert_allclose(out[~off], ref[~off], rtol=0, atol=2e-2)


_PINNED = [c for c in GC.CONFIGS if c.dyadic and c.k >= 1 and not c.name.startswith("demo")]


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "geotransformer")), reason="the reference tree is not present")
def test_restatement_matches_the_reference_module_in_float64(tmp_path):
    feed = {}
    for c in _PINNED:
        pts, params = GC.build(c)
        feed.update({f"{c.name}/points": pts, f"{c.name}/cfg": np.array([c.C, c.k, c.red == "mean"], np.int64),
                     f"{c.name}/sigma": np.array([c.sigma_d, c.sigma_a], np.float64)})
        feed.update({f"{c.name}/{k}": (v if k == "div" else v.astype(np.float64)) for k, v in params.items()})
    fin, fout = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(fin, **feed)
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-c", CHILD, REF, fin, fout], capture_output=True, text=True, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    got = dict(np.load(fout))
    worst, left_out, tie_free_compared = 0.0, 0, 0
    for c in _PINNED:
        pts, params = GC.build(c)
        want = F.embedding(pts, params, c.sigma_d, c.sigma_a, c.k, c.red, np.float64)
        d_idx, a_idx, knn = F.embedding_indices(pts, c.sigma_d, c.sigma_a, c.k, np.float64)
        assert np.abs(got[f"{c.name}/d_idx"] - d_idx).max() <= 1e-12 * max(1.0, d_idx.max()), c.name
        # rows where torch.topk chose another member of an exact tie: recognised by their angular indices (as multisets
        # over k), admitted only if the float64 distances really tie at a cut of the sorted row
        same = np.abs(np.sort(got[f"{c.name}/a_idx"], axis=2) - np.sort(a_idx, axis=2)).max(axis=(1, 2)) <= 1e-12 * 64
        dist = np.sort(d_idx, axis=1)
        for row in np.nonzero(~same)[0]:
            tied = dist[row, 0] == dist[row, 1] or (c.k + 1 < len(pts) and dist[row, c.k] == dist[row, c.k + 1])
            assert tied, f"{c.name}: row {row} differs from the reference without a tie at the cut"
        left_out += int((~same).sum())
        if same.all():
            tie_free_compared += 1
        scale = np.abs(want).max()
        rel = np.abs(got[f"{c.name}/out"][same] - want[same]).max() / scale if same.any() else 0.0
        worst = max(worst, rel)
        assert rel <= 1e-12, f"{c.name}: the restatement differs from the reference module by {rel:.2e} of the scale"
    print(f"worst difference to the reference module: {worst:.2e} of the scale over {len(_PINNED)} configurations, "
          f"{left_out} tie rows left out, {tie_free_compared} configurations compared in full")
    assert tie_free_compared >= len(_PINNED) - 12


# ------------------------------------------------------------------------------------------------------------ admission
_ADMITTED = [c for c in GC.CONFIGS if c.dyadic]


@pytest.mark.parametrize("cfg", _ADMITTED, ids=lambda c: c.name)
def test_dyadic_case_is_admitted(cfg):
    pts, params = GC.build(cfg)
    assert np.array_equal(pts.astype(np.float32).astype(np.float64), pts)
    d32, d64 = F.squared_distances(pts, np.float32), F.squared_distances(pts, np.float64)
    assert d32.dtype == np.float32 and np.array_equal(d32.astype(np.float64), d64), "fp32 squared distances are not exact"
    assert (np.diag(d64) == 0).all()
    i32, a32, k32 = F.embedding_indices(pts, cfg.sigma_d, cfg.sigma_a, cfg.k, np.float32)
    i64, a64, k64 = F.embedding_indices(pts, cfg.sigma_d, cfg.sigma_a, cfg.k, np.float64)
    assert np.array_equal(k32, k64), "fp32 and float64 neighbour lists differ"
    assert cfg.marked == bool(i64.max() > GC.MARK_INDEX), f"largest float64 index {i64.max():.4g}: the marking must follow"
    r32 = F.embedding(pts, params, cfg.sigma_d, cfg.sigma_a, cfg.k, cfg.red, np.float32)
    r64 = F.embedding(pts, params, cfg.sigma_d, cfg.sigma_a, cfg.k, cfg.red, np.float64)
    assert r32.dtype == np.float32 and r64.dtype == np.float64
    scale, e_ref = np.abs(r64).max(), np.abs(r32.astype(np.float64) - r64).max()
    print(f"GSEF64-ADMIT {cfg.name:<18s} max index {i64.max():9.3f} scale {scale:.3e} e_ref/scale {e_ref / scale:.2e}")
    if not cfg.marked:
        assert e_ref <= 1.25e-6 * scale, f"|ref32 - f64| = {e_ref / scale:.2e} of the scale: replace the case"


def test_cases_reach_what_they_are_built_for():
    B = GC.BY_NAME
    # both sides of the table / direct switch of the distance table: rows = 256 * 32 + 4, the table serves m + 3 <= rows - 1
    pts, _ = GC.build(B["table-edge"])
    i64 = F.embedding_indices(pts, 0.25, 15, 2, np.float64)[0]
    i32 = F.embedding_indices(pts, 0.25, 15, 2, np.float32)[0]
    cells = set(np.floor(i32[0].astype(np.float64) * GC.TABLE_INV_H).astype(int).tolist())
    last = int(GC.TABLE_X_MAX_D * GC.TABLE_INV_H) + 4 - 1 - 3
    assert {last - 2, last - 1, last, last + 1} <= cells and max(cells) > last + 100, sorted(cells)
    assert 256.0 in i32[0] and 256.03125 in i32[0]                 # t = 0 in the last cell; the first index served directly
    assert np.floor(i64[0] * 32).max() > last and (i64[0] < 256.03125).sum() >= 10
    # angles exactly 0 and pi
    for name in ("collinear", "collinear-mean"):
        c = B[name]
        a32 = F.embedding_indices(GC.build(c)[0], c.sigma_d, c.sigma_a, c.k, np.float32)[1]
        fa = np.float32(180.0 / (c.sigma_a * np.pi))
        assert set(np.unique(a32).tolist()) == {0.0, float(np.float32(np.pi) * fa)}
    # workgroups (128 consecutive pairs) on either side of the split kernel's 2^11 switch; none beyond it in far-1500
    for name in ("far-2800", "far-2800-c16"):
        c = B[name]
        d = F.embedding_indices(GC.build(c)[0], c.sigma_d, c.sigma_a, c.k, np.float32)[0].reshape(-1)
        big = [bool((d[i:i + 128] >= 2048).any()) for i in range(0, d.size, 128)]
        assert any(big) and not all(big), big
    c = B["far-1500"]
    d = F.embedding_indices(GC.build(c)[0], c.sigma_d, c.sigma_a, c.k, np.float32)[0]
    assert 1024 < d.max() < 2048
    # a duplicate whose twin has the lower index keeps itself as a neighbour; lattices tie at the cut
    c = B["duplicates"]
    pts = GC.build(c)[0]
    knn = F.embedding_indices(pts, c.sigma_d, c.sigma_a, c.k, np.float64)[2]
    assert knn[17, 0] == 17 and knn[3, 0] == 17 and knn[10, 0] == 10 and knn[5, 0] == 20 and knn[20, 0] == 20
    for name in ("lattice-k3", "lattice-k2-mean", "lattice-k8"):
        c = B[name]
        dist = np.sort(F.embedding_indices(GC.build(c)[0], c.sigma_d, c.sigma_a, c.k, np.float64)[0], axis=1)
        assert (dist[:, c.k] == dist[:, c.k + 1]).mean() > 0.3, name


def test_table_lists_what_the_issue_lists():
    width = lambda kern: {c.cfg.C for c in GC.CASES if GC.kernel_of(c.cfg.C, c.mode) == kern and c.cfg.dyadic}
    assert {4, 20, 64, 256, 320, 512} <= width("table")
    assert {16, 48, 64, 128, 256, 320, 512} <= width("split-bf16")
    assert {32, 64, 256, 320, 512} <= width("fp32-mfma")
    assert any(c.cfg.C > 512 and c.cfg.C % 32 == 0 and c.mode == "gemm" for c in GC.CASES)
    D = [c for c in GC.CONFIGS if c.dyadic]
    assert {0, 1, 2, 3, 8} <= {c.k for c in D}
    assert all({"max", "mean"} <= {c.red for c in D if c.k == k} for k in (2, 3, 8))
    n = lambda c: len(GC.build_cloud(c.cloud))
    sizes = {(n(c), c.k) for c in D}
    assert {(1, 0), (2, 1), (4, 3), (9, 8), (16, 3)} <= sizes and any(s[0] == 2 for s in sizes)
    assert {128, 767} <= {s[0] for s in sizes} and sum(1 for s in sizes if s[0] ** 2 % 128 != 0 and s[0] > 40) >= 2
    assert [c.modes for c in D if c.name.startswith("demo")] == [("table",)]
    assert {c.sigma_d for c in D} >= {0.2, 0.25, 0.05} and {c.sigma_a for c in D} >= {15, 10, 20}
    assert {c.wscale for c in D} >= {1.0, 4.0}
    assert sum(1 for c in GC.CONFIGS if not c.dyadic) >= 3
    assert len({c.name for c in GC.CASES}) == len(GC.CASES)


# ------------------------------------------------------------------------------------------------------------ tables
def _module(cfg, params):
    import torch
    from gaussreg_amd.embedding import GeometricStructureEmbedding
    m = GeometricStructureEmbedding(cfg.C, cfg.sigma_d, cfg.sigma_a, cfg.k, reduction_a=cfg.red)
    m.load_state_dict({"embedding.div_term": torch.from_numpy(params["div"]), "proj_d.weight": torch.from_numpy(params["w_d"]),
                       "proj_d.bias": torch.from_numpy(params["b_d"]), "proj_a.weight": torch.from_numpy(params["w_a"]),
                       "proj_a.bias": torch.from_numpy(params["b_a"])})
    return m


def _lagrange(tab, x, inv_h):
    """The kernel's rule in float64: cell m = floor(x / h), rows m .. m + 3 stand for x = (m - 1 .. m + 2) h."""
    m = np.floor(x * inv_h).astype(np.int64)
    t = (x * inv_h - m)[:, None]
    w0, w1 = -t * (t - 1) * (t - 2) / 6, (t + 1) * (t - 1) * (t - 2) / 2
    w2, w3 = -(t + 1) * t * (t - 2) / 2, (t + 1) * t * (t - 1) / 6
    return w0 * tab[m] + w1 * tab[m + 1] + w2 * tab[m + 2] + w3 * tab[m + 3]


@pytest.mark.parametrize("name", ["w64", "w256", "w20", "weights-x4", "weights-x4-c256", "weights-x8-c20", "sigma-dyadic"])
def test_function_tables_interpolate_within_the_derived_bound(name):
    import torch
    cfg = GC.BY_NAME[name]
    _, params = GC.build(cfg)
    m = _module(cfg, params)
    td, ta = (t.numpy() for t in m._function_tables(torch.device("cpu")))
    h, inv_h = 1.0 / m.TABLE_INV_H, m.TABLE_INV_H
    assert inv_h == GC.TABLE_INV_H and m.TABLE_X_MAX_D == GC.TABLE_X_MAX_D
    assert td.dtype == np.float32 and td.shape == (int(m.TABLE_X_MAX_D * inv_h) + 4, cfg.C)
    p = _f64(params)
    rng = np.random.default_rng(GC._seed(name))
    x_top_a = np.pi * 180.0 / (cfg.sigma_a * np.pi)
    for tab32, w, b, x_top in ((td, p["w_d"], p["b_d"], (td.shape[0] - 4) / inv_h), (ta, p["w_a"], p["b_a"], x_top_a)):
        rows = tab32.shape[0]
        assert (rows - 4) / inv_h >= x_top                      # the table serves every index up to x_top
        grid = (np.arange(rows) - 1.0) * h
        tab64 = F.project(grid, p["div"], w, b, np.float64)     # the rows, independently: row j <-> x = (j - 1) h
        big = np.abs(tab64).max()
        assert np.abs(tab32.astype(np.float64) - tab64).max() <= 2.0 ** -24 * big * 1.0001, "a row is not the rounded function"
        # |F''''| <= sum_i div_i^4 hypot(W[c, 2i], W[c, 2i + 1]) for every x
        m4 = (p["div"] ** 4 * np.hypot(w[:, 0::2], w[:, 1::2])).sum(axis=1).max()
        x = np.concatenate([rng.uniform(0.0, x_top, 6000), np.arange(0, int(x_top * inv_h)) * h, [x_top],
                            (np.arange(0, int(x_top * inv_h)) + 0.5) * h])
        x = x[np.floor(x * inv_h) + 3 <= rows - 1]              # the kernel's own condition
        exact = F.project(x, p["div"], w, b, np.float64)
        e64 = np.abs(_lagrange(tab64, x, inv_h) - exact).max()
        e32 = np.abs(_lagrange(tab32.astype(np.float64), x, inv_h) - exact).max()
        bound = 0.024 * h ** 4 * m4
        print(f"GSEF64-TABLE {name:<16s} rows {rows:5d} max|F| {big:.3e} interpolation {e64:.2e} (bound {bound:.2e}), "
              f"with fp32 rows {e32:.2e}")
        assert e64 <= bound + 1e-15 * big
        assert e32 <= bound + 1.25 * 2.0 ** -24 * big
