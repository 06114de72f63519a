"""CPU: pin the float64 restatements of tests/coarse_stage_f64.py (pairwise_distance, point_to_node_partition) against the
pd_* / p2n_* goldens that the reference's own modules produced, against oracle/matching_np.py and against the reference's
modules themselves on doubles (a child interpreter; skipped where the reference tree is absent: nothing of it is copied),
pin the rules the reference leaves open, and walk the case tables of tests/coarse_stage_cases.py through their admission
rules: the float32 figures behind PD_BOUND, and the float32 oracle under the point-to-node comparison."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

import coarse_stage_cases as C
import coarse_stage_f64 as F
from helpers import load_golden

REF = "/root/reference"


def _row_sets_equal(idx, want, kmask):
    return all(set(a[m].tolist()) == set(b[m].tolist()) for a, b, m in zip(idx, want, kmask))


def test_restatements_match_the_reference_golden():
    g = load_golden("matching.npz")
    for x, y, normalized, want in ((g["pd_x"], g["pd_y"], False, g["pd_plain"]), (g["pd_xn"], g["pd_yn"], True, g["pd_normalized"])):
        got, scale = F.pairwise_distance(x, y, normalized), F.pairwise_scale(x, y, normalized)
        assert got.dtype == np.float64 and (np.abs(got - want) <= C.PD_F32_WORST * scale).all()
        for fn in (F.pairwise_fp32_torch, F.pairwise_fp32_chain):
            assert fn(x, y, normalized).dtype == np.float32 and (np.abs(fn(x, y, normalized) - got) <= C.PD_F32_WORST * scale).all()
    pts, nodes = g["p2n_points"], g["p2n_nodes"]
    ref = F.partition(pts, nodes)
    idx, mask = F.knn_tables(ref, 64)
    assert np.array_equal(ref["owner"], g["p2n_point_to_node"]) and np.array_equal(ref["node_masks"], g["p2n_node_masks"])
    assert np.array_equal(mask, g["p2n_knn_masks"]) and np.array_equal(idx, g["p2n_knn_idx"])
    got = (g["p2n_point_to_node"], g["p2n_node_masks"], g["p2n_knn_idx"], g["p2n_knn_masks"])
    F.compare_partition(got, pts, nodes, ref, 64, C.PD_BOUND)   # (and the comparison the GPU tests use accepts it)


@pytest.mark.parametrize("seed", [21, 22])
def test_restatements_match_the_numpy_oracle(seed):
    from oracle import matching_np as M
    rng = np.random.default_rng(seed)
    x, y = rng.normal(size=(37, 45)).astype(np.float32), rng.normal(size=(53, 45)).astype(np.float32)
    for normalized in (False, True):
        err = np.abs(M.pairwise_distance(x, y, normalized) - F.pairwise_distance(x, y, normalized))
        assert (err <= C.PD_F32_WORST * F.pairwise_scale(x, y, normalized)).all()
    pts = ((rng.random((2500, 3)) - 0.5) * 3.0).astype(np.float32)
    nodes = pts[rng.permutation(2500)[:90]]
    ref = F.partition(pts, nodes)
    got = M.point_to_node_partition(pts, nodes, 40)[:4]
    unclear, loose = F.compare_partition(got, pts, nodes, ref, 40, C.PD_BOUND)
    assert unclear <= 3 and loose < 45          # (28 members per node: some gaps are unclear; most rows are compared in order)


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
    torch.set_num_threads(1)
    from geotransformer.modules.ops import pairwise_distance, point_to_node_partition
    import geotransformer
    assert geotransformer.__file__.startswith(REF), geotransformer.__file__
    data, out = dict(np.load(fin)), {}
    t = lambda a: torch.from_numpy(a)
    for key in [k[:-2] for k in data if k.endswith("/x")]:
        x, y = t(data[key + "/x"]), t(data[key + "/y"])
        out[key + "/plain"] = pairwise_distance(x, y).numpy()
        out[key + "/normalized"] = pairwise_distance(x, y, normalized=True).numpy()
        out[key + "/cf"] = pairwise_distance(x.transpose(-1, -2).contiguous(), y.transpose(-1, -2).contiguous(), channel_first=True).numpy()
    for key in [k[:-7] for k in data if k.endswith("/points")]:
        K = int(data[key + "/K"])
        res = point_to_node_partition(t(data[key + "/points"]), t(data[key + "/nodes"]), K, return_count=True)
        for name, r in zip(("p2n", "sizes", "masks", "idx", "kmask"), res):
            out[key + "/" + name] = r.numpy()
    np.savez(fout, **out)
''')


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "geotransformer")), reason="the reference tree is not present")
def test_restatements_match_the_reference_modules(tmp_path):
    """The reference's pairwise_distance and point_to_node_partition on float64 tensors: distances to 1e-13 of the
    scale; owners, masks, sizes, rows and knn masks exactly -- on the room cloud, on the tie cloud (torch's argmin takes
    the first of two equal nodes; its topk leaves equal members open, so those rows are compared as sets) and with a NaN
    point (assigned to node 0, listed nowhere)."""
    d64 = lambda a: np.ascontiguousarray(a, np.float64)
    feed = {}
    for name in ("small_1x65x63x33_gauss", "small_3x50x70x17_gauss_cf", "small_1x31x97x3_room"):
        x, y = C.build_pairwise(C.PD_BY_NAME[name])
        feed[f"pd/{name}/x"], feed[f"pd/{name}/y"] = d64(x), d64(y)
    x, y = C.build_pairwise(C.PD_BY_NAME["small_1x65x63x33_gauss"])
    x, y = d64(x), d64(y)
    x[0, 3, 5], y[0, 7, 0] = np.nan, np.nan
    feed["pd/nan/x"], feed["pd/nan/y"] = x, y
    clouds = {"room": (*C.cloud("room"), 64), "ties": (*C.cloud("ties"), 128), "small3": (*C.cloud("small3"), 128)}
    pts, nodes = C.cloud("small3")
    pts = pts.copy()
    pts[11, 2] = np.nan
    clouds["nan"] = (pts, nodes, 128)
    clouds["nan_k16"] = (pts, nodes, 16)
    for name, (p, nd, K) in clouds.items():
        feed[f"p2n/{name}/points"], feed[f"p2n/{name}/nodes"], feed[f"p2n/{name}/K"] = d64(p), d64(nd), np.int64(K)
    fin, fout = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(fin, **feed)
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-c", CHILD, REF, fin, fout], capture_output=True, text=True, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    got = dict(np.load(fout))
    for key in [k[:-2] for k in feed if k.endswith("/x")]:
        x, y = feed[key + "/x"], feed[key + "/y"]
        for out, normalized in (("plain", False), ("normalized", True), ("cf", False)):
            want, scale = F.pairwise_distance(x, y, normalized), F.pairwise_scale(np.nan_to_num(x), np.nan_to_num(y), normalized)
            assert np.array_equal(np.isnan(got[f"{key}/{out}"]), np.isnan(want))
            ok = ~np.isnan(want)
            assert (np.abs(got[f"{key}/{out}"] - want)[ok] <= 1e-13 * scale[ok]).all(), key
    assert np.isnan(got["pd/nan/plain"]).sum() == 63 + 65 - 1 and np.isnan(got["pd/nan/plain"][0, 3]).all()
    for name, (p, nd, K) in clouds.items():
        ref = F.partition(p, nd)
        idx, mask = F.knn_tables(ref, K)
        g = lambda n: got[f"p2n/{name}/{n}"]
        assert np.array_equal(g("p2n"), ref["owner"]) and np.array_equal(g("masks"), ref["node_masks"]), name
        assert np.array_equal(g("sizes"), np.bincount(ref["owner"], minlength=ref["M"])), name
        assert np.array_equal(g("kmask"), mask), name
        if name == "ties":
            assert _row_sets_equal(g("idx"), idx, mask)
        else:
            assert np.array_equal(g("idx"), idx), name
    assert got["p2n/nan/p2n"][11] == 0 and not (got["p2n/nan/idx"] == 11).any() and not (got["p2n/nan_k16/idx"] == 11).any()


def test_rules_the_reference_leaves_open():
    """First minimum, (distance, index) order, NaN: stated by the restatement on a hand-made cloud, and the NaN rules by
    torch's own clamp / min / topk, which the reference calls."""
    nodes = np.array([[0, 0, 0], [2, 0, 0], [0, 0, 0]], np.float32)              # node 2 repeats node 0
    pts = np.array([[0.5, 0, 0], [0.1, 0, 0], [0.5, 0, 0], [1.9, 0, 0], [1, 0, 0], [np.nan, 0, 0], [0, 0.5, 0]], np.float32)
    ref = F.partition(pts, nodes)
    assert ref["owner"].tolist() == [0, 0, 0, 1, 0, 0, 0]       # (1, 0, 0) ties between nodes 0 and 1: the first; NaN: 0
    assert ref["node_masks"].tolist() == [True, True, False]
    assert ref["members"][0].tolist() == [1, 0, 2, 6, 4] and ref["members"][2].tolist() == []   # 0, 2, 6 tie at 0.25: by index
    idx, mask = F.knn_tables(ref, 3)
    assert idx.tolist() == [[1, 0, 2], [3, 7, 7], [7, 7, 7]] and mask.tolist() == [[1, 1, 1], [1, 0, 0], [0, 0, 0]]
    unclear, pairs = F.clarity(pts, nodes, ref, C.PD_BOUND)
    assert unclear.tolist() == [False] * 4 + [True] + [False] * 2    # the tie between two different nodes is open
    assert pairs[0].tolist() == [False, False, True, False]           # 0 / 2 are one point; 2 / 6 tie between two points
    d = torch.tensor([[float("nan"), 1.0], [0.5, 2.0]])
    assert torch.isnan(d.clamp(min=0.0)[0, 0]) and d.min(dim=0)[1].tolist() == [0, 0]
    assert torch.tensor([float("nan"), 1e12, 3.0]).topk(2, largest=False)[1].tolist() == [2, 1]
    x = np.array([[np.nan, 1.0], [1.0, 0.0]], np.float32)
    for fn in (F.pairwise_distance, F.pairwise_fp32_torch, F.pairwise_fp32_chain):
        for normalized in (False, True):
            assert np.array_equal(np.isnan(fn(x, x, normalized)), [[True, True], [True, False]])


def test_every_pairwise_case_is_admitted():
    """The float32 restatements -- the reference's expression in torch, and the kernels' ascending-k chain -- lie within a
    quarter of the bound of float64 for every case, and PD_BOUND is four times the worst of them, as measured here."""
    worst_t = worst_c = 0.0
    per_kernel = {}
    for case in C.PD_CASES:
        for normalized in (False, True):
            t, c = C.pairwise_f32_figures(case.name, normalized)
            worst_t, worst_c = max(worst_t, t), max(worst_c, c)
            per_kernel[case.kernel] = max(per_kernel.get(case.kernel, 0.0), t, c)
            assert max(t, c) <= 0.25 * C.PD_BOUND, f"{case.name}: float32 is {max(t, c):.3e} of the scale from float64"
    print(f"\nCSF64-ADMIT pairwise: torch float32 at most {worst_t:.3e}, ascending-k chain at most {worst_c:.3e} of s_ij; "
          + ", ".join(f"{k} {v / C.PD_BOUND:.3f} of the bound" for k, v in per_kernel.items()))
    assert worst_t <= C.PD_F32_TORCH * 1.001 and 0.99 * C.PD_F32_CHAIN <= worst_c <= C.PD_F32_CHAIN
    assert C.PD_BOUND == 4.0 * max(C.PD_F32_TORCH, C.PD_F32_CHAIN) <= 1e-5


def test_every_point_to_node_case_is_admitted():
    """The float32 oracle passes the comparison of every case at every K; the planted clouds have nothing unclear."""
    for name, (_, Ks, cap_p, cap_r) in C.P2N_CASES.items():
        for K in Ks:
            unclear, loose = C.p2n_admitted(name, K)
            print(f"\nCSF64-ADMIT p2n {name} K={K}: oracle passes with {unclear} unclear points, {loose} rows compared as sets")
            assert (unclear, loose) == (0, 0) or name == "room"
    ref = C.p2n_reference("planted")
    gaps = np.concatenate([np.diff(d) for d in ref["member_d"] if len(d) > 1])
    assert 1.9e-5 < gaps.min() < 2.1e-5 and ref["gap"].min() > 0.3


def test_case_tables_reach_the_paths_they_name():
    for case in C.PD_CASES:
        assert C.kernel_of(case.B, case.n, case.m, case.C, not case.misaligned) == case.kernel, case.name
    assert {c.kernel for c in C.PD_CASES} == {"small", "big_aligned", "big_vec", "big_scalar"}
    assert C.kernel_of(191, 5, 7, 20) == "small" and C.kernel_of(192, 5, 7, 20) == "big_vec"
    assert {c.C % 16 for c in C.PD_CASES if c.kernel != "small"} >= {0, 1, 15, 4, 3}
    for name in C.PD_NAN_CASES:
        assert name in C.PD_BY_NAME
    assert {C.PD_BY_NAME[n].kernel for n in C.PD_NAN_CASES} == {"small", "big_aligned", "big_vec", "big_scalar"}
    pts, nodes = C.cloud("planted")
    assert nodes.shape == (2049, 3) and 17000 < pts.shape[0] < 18500
    sizes = np.array([len(m) for m in C.p2n_reference("planted")["members"]])
    assert sizes[[1023, 1024, 2048, 0, 1025]].tolist() == [3969, 3968, 2049, 2048, 2047] and sizes.max() == 3969
    assert {63, 64, 65, 127, 128, 129} <= set(sizes.tolist()) and (sizes == 0).sum() > 100
    assert [C.cloud(n)[0].shape[0] for n in C.STACK][1:4] == [130, 40, 0] and [C.cloud(n)[1].shape[0] for n in C.STACK] == [2049, 3, 0, 0, 1030]
