"""CPU pins of tests/registration_f64.py, the float64 restatements the GPU tests of lgr.hip and ransac.hip compare with:

  * weighted_procrustes and local_to_global against the reference's OWN procrustes.py / local_global_registration.py,
    run in torch float64 in a child interpreter on the shared cases (skipped where the reference tree is absent: nothing
    of it is copied) -- transforms to 1e-12 relative, per-hypothesis inlier counts exactly;
  * umeyama without Open3D: planted similarities recovered, proper rotations, stationarity of the squared error;
  * the admission rule of tests/registration_cases.py for every case of the table.
"""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import registration_cases as RC
import registration_f64 as F

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
    torch.Tensor.cuda = lambda self, *a, **k: self          # the modules call .cuda() on every buffer they allocate
    torch.set_default_dtype(torch.float64)                  # ... and allocate them in the default dtype
    torch.set_num_threads(1)
    from geotransformer.modules.geotransformer.local_global_registration import LocalGlobalRegistration
    from geotransformer.modules.registration.procrustes import weighted_procrustes
    from geotransformer.modules.ops import apply_transform
    import geotransformer
    assert geotransformer.__file__.startswith(REF), geotransformer.__file__
    data, out = dict(np.load(fin)), {}
    for key in [k[:-4] for k in data if k.endswith("/ref")]:
        g = lambda n: data[key + "/" + n]
        if key.startswith("procrustes/"):
            T = weighted_procrustes(torch.from_numpy(g("src")), torch.from_numpy(g("ref")), torch.from_numpy(g("w")),
                                    return_transform=True)
            out[key + "/T"] = T.numpy()
            continue
        ref, src, sc, offs = g("ref"), g("src"), g("scores"), g("offsets")
        radius, thr, steps, limit = float(g("radius")), int(g("thr")), int(g("steps")), int(g("limit"))
        P, K = len(offs) - 1, max(1, int(np.diff(offs).max()))
        rk, sk = torch.zeros(P, K, 3), torch.zeros(P, K, 3)
        sm, cm = torch.zeros(P, K, K), torch.zeros(P, K, K, dtype=torch.bool)
        for p in range(P):                                  # row i of patch p matches column i: nonzero order = row order
            m = int(offs[p + 1] - offs[p])
            rk[p, :m], sk[p, :m] = torch.from_numpy(ref[offs[p]:offs[p + 1]]), torch.from_numpy(src[offs[p]:offs[p + 1]])
            sm[p, range(m), range(m)] = torch.from_numpy(sc[offs[p]:offs[p + 1]])
            cm[p, range(m), range(m)] = True
        lgr = LocalGlobalRegistration(1, radius, correspondence_threshold=thr,
                                      correspondence_limit=None if limit < 0 else limit, num_refinement_steps=steps)
        seen = []
        inner = lgr.procrustes.forward
        def spy(s_, r_, w_=None):
            T = inner(s_, r_, w_)
            if s_.ndim == 3:
                seen.append(T)
            return T
        lgr.procrustes.forward = spy
        gr, gs, gsc, T = lgr.local_to_global_registration(rk, sk, sm, cm)
        assert np.array_equal(gr.numpy(), ref) and np.array_equal(gs.numpy(), src) and np.array_equal(gsc.numpy(), sc)
        out[key + "/T"] = T.numpy()
        if seen:                                            # the counts of :172-177, with the reference's own operations
            if limit >= 0 and sc.shape[0] > limit:
                vsc, sel = gsc.topk(k=limit, largest=True)
                vr, vs = gr[sel], gs[sel]
            else:
                vr, vs = gr, gs
            res = torch.linalg.norm(vr.unsqueeze(0) - apply_transform(vs.unsqueeze(0), seen[0]), dim=2)
            out[key + "/counts"] = torch.lt(res, radius).sum(dim=1).numpy()
            out[key + "/hyp_T"] = seen[0].numpy()
    np.savez(fout, **out)
''')


def _pairs(b):
    """One (key suffix, arrays) per scene pair of a built LGR case: the reference handles one pair per call."""
    if b["seg"] is None:
        yield "", b["ref"], b["src"], b["scores"], b["offsets"]
        return
    for s, (pa, pe) in enumerate(zip(b["seg"][:-1], b["seg"][1:])):
        a, e = int(b["offsets"][pa]), int(b["offsets"][pe])
        if e > a:
            yield f"@{s}", b["ref"][a:e], b["src"][a:e], b["scores"][a:e], b["offsets"][pa:pe + 1] - a


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "geotransformer")), reason="the reference tree is not present")
def test_restatements_match_the_reference_modules(tmp_path):
    d64 = lambda a: np.ascontiguousarray(a, np.float64)
    feed, want = {}, {}
    rng = np.random.default_rng(5)
    for i, (n, wkind) in enumerate([(40, "uniform"), (7, "tiny"), (6, "negative"), (200, "span")]):
        src, ref, _ = RC.planted_pair("unit", "generic", n, 1.0, 0.02, rng)
        w = {"uniform": rng.random(n), "tiny": rng.random(n) * 1e-6, "negative": np.array([0.5, -0.2, 0.9, 0.3, -1.0, 0.7]),
             "span": 10.0 ** rng.uniform(-6, 0, n)}[wkind]
        key = f"procrustes/{i}"
        feed.update({key + "/ref": d64(ref + 3.0), key + "/src": d64(src + 3.0), key + "/w": d64(w)})
        want[key] = F.weighted_procrustes(src + 3.0, ref + 3.0, w)
    for c in RC.LGR_CASES:
        b = RC.build_lgr(c)
        exp = RC.lgr_expected(b)
        for (sfx, ref, src, sc, offs), e in zip(_pairs(b), [exp] if b["seg"] is None else [x for x in exp if x["branch"] != "empty"]):
            key = f"lgr/{c['name']}{sfx}"
            feed.update({key + "/ref": d64(ref), key + "/src": d64(src), key + "/scores": d64(sc),
                         key + "/offsets": np.asarray(offs, np.int64), key + "/radius": np.float64(b["radius"]),
                         key + "/thr": np.int64(b["thr"]), key + "/steps": np.int64(b["steps"]),
                         key + "/limit": np.int64(-1 if b["limit"] is None else b["limit"])})
            want[key] = e
    fin, fout = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(fin, **feed)
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-c", CHILD, REF, fin, fout], capture_output=True, text=True, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    got = dict(np.load(fout))
    worst = 0.0
    for key, e in want.items():
        T = e if isinstance(e, np.ndarray) else e["T"]
        rel = np.abs(got[key + "/T"] - T).max() / np.abs(T).max()
        worst = max(worst, rel)
        assert rel <= 1e-12, f"{key}: transform differs from the reference by {rel:.2e} relative"
        if not isinstance(e, np.ndarray) and e["branch"] == "local":
            assert np.array_equal(got[key + "/counts"], np.array(e["counts"])), f"{key}: per-hypothesis inlier counts"
            hrel = np.abs(got[key + "/hyp_T"] - np.array(e["hyp_T"])).max() / np.abs(np.array(e["hyp_T"])).max()
            assert hrel <= 1e-12, f"{key}: hypothesis transforms differ by {hrel:.2e}"
        elif not isinstance(e, np.ndarray):
            assert key + "/counts" not in got, f"{key}: the reference took the local branch, the restatement did not"
    print(f"worst relative difference to the reference modules: {worst:.2e} over {len(want)} problems")


# ------------------------------------------------------------------------------------------------------------ Umeyama
_PLANTED = [("unit", "generic", 1.8, 1), ("unit", "half_turn", 1.8, 1), ("unit", "identity", 0.05, 1),
            ("unit", "generic", 20.0, 1), ("near_planar", "generic", 1.8, 1), ("planar", "half_turn", 1.0, 0),
            ("planar_mirrored", "generic", 1.8, 1), ("planar_mirrored", "half_turn", 1.0, 0), ("unit", "generic", 1.0, 0)]


@pytest.mark.parametrize("geom,rot,scale,ws", _PLANTED)
def test_umeyama_recovers_planted_similarity(geom, rot, scale, ws):
    rng = np.random.default_rng(17)
    src, ref, T = RC.planted_pair(geom, rot, 50, scale, 0.0, rng)
    s, R, t = F.umeyama(src, ref, bool(ws))
    assert np.linalg.det(R) > 0 and np.abs(R @ R.T - np.eye(3)).max() <= 1e-13
    assert np.abs(ref - (s * src @ R.T + t)).max() <= 1e-13 * max(1.0, scale)      # noise-free: the fit is exact
    Rp, tp = T[:, :3] / scale, T[:, 3]
    if geom == "planar_mirrored":
        # (x, y, 0) -> (1 - x, y, 0) is, on the plane, the half turn about the line x = 1/2, z = 0: the proper rotation the
        # SVD form must return in place of the planted reflection
        tp = tp + scale * Rp @ np.array([1.0, 0.0, 0.0])
        Rp = Rp @ np.diag([-1.0, 1.0, -1.0])
    assert abs(s - scale) <= 1e-13 * scale
    assert np.abs(R - Rp).max() <= 1e-13 and np.abs(t - tp).max() <= 1e-12 * max(1.0, scale)


def _rodrigues(v):
    th = np.linalg.norm(v)
    if th == 0.0:
        return np.eye(3)
    k = v / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


@pytest.mark.parametrize("geom,rot,ws", [("unit", "generic", 1), ("unit", "half_turn", 0), ("near_planar", "identity", 1),
                                         ("planar_mirrored", "generic", 1)])
def test_umeyama_is_a_stationary_point_of_the_squared_error(geom, rot, ws):
    """Central differences over (log s, rotation vector, t) at the returned similarity: the gradient vanishes, to the
    accuracy of the differences, and no probe lowers the error.  Scale of the problem: sum |ref - cr|^2."""
    rng = np.random.default_rng(23)
    src, ref, _ = RC.planted_pair(geom, rot, 60, 1.8 if ws else 1.0, 0.02, rng)
    ref = ref + rng.normal(0, 0.02, ref.shape)
    s, R, t = F.umeyama(src, ref, bool(ws))
    E = lambda p: float(((ref - (s * np.exp(p[0]) * src @ (_rodrigues(p[1:4]) @ R).T + t + p[4:7])) ** 2).sum())
    big = float(((ref - ref.mean(0)) ** 2).sum())
    h, E0 = 1e-5, E(np.zeros(7))
    for k in range(0 if ws else 1, 7):
        e = np.zeros(7)
        e[k] = h
        grad = (E(e) - E(-e)) / (2 * h)
        assert abs(grad) <= 1e-8 * big, f"parameter {k}: dE = {grad:.3e} (scale {big:.3g})"
        assert E(e) >= E0 * (1 - 1e-12) and E(-e) >= E0 * (1 - 1e-12)


def test_umeyama_undefined_cases():
    p = np.tile([[0.3, 0.6, 0.2]], (5, 1))
    assert F.umeyama(p, p + 1.0, True) is None                 # no spread in src: the scale is 0 / 0
    s, R, t = F.umeyama(p, p + 1.0, False)                     # rigid: any rotation fits; the centroids must map
    assert np.allclose(R @ p[0] + t, p[0] + 1.0, atol=1e-14)


def test_sampler_retries_duplicates():
    idx = F.ransac_samples(300, 8, 2000, 3)
    assert all(len(set(r)) == 8 for r in idx.tolist()) and idx.min() >= 0 and idx.max() < 300
    idx = F.ransac_samples(4, 3, 500, 9)                        # barely above n: many retries
    first = (F.sample_hash(9, np.arange(500), 1, 0) % np.uint64(4)).astype(np.int64)
    assert (first == idx[:, 0]).any(), "no duplicate on the first try: the retry loop is not exercised"
    assert sum(len(set(r)) == 3 for r in idx.tolist()) >= 499   # 65 retries at 1/2 chance each
    assert int(F.sample_hash(0, 0, 0, 0)) == 0 and int(F.sample_hash(1, 2, 3, 4)) < 2 ** 32


# ------------------------------------------------------------------------------------------------------------ admission
@pytest.mark.parametrize("case", RC.RANSAC_CASES, ids=lambda c: c["name"])
def test_ransac_case_is_admitted(case):
    b = RC.build_ransac(case)
    rep = F.ransac_replay(b["src"], b["ref"], case["n"], case["H"], b["seed"], b["thr"], case["ws"])
    why = RC.ransac_admission(case, rep)
    assert not why, f"{case['name']} (seed {case['seed']}): {why}"
    assert rep["count"][rep["best"]] >= case["n"]


@pytest.mark.parametrize("case", RC.LGR_CASES, ids=lambda c: c["name"])
def test_lgr_case_is_admitted(case):
    b = RC.build_lgr(case)
    exp = RC.lgr_expected(b)
    for s, res in enumerate([exp] if b["seg"] is None else exp):
        why = RC.lgr_admission(res)
        assert not why, f"{case['name']} pair {s} (seed {case['seed']}): {why}"
    if case["name"] == "threshold_edge":
        assert exp["hyp_patch"] == [0, 13, 14, 15] and exp["best"] == 0      # the 5-row patches give no hypothesis
    if case["name"] == "global_branch" or case["weights"] == "tiny":
        assert exp["branch"] == "global"
    if case["name"] == "tie_first_index":
        top = [p for p, c_ in zip(exp["hyp_patch"], exp["counts"]) if c_ == max(exp["counts"])]
        assert top == [1, 2, 3, 4] and exp["hyp_patch"][exp["best"]] == 1
    if case["weights"] == "tiny":
        other = RC.lgr_expected(b, renormalise=True)
        assert np.abs(other["T"][:3, 3] - exp["T"][:3, 3]).max() > 1e-3      # the eps visibly moves the centroids


@pytest.mark.parametrize("case", RC.LGR_DEGENERATE, ids=lambda c: c["name"])
def test_lgr_degenerate_case_is_well_formed(case):
    """Collinear / identical correspondences: exempt from the gap rule, but the float64 fit must be a finite proper rigid
    transform with every correspondence an inlier far inside the radius, on the branch the case is meant to take."""
    b = RC.build_lgr(case)
    for bb in (b, dict(b, limit=None)):
        exp = RC.lgr_expected(bb)
        assert exp["branch"] == ("global" if "global" in case["name"] else "local")
        R = exp["T"][:3, :3]
        assert np.isfinite(exp["T"]).all() and np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and np.linalg.det(R) > 0
        assert min(exp["step_gaps"]) <= RC.GAP_MIN                             # really degenerate
        for st in exp["steps"]:
            assert st["mask"].all() and st["margin"].min() > 0.5 * b["radius"] > st["delta"]


def test_table_lists_what_the_issue_lists():
    R = RC.RANSAC_CASES
    for cases in (RC.RANSAC_CASES + RC.RANSAC_DEGENERATE, RC.LGR_CASES + RC.LGR_DEGENERATE):   # geometry, both solvers
        assert {"unit", "near_planar", "planar_mirrored", "collinear", "identical"} <= {c["geom"] for c in cases}
        assert {"identity", "half_turn", "generic"} <= {c["rot"] for c in cases}
        assert {1.0, 100.0, 0.01} <= {c["g"] for c in cases} and RC.OFFSET in {tuple(c["off"]) for c in cases}
    assert {"local", "global"} == {"global" if "global" in c["name"] else "local" for c in RC.LGR_DEGENERATE}
    assert {c["n"] for c in R} == {3, 4, 5, 8} and {c["ws"] for c in R} == {0, 1} and {c["refine"] for c in R} == {0, 1}
    assert {0.05, 1.8, 20.0} <= {c["scale"] for c in R} and {0.0, 0.5, 0.8} <= {c["outl"] for c in R}
    assert {1, 63, 64, 65, 10000, 131072} <= {c["H"] for c in R} and {300, 2500, 3073} <= {c["C"] for c in R}
    assert any(c["C"] == c["n"] for c in R) and any(c["C"] == c["n"] + 1 for c in R)
    assert {c["steps"] for c in RC.LGR_CASES} == {0, 1, 5} and {c["entry"] for c in RC.LGR_CASES} == {"register", "verify", "seg"}
    total = len(R) + len(RC.LGR_CASES)
    assert len(RC.SEED_REPLACED) * 10 <= total, "at most one case in ten may take another seed"
