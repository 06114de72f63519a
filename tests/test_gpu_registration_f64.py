"""gaussreg_amd/csrc/lgr.hip and ransac.hip against the float64 restatements of tests/registration_f64.py (SVD form, pinned
on the CPU against the reference's own modules), on the cases of tests/registration_cases.py, through every entry point.

Transform bound (derived, not tuned): both kernels form the result in fp64 and round once to fp32, so an entry of the 3x3
block may differ from the float64 value by at most 4 fp32 ulps of the scale, an entry of the translation by at most 4 fp32
ulps of |cr| + s |R cs| (registration_f64.transform_bound).  Every case prints its measured maximum as a fraction of that
bound ("REGF64 ..." lines; docs/registration_f64_errors.md holds the table of an MI355X run).

Decisions (inlier counts, the winner) are exact: admission (asserted on the CPU for every case) keeps every residual
that matters outside the fp32 evaluation band of the threshold.

Tie-break of RANSAC.  The kernel orders equal counts by its fp32 sum of squared inlier residuals, then by index.  The
winner must therefore lie within a relative 1e-5 of the smallest float64 squared error among the hypotheses of its count
(fp32 sums of up to a few thousand terms), and must be the FIRST of the hypotheses that drew the same samples in the
same order (their transforms and sums are the same bits, so only the index separates them).
"""
import numpy as np
import pytest
import torch

import registration_cases as RC
import registration_f64 as F

pytestmark = pytest.mark.gpu

GR_ERR_INVALID = -1
IDENTITY = np.eye(4, dtype=np.float32)


def _c(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))).cuda()


def _report(family, name, ratio):
    print(f"REGF64 {family:<8s} {name:<32s} max |gpu - f64| / bound = {ratio:.3f}")
    assert ratio <= 1.0, f"{family}/{name}: {ratio:.3f} of the 4-ulp bound -- a finding, not a tolerance to raise"


# ------------------------------------------------------------------------------------------------------------ RANSAC
def _ransac_single(b, c):
    from gaussreg_amd.registration import registration_with_ransac_from_correspondences as ransac
    T, st = ransac(_c(b["src"]), _c(b["ref"]), distance_threshold=b["thr"], ransac_n=c["n"], num_iterations=c["H"],
                   with_scaling=bool(c["ws"]), refine=bool(c["refine"]), seed=b["seed"], return_stats=True)
    return T.cpu().numpy(), st.cpu().numpy()


def _check_ransac(name, c, rep, T, stats):
    cnt, hid = int(stats[0]), int(stats[1])
    assert T[3].tolist() == [0, 0, 0, 1]
    assert 0 <= hid < c["H"] and rep["valid"][hid]
    assert rep["upper"][hid] >= rep["lower"].max(), f"hypothesis {hid} cannot be the best one"
    assert rep["lower"][hid] <= cnt <= rep["upper"][hid], (cnt, rep["lower"][hid], rep["upper"][hid])
    share = np.nonzero(rep["valid"] & (rep["lower"] <= cnt) & (cnt <= rep["upper"]))[0]
    e_min = rep["sqerr"][share].min()
    assert rep["sqerr"][hid] <= e_min * (1 + 1e-5), f"squared error {rep['sqerr'][hid]:.9g} of the winner, best {e_min:.9g}"
    band = share[rep["sqerr"][share] <= e_min * (1 + 1e-5)]
    # (only C_eq_n3_H64 and C_n_plus1_n3_H63 have more than one such hypothesis -- 12 and 4: they carry the index rule)
    same = [h for h in band if np.array_equal(rep["idx"][h], rep["idx"][hid])]
    assert hid == min(same), f"hypothesis {min(same)} draws the same samples as the winner {hid} and comes first"
    if c["refine"] and cnt >= 3:
        rf = rep["refit"](hid)
        want, parts = rf["T"], (rf["scale"], rf["R"], rf["cs"], rf["cr"])
    else:
        want, parts = rep["T"][hid], (rep["scale"][hid], rep["R"][hid], rep["cs"][hid], rep["cr"][hid])
    _report("ransac", name, F.bound_ratio(T, want, *parts))
    if not c["ws"]:
        assert abs(np.linalg.det(T[:3, :3].astype(np.float64)) - 1.0) < 1e-5


@pytest.mark.parametrize("case", RC.RANSAC_CASES, ids=lambda c: c["name"])
def test_ransac_matches_float64_replay(case):
    b = RC.build_ransac(case)
    rep = F.ransac_replay(b["src"], b["ref"], case["n"], case["H"], b["seed"], b["thr"], case["ws"])
    T, stats = _ransac_single(b, case)
    _check_ransac(case["name"], case, rep, T, stats)
    if case.get("tie"):
        # the tighter group wins on squared error although both groups reach the same count
        assert int(stats[0]) == 40 and np.abs(T[:3] - b["planted"]).max() < 0.05


def test_sample_hash_restatement():
    """The Python restatement of the counter hash against the library's, on 4096 tuples."""
    from gaussreg_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(0)
    tup = rng.integers(0, 2 ** 32, (4096, 4), dtype=np.uint64)
    tup[:64] = [[s, h, k, a] for s in (0, 7) for h in (0, 1, 131071, 2 ** 24 - 1) for k in (0, 7) for a in (0, 1, 64, 65)]
    got = np.array([L.gr_ransac_sample_hash(int(s), int(h), int(k), int(a)) for s, h, k, a in tup], np.uint64)
    assert np.array_equal(got, F.sample_hash(tup[:, 0], tup[:, 1], tup[:, 2], tup[:, 3]))


def test_ransac_identical_points_are_invalid():
    c = RC.RANSAC_DEGENERATE[1]
    b = RC.build_ransac(c)
    T, stats = _ransac_single(b, c)
    assert np.array_equal(T, IDENTITY) and stats.tolist() == [-1, -1]


@pytest.mark.parametrize("ws", [0, 1])
def test_ransac_collinear_points_give_a_finite_similarity(ws):
    c = dict(RC.RANSAC_DEGENERATE[0], ws=ws, scale=1.8 if ws else 1.0)
    b = RC.build_ransac(c)
    T, stats = _ransac_single(b, c)
    T = T.astype(np.float64)
    assert np.isfinite(T).all() and int(stats[0]) >= c["n"]
    s = np.cbrt(np.linalg.det(T[:3, :3]))
    R = T[:3, :3] / s
    assert s > 0 and np.abs(R @ R.T - np.eye(3)).max() <= 1e-5 and abs(np.linalg.det(R) - 1) <= 1e-5
    want = F.umeyama_batch(b["src"][None].astype(np.float64), b["ref"][None].astype(np.float64), bool(ws))["T"][0]
    worst64 = F.residuals(b["ref"], b["src"], want).max()
    worst = F.residuals(b["ref"], b["src"], T).max()
    print(f"REGF64 ransac   collinear ws={ws}: worst residual {worst:.3e} (float64 fit {worst64:.3e})")
    assert worst <= worst64 + float(F.residual_band(b["ref"], b["src"], T))


@pytest.mark.parametrize("n,C", [(2, 300), (9, 300), (5, 4), (3, 0)])
def test_ransac_rejects_bad_arguments_on_the_host(n, C):
    from gaussreg_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    pts = torch.rand((max(C, 1), 3), device=dev)
    out, st = torch.full((4, 4), 7.0, device=dev), torch.full((2,), 7, dtype=torch.int32, device=dev)
    ws = _lib.workspace(dev, L.gr_ransac_workspace_bytes(64))
    rc = L.gr_ransac_similarity(_lib.ptr(pts), _lib.ptr(pts), C, n, 64, 1, 0.05, 1, 1, _lib.ptr(out), _lib.ptr(st), _lib.ptr(ws),
                                ws.numel(), _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    assert rc == GR_ERR_INVALID and (out == 7.0).all() and (st == 7).all()      # nothing was launched
    off = torch.tensor([0, max(C, 1)], dtype=torch.int32, device=dev)
    ws = _lib.workspace(dev, L.gr_ransac_seg_workspace_bytes(64, 1))
    if n in (2, 9):
        rc = L.gr_ransac_similarity_seg(_lib.ptr(pts), _lib.ptr(pts), _lib.ptr(off), 1, n, 64, 1, 0.05, 1, 1, None, _lib.ptr(out),
                                        _lib.ptr(st), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev))
        assert rc == GR_ERR_INVALID


@pytest.mark.parametrize("with_fallback", [True, False])
def test_ransac_stack_mode(with_fallback):
    from gaussreg_amd.registration import registration_with_ransac_batch
    s = RC.build_ransac_stack()
    fb = None
    if with_fallback:
        fb = torch.arange(4 * 16, dtype=torch.float32).reshape(4, 4, 4).cuda() + 0.5
    T, st = registration_with_ransac_batch(_c(s["src"]), _c(s["ref"]), _c(s["off"]), fb, distance_threshold=s["thr"],
                                           ransac_n=s["n"], num_iterations=s["H"], seed=s["seed"], return_stats=True)
    T, st = T.cpu().numpy(), st.cpu().numpy()
    for p in (0, 1):                                  # 0 and n - 1 rows: the fallback (or the identity), stats of -1
        assert np.array_equal(T[p], fb[p].cpu().numpy() if with_fallback else IDENTITY) and st[p].tolist() == [-1, -1]
    c = dict(n=s["n"], H=s["H"], ws=1, refine=1)
    for p in (2, 3):                                  # n and 2500 rows: pair p draws with seed + p
        a, e = int(s["off"][p]), int(s["off"][p + 1])
        rep = F.ransac_replay(s["src"][a:e], s["ref"][a:e], s["n"], s["H"], s["seed"] + p, s["thr"], 1)
        if p == 3:
            assert not RC.ransac_admission(c, rep)
        _check_ransac(f"stack pair {p} fallback={int(with_fallback)}", c, rep, T[p], st[p])


# ------------------------------------------------------------------------------------------------------------ LGR
def _lgr_call(b, entry, verify=None, seg=None):
    """Straight through the C ABI: the correspondences in torch.nonzero order plus the per-patch counts / offsets / total
    the matching kernels leave in their workspace (counts[B], offsets[B], total)."""
    from gaussreg_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    ref, src, sc = _c(b["ref"]), _c(b["src"]), _c(b["scores"])
    n, B = int(ref.shape[0]), int(b["counts"].shape[0])
    pm = _c(np.concatenate([b["counts"], b["offsets"][:-1], [n]]), np.int32)
    ws = torch.empty(L.gr_lgr_workspace_bytes(B) + 256, dtype=torch.uint8, device=dev)
    st = _lib.stream_ptr(dev)
    if entry == "seg":
        nseg = len(seg) - 1
        out = torch.full((nseg, 4, 4), 7.0, device=dev)
        rows = torch.zeros(nseg + 1, dtype=torch.int32, device=dev)
        _lib.check(L.gr_lgr_register_seg(_lib.ptr(ref), _lib.ptr(src), _lib.ptr(sc), n, B, _lib.ptr(pm), _lib.ptr(_c(seg, np.int32)),
                                         nseg, b["radius"], b["thr"], b["steps"], _lib.ptr(out), _lib.ptr(rows), _lib.ptr(ws),
                                         ws.numel(), st))
        assert rows.cpu().numpy().tolist() == [int(b["offsets"][p]) for p in seg]
        return out.cpu().numpy()
    out = torch.full((4, 4), 7.0, device=dev)
    if entry == "verify":
        vr, vs, vw = [_c(a) for a in verify]
        _lib.check(L.gr_lgr_register_verify(_lib.ptr(ref), _lib.ptr(src), _lib.ptr(sc), n, B, _lib.ptr(pm), _lib.ptr(vr), _lib.ptr(vs),
                                            _lib.ptr(vw), int(vw.shape[0]), b["radius"], b["thr"], b["steps"], _lib.ptr(out),
                                            _lib.ptr(ws), ws.numel(), st))
    else:
        _lib.check(L.gr_lgr_register(_lib.ptr(ref), _lib.ptr(src), _lib.ptr(sc), n, B, _lib.ptr(pm), b["radius"], b["thr"],
                                     b["steps"], _lib.ptr(out), _lib.ptr(ws), ws.numel(), st))
    return out.cpu().numpy()


def _check_lgr(name, T, res):
    assert T[3].tolist() == [0, 0, 0, 1]
    if res["branch"] == "empty":
        assert np.array_equal(T, IDENTITY), name
        return
    last = res["last"]
    _report("lgr", name, F.bound_ratio(T, last["T"], 1.0, last["R"], last["cs"], last["cr"]))


@pytest.mark.parametrize("case", RC.LGR_CASES, ids=lambda c: c["name"])
def test_lgr_matches_float64_restatement(case):
    b = RC.build_lgr(case)
    exp = RC.lgr_expected(b)
    if case["entry"] == "seg":
        assert (len(case["patches"]) >= 2048) == ("wide" in case["name"])      # both sides of the wide-verify dispatch
        T = _lgr_call(b, "seg", seg=b["seg"])
        for s, res in enumerate(exp):
            _check_lgr(f"{case['name']} pair {s}", T[s], res)
        return
    if case["entry"] == "verify":
        T = _lgr_call(b, "verify", verify=RC.lgr_verify_set(b))
        _check_lgr(case["name"] + " (verify)", T, exp)
        return
    T = _lgr_call(b, "register")
    _check_lgr(case["name"] + " (register)", T, exp)
    Ts = _lgr_call(b, "seg", seg=[0, len(case["patches"])])                   # the same problem as a batch of one pair
    _check_lgr(case["name"] + " (seg, 1 pair)", Ts[0], exp)
    if case["name"] == "tie_first_index":
        assert exp["hyp_patch"][exp["best"]] == 1
    if case["weights"] == "tiny":
        # the reference divides by (sum w + eps) and does not renormalise: the result must be ITS shrunken centroids, not
        # the exactly renormalised ones
        other = RC.lgr_expected(b, renormalise=True)["T"]
        d_ref, d_var = np.abs(T - exp["T"]).max(), np.abs(T - other).max()
        print(f"REGF64 lgr      {case['name']}: |gpu - reference form| = {d_ref:.3e}, |gpu - renormalised| = {d_var:.3e}")
        assert d_ref < d_var


def _lgr_degenerate_checks(name, b, T, exp):
    """What is defined when the rotation is not: a finite proper rigid transform, residuals on the points no worse than
    the float64 fit's plus the fp32 band, and (R cs + t = cr) for the weighted centroids of the last fit in the
    reference's form w / (sum w + eps) -- the translation is cr - R cs whatever R the solver picked."""
    assert np.isfinite(T).all() and T[3].tolist() == [0, 0, 0, 1], name
    T = T.astype(np.float64)
    R = T[:3, :3]
    assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-5 and abs(np.linalg.det(R) - 1.0) <= 1e-5, name
    worst64, worst = F.residuals(b["ref"], b["src"], exp["T"]).max(), F.residuals(b["ref"], b["src"], T).max()
    delta = float(F.residual_band(b["ref"], b["src"], T))
    last = exp["last"]
    off = np.abs(R @ last["cs"] + T[:3, 3] - last["cr"]).max()
    print(f"REGF64 lgr      {name:<32s} worst residual {worst:.3e} (float64 fit {worst64:.3e}), "
          f"|R cs + t - cr| = {off:.3e}, delta {delta:.3e}")
    assert worst <= worst64 + delta, name
    assert off <= 4 * np.spacing(np.float32(np.abs(last["cr"]).max() + np.abs(last["cs"]).max())), name


@pytest.mark.parametrize("case", RC.LGR_DEGENERATE, ids=lambda c: c["name"])
def test_lgr_collinear_and_identical_points(case):
    b = RC.build_lgr(case)
    plain = dict(b, limit=None)
    exp = RC.lgr_expected(plain)
    assert exp["branch"] == ("global" if "global" in case["name"] else "local")
    assert all(st["mask"].all() for st in exp["steps"])                       # every correspondence is an inlier
    _lgr_degenerate_checks(case["name"] + " (register)", b, _lgr_call(plain, "register"), exp)
    _lgr_degenerate_checks(case["name"] + " (seg)", b, _lgr_call(plain, "seg", seg=[0, len(case["patches"])])[0], exp)
    vset = RC.lgr_verify_set(b)
    vb = dict(ref=vset[0], src=vset[1])
    _lgr_degenerate_checks(case["name"] + " (verify)", vb, _lgr_call(b, "verify", verify=vset), RC.lgr_expected(b))


def _module_forward(b, limit, confidence_threshold=1e-9):
    """LocalGlobalRegistration.forward on the correspondences of a built case: row i of a patch matches column i (k = 1,
    the diagonal of the score matrix holds log w, everything else -50), confidence_threshold lowered so that the scores
    of the case survive.  -> (ref, src, scores, transform) as the module returns them, and a module for further calls."""
    from gaussreg_amd.matching import LocalGlobalRegistration
    P, K = len(b["counts"]), int(b["counts"].max())
    rk, sk = np.zeros((P, K, 3), np.float32), np.zeros((P, K, 3), np.float32)
    mask, logs = np.zeros((P, K), bool), np.full((P, K, K), -50.0, np.float32)
    for p in range(P):
        a, e = int(b["offsets"][p]), int(b["offsets"][p + 1])
        rk[p, :e - a], sk[p, :e - a], mask[p, :e - a] = b["ref"][a:e], b["src"][a:e], True
        logs[p, np.arange(e - a), np.arange(e - a)] = np.log(b["scores"][a:e])
    lgr = LocalGlobalRegistration(1, b["radius"], confidence_threshold=confidence_threshold,
                                  correspondence_threshold=b["thr"], correspondence_limit=limit,
                                  num_refinement_steps=b["steps"])
    out = [x.cpu().numpy() for x in lgr(_c(rk), _c(sk), _c(mask), _c(mask), _c(logs), None)]
    assert np.array_equal(out[0], b["ref"]) and np.array_equal(out[1], b["src"])
    np.testing.assert_allclose(out[2], b["scores"], rtol=1e-5)
    return out, (lgr, rk, sk, mask, logs)


def test_lgr_module_with_correspondence_limit():
    """gr_lgr_register_verify the way the model reaches it: LocalGlobalRegistration.forward with correspondence_limit, the
    correspondences coming out of the matching kernels (confidence_threshold lowered so that scores down to 1e-6
    survive).  Expectation: the restatement on the correspondences the module returns."""
    case = next(c for c in RC.LGR_CASES if c["name"] == "verify_limit")
    b = RC.build_lgr(case)
    for limit in (b["limit"], None):
        (r, s, w, T), (lgr, rk, sk, mask, logs) = _module_forward(b, limit)
        exp = RC.lgr_expected(dict(b, scores=w, limit=limit))
        assert not RC.lgr_admission(exp)
        _check_lgr(f"module forward limit={limit}", T, exp)
    none = np.zeros_like(mask)
    T = lgr(_c(rk), _c(sk), _c(none), _c(none), _c(logs), None)[3].cpu().numpy()
    assert np.array_equal(T, IDENTITY)                                        # no correspondence at all


def test_lgr_module_with_tiny_scores():
    """A weight sum of the order of eps the way the model can reach it: scores of ~6e-8 that survive only because
    confidence_threshold is lowered below them.  The module's result must be the reference form's shrunken centroids."""
    case = next(c for c in RC.LGR_CASES if c["name"] == "weights_tiny_global")
    b = RC.build_lgr(case)
    assert b["scores"].max() < 1e-6 and b["scores"].min() > 1e-9
    (r, s, w, T), _ = _module_forward(b, None)
    assert abs(float(w.astype(np.float64).sum()) / 1e-5 - 1.0) < 0.5
    b2 = dict(b, scores=w)
    exp = RC.lgr_expected(b2)
    assert exp["branch"] == "global" and not RC.lgr_admission(exp)
    _check_lgr("module forward tiny scores", T, exp)
    other = RC.lgr_expected(b2, renormalise=True)["T"]
    d_ref, d_var = np.abs(T - exp["T"]).max(), np.abs(T - other).max()
    print(f"REGF64 lgr      module tiny scores: |gpu - reference form| = {d_ref:.3e}, |gpu - renormalised| = {d_var:.3e}")
    assert d_ref < d_var
    # with the default threshold (0.05) none of these scores is a correspondence: identity
    T0 = _module_forward_default_threshold(b)
    assert np.array_equal(T0, IDENTITY)


def _module_forward_default_threshold(b):
    from gaussreg_amd.matching import LocalGlobalRegistration
    P, K = len(b["counts"]), int(b["counts"].max())
    z = np.zeros((P, K, 3), np.float32)
    logs = np.full((P, K, K), -50.0, np.float32)
    for p in range(P):
        a, e = int(b["offsets"][p]), int(b["offsets"][p + 1])
        logs[p, np.arange(e - a), np.arange(e - a)] = np.log(b["scores"][a:e])
    m = np.ones((P, K), bool)
    lgr = LocalGlobalRegistration(1, b["radius"], correspondence_threshold=b["thr"], num_refinement_steps=b["steps"])
    return lgr(_c(z), _c(z), _c(m), _c(m), _c(logs), None)[3].cpu().numpy()
