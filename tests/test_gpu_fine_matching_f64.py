"""GPU: the fine-matching stage -- csrc/sinkhorn.hip (LearnableLogOptimalTransport) and csrc/point_matching.hip
(gr_corr_matrix, gr_corr_matrix_exp, gr_corr_gather) -- against the float64 restatements of tests/fine_matching_f64.py on
the case table of tests/fine_matching_cases.py: every kernel of the two files, every branch inside them, the sizes where
one path hands over to another.  Each case is admitted on the CPU before the kernel is called (see the case module).

Sinkhorn: max |gpu - f64| <= 1e-5 * max |f64| over the live entries (per matrix in the work-list cases); masked entries
are the -1e12 stand-ins, rtol 1e-6; the live pattern is equal; everything is finite.  Correspondences: corr_mat, counts,
offsets, gathered points and indices exact and in torch.nonzero order, scores at rtol 1e-5.  Every case prints its
figure on a line starting with FMF64; docs/fine_matching_f64_errors.md holds one run."""
import numpy as np
import pytest
import torch

import fine_matching_cases as C
import fine_matching_f64 as F

pytestmark = pytest.mark.gpu


def _c(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()  # (a copy: the shared references are read-only)


def _names(cases, *families):
    return [c.name for c in cases if c.family in families]


# ================================================================================================== Sinkhorn
def _transport(x):
    from gaussreg_amd.sinkhorn import LearnableLogOptimalTransport
    ot = LearnableLogOptimalTransport(x["iters"])
    with torch.no_grad():
        ot.alpha.fill_(x["alpha"])
    return ot


def _run_sinkhorn(x, **kw):
    return _transport(x)(_c(x["scores"]), _c(x["row_masks"]), _c(x["col_masks"]), **kw)


def _check_sinkhorn(name):
    case = C.SINKHORN_BY_NAME[name]
    admit = C.sinkhorn_admitted(name)                      # on the CPU, before the kernel is called
    x, want, live, _ = C.sinkhorn_reference(name)
    out = _run_sinkhorn(x)
    assert out.dtype == torch.float32 and tuple(out.shape) == (case.B, case.M + 1, case.N + 1)
    got = out.cpu().numpy()
    ratio = C.sinkhorn_ratio(got, want, live, case.per_matrix) if np.isfinite(got).all() else np.inf
    print(f"\nFMF64 sinkhorn {case.family} {name}: max error / bound = {ratio:.3f} (float32 iteration: {admit:.3f})")
    assert np.isfinite(got).all()
    assert np.array_equal(got > -1e6, live), "live / masked pattern"
    np.testing.assert_allclose(got[~live], want[~live], rtol=1e-6)
    if case.per_matrix:
        bad = [b for b in range(case.B) if C.sinkhorn_ratio(got[b:b + 1], want[b:b + 1], live[b:b + 1], False) > 1.0]
        assert not bad, f"matrices over the bound: {bad}"
    assert ratio <= 1.0, f"{name}: max |gpu - f64| is {ratio:.3f} of the bound {C.SK_BOUND:g} x scale"
    return x, got, want


@pytest.mark.parametrize("name", _names(C.SINKHORN_CASES, "scaling_512"))
def test_sinkhorn_512_thread_scaling_form(name):
    """No masks, more than 63 rows or columns: the 512-thread kernel, launched one workgroup per matrix.  Rows and
    columns 128.. belong to side waves; the shapes sit where those begin, where they end and at the maximum."""
    _check_sinkhorn(name)


@pytest.mark.parametrize("name", _names(C.SINKHORN_CASES, "log_domain"))
def test_sinkhorn_log_domain_fallback(name):
    """Scores ~ N(0, 40^2) underflow K or drive the sums out of range: the matrix is redone with logsumexp iterations."""
    _check_sinkhorn(name)


@pytest.mark.parametrize("name", _names(C.SINKHORN_CASES, "one_wave"))
def test_sinkhorn_one_wave_kernel_and_its_limit(name):
    """At most 63 valid rows and columns: one wave on the compacted problem.  63 / 64 valid on either side, prefix and
    scattered masks, a single valid row or column; nr != nc wherever masks allow, so the dustbin marginals log(nc) + norm
    (row) and log(nr) + norm (column) cannot be swapped unnoticed."""
    _check_sinkhorn(name)


@pytest.mark.parametrize("name", _names(C.SINKHORN_CASES, "work_list"))
def test_sinkhorn_work_list(name):
    """The one-wave kernel hands the matrices it does not take to the 512-thread kernel through a work list that at most
    512 workgroups walk: all four kinds of matrix in one call, and 520 items, compared matrix by matrix."""
    _check_sinkhorn(name)


def test_sinkhorn_work_list_items_do_not_depend_on_their_predecessor():
    """1024 work items on 512 workgroups: every workgroup runs two matrices, and every 13th matrix is rejected by the
    scaling form.  A matrix computes the same bits whatever its workgroup ran before it -- the give-up flags, like the
    rest of the LDS image, are set up per matrix -- so the call equals, bit for bit, two calls of 512 matrices, in which
    no workgroup has a predecessor.  (Values cannot tell: a stale flag sends a matrix to the log-domain iterations, which
    are correct too.)"""
    rng = np.random.default_rng(1024)
    B, K = 1024, 64
    sigma = np.where(np.arange(B) % 13 == 0, 40.0, 1.5)
    x = dict(scores=(rng.normal(size=(B, K, K)) * sigma[:, None, None]).astype(np.float32), row_masks=np.ones((B, K), bool),
             col_masks=np.ones((B, K), bool), alpha=1.0, iters=20)
    ot = _transport(x)
    s, rm, cm = _c(x["scores"]), _c(x["row_masks"]), _c(x["col_masks"])
    whole = ot(s, rm, cm)
    halves = torch.cat([ot(s[:512], rm[:512], cm[:512]), ot(s[512:], rm[512:], cm[512:])])
    assert bool(torch.isfinite(whole).all()) and torch.equal(whole, halves)


@pytest.mark.parametrize("name", _names(C.SINKHORN_CASES, "iterations"))
def test_sinkhorn_iteration_counts(name):
    x, got, want = _check_sinkhorn(name)
    if x["iters"] == 0:                                     # learnable_sinkhorn.py:18 with u = v = 0: padded scores - norm
        B, M, N = x["scores"].shape
        P = np.full((B, M + 1, N + 1), x["alpha"], np.float64)
        P[:, :M, :N] = x["scores"]
        np.testing.assert_allclose(got, P + np.log(float(M + N)), rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("name", _names(C.SINKHORN_CASES, "alpha"))
def test_sinkhorn_alpha(name):
    _check_sinkhorn(name)


@pytest.mark.parametrize("name", ["onewave_nomask_40x50", "scaling_129x129_s1.5", "onewave_63_vs_64", "worklist_mixed24"])
def test_sinkhorn_drop_dustbin_and_out(name):
    """drop_dustbin=True is the full result without its last row and column, bit for bit, from the one-wave kernel, the
    512-thread kernel and a call that mixes them; out= is written and returned."""
    case = C.SINKHORN_BY_NAME[name]
    x = C.sinkhorn_reference(name)[0]
    full = _run_sinkhorn(x)
    dropped = _run_sinkhorn(x, drop_dustbin=True)
    assert tuple(dropped.shape) == (case.B, case.M, case.N)
    assert torch.equal(dropped, full[:, :case.M, :case.N])
    for drop in (False, True):
        out = torch.full_like(dropped if drop else full, float("nan"))
        ret = _run_sinkhorn(x, drop_dustbin=drop, out=out)
        assert ret is out and torch.equal(out, dropped if drop else full)


def test_sinkhorn_out_is_checked_on_the_host():
    x = C.sinkhorn_reference("onewave_nomask_40x50")[0]
    B, M, N = x["scores"].shape
    for bad in (torch.empty(B, M, N, device="cuda"),                                   # shape (of the dropped form)
                torch.empty(B, M + 1, N + 1, device="cuda", dtype=torch.float64),      # dtype
                torch.empty(B, M + 1, 2 * (N + 1), device="cuda")[:, :, ::2],          # stride
                torch.empty(B, N + 1, M + 1, device="cuda").transpose(1, 2)):
        with pytest.raises(ValueError):
            _run_sinkhorn(x, out=bad)
    with pytest.raises(ValueError):
        _run_sinkhorn(x, drop_dustbin=True, out=torch.empty(B, M + 1, N + 1, device="cuda"))


def test_sinkhorn_refusals():
    """Host-side argument checks: nothing is launched."""
    from gaussreg_amd import _lib
    from gaussreg_amd.sinkhorn import LearnableLogOptimalTransport
    ot = LearnableLogOptimalTransport(100)
    for shape in ((2, 144, 10), (2, 10, 144)):
        with pytest.raises(RuntimeError, match="larger than 143"):
            ot(torch.zeros(shape, device="cuda"))
    empty = ot(torch.zeros(0, 5, 6, device="cuda"))
    assert tuple(empty.shape) == (0, 6, 7) and empty.dtype == torch.float32
    assert tuple(ot(torch.zeros(0, 5, 6, device="cuda"), drop_dustbin=True).shape) == (0, 5, 6)
    # the C entry with the header's workspace rule: accepted at that size, refused one byte below it
    L = _lib.lib()
    x = C.sinkhorn_reference("onewave_nomask_40x50")[0]
    s, alpha = _c(x["scores"]), torch.tensor([float(x["alpha"])], device="cuda")
    B, M, N = s.shape
    nbytes = L.gr_sinkhorn_workspace_bytes(B)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = torch.empty(B, M + 1, N + 1, device="cuda")

    def entry(n):
        return L.gr_sinkhorn(_lib.ptr(s), B, M, N, _lib.ptr(None), _lib.ptr(None), _lib.ptr(alpha), 100, 1e12, 0, _lib.ptr(out),
                             _lib.ptr(ws), n, _lib.stream_ptr(s.device))
    _lib.check(entry(nbytes))
    assert torch.equal(out, _run_sinkhorn(x))
    assert entry(nbytes - 1) == -3  # GR_ERR_WORKSPACE (include/gaussreg_hip.h)


# ================================================================================================== correspondences
def _matcher(case):
    from gaussreg_amd.matching import PointMatching
    return PointMatching(case.k, case.mutual, case.threshold, use_global_score=case.use_global)


def _check_point_matching(name):
    case = C.PM_BY_NAME[name]
    C.point_matching_admitted(name)                        # on the CPU, before the kernels are called
    x, want, corr_exp, _ = C.point_matching_reference(name)
    w_rp, w_sp, w_ri, w_si, w_sc, w_corr, w_off = want
    t = {k: _c(v) for k, v in x.items()}
    pm = _matcher(case)
    B = case.B
    # gr_corr_matrix_exp: the exponentiated float32 matrix, thresholded as given
    corr = pm.compute_correspondence_matrix(t["exp32"], t["ref_masks"], t["src_masks"])
    assert corr.dtype == torch.bool and np.array_equal(corr.cpu().numpy(), corr_exp)
    # gr_corr_matrix: log scores; corr_mat, the count, the per-patch counts and their exclusive scan
    _, corr, n, ws = pm._corr(t["score"], t["ref_masks"], t["src_masks"], True)
    ints = ws[:4 * (2 * B + 1)].view(torch.int32).cpu().numpy()
    assert np.array_equal(corr.cpu().numpy(), w_corr)
    assert n == int(w_corr.sum()) == int(ints[2 * B])
    assert np.array_equal(ints[:B], w_corr.reshape(B, -1).sum(1)) and np.array_equal(ints[B:2 * B], w_off)
    # gr_corr_gather through PointMatching.forward
    rp, sp, ri, si, sc = pm(t["ref_points"], t["src_points"], t["ref_masks"], t["src_masks"], t["ref_idx"], t["src_idx"],
                            t["score"], t["global_scores"])
    assert (rp.dtype, sp.dtype, ri.dtype, si.dtype, sc.dtype) == (torch.float32, torch.float32, torch.int64, torch.int64,
                                                                   torch.float32)
    assert tuple(rp.shape) == tuple(sp.shape) == (n, 3) and tuple(ri.shape) == tuple(si.shape) == tuple(sc.shape) == (n,)
    assert np.array_equal(ri.cpu().numpy(), w_ri) and np.array_equal(si.cpu().numpy(), w_si)
    assert np.array_equal(rp.cpu().numpy(), w_rp) and np.array_equal(sp.cpu().numpy(), w_sp)
    rel = float((np.abs(sc.cpu().numpy().astype(np.float64) - w_sc) / w_sc).max()) if n else 0.0
    print(f"\nFMF64 corr {case.family} {name}: {n} correspondences, score error / rtol = {rel / C.PM_SCORE_RTOL:.3f}")
    np.testing.assert_allclose(sc.cpu().numpy(), w_sc, rtol=C.PM_SCORE_RTOL, atol=0)
    return x, want


@pytest.mark.parametrize("name", _names(C.PM_CASES, "k<=4"))
def test_correspondences_one_scan_kernel(name):
    """corr_matrix_topk_kernel: K1 != K2 (row and column lines of different length in one wave), K1 + K2 > 256 (the line
    loop runs twice), widths that are no multiple of 4 and patch bases off 16 bytes (the scalar load / store branch), one
    row or one column, k = K1 = K2; the gather's 16-byte branch at the three 16384-entry shapes and its scalar branch
    elsewhere, with and without the global score, indices up to 2^40."""
    x, want = _check_point_matching(name)
    assert want[4].shape[0] > 0


@pytest.mark.parametrize("name", _names(C.PM_CASES, "k>4"))
def test_correspondences_k_rounds_kernel(name):
    """corr_matrix_kernel (k > 4): k rounds of 'largest not yet taken' per line."""
    x, want = _check_point_matching(name)
    assert want[4].shape[0] > 0


@pytest.mark.parametrize("name", _names(C.PM_CASES, "ties"))
def test_correspondences_ties_take_the_lowest_index(name):
    """Half-integer scores: most lines hold groups of bit-equal values across their k-th place; patch 1 is constant."""
    x, want = _check_point_matching(name)
    case = C.PM_BY_NAME[name]
    k = case.k
    rows, cols = np.nonzero(x["ref_masks"][1])[0], np.nonzero(x["src_masks"][1])[0]
    c1 = want[5][1]
    if case.mutual:                                         # the constant patch: the first k of every line
        assert set(zip(*np.nonzero(c1))) == {(i, j) for i in rows for j in cols if i < k and j < k}
    else:
        assert set(zip(*np.nonzero(c1))) == {(i, j) for i in rows for j in cols if i < k or j < k}


def test_correspondences_hand_made_ties():
    from gaussreg_amd.matching import PointMatching
    on = torch.ones(1, 4, dtype=torch.bool, device="cuda"), torch.ones(1, 5, dtype=torch.bool, device="cuda")
    for mutual, want in ((True, C.TIE_MUTUAL), (False, C.TIE_EITHER)):
        got = PointMatching(2, mutual, 0.05).compute_correspondence_matrix(_c(C.TIE_E), *on)
        assert np.array_equal(got[0].cpu().numpy(), want)


@pytest.mark.parametrize("name", _names(C.PM_CASES, "thresholds"))
def test_correspondences_thresholds(name):
    x, want = _check_point_matching(name)
    case = C.PM_BY_NAME[name]
    if case.threshold > 1.0:                                # above every entry: five empty tensors (checked above), count 0
        assert want[4].shape[0] == 0
    else:                                                   # 0: every top-k pick counts; 0.05 drops some of them
        loose = F.correspondence_matrix(np.exp(x["score"].astype(np.float64)), x["ref_masks"], x["src_masks"], case.k, case.mutual, 0.0)
        tight = F.correspondence_matrix(np.exp(x["score"].astype(np.float64)), x["ref_masks"], x["src_masks"], case.k, case.mutual, 0.05)
        assert 0 < tight.sum() < loose.sum() and want[5].sum() == (loose if case.threshold == 0.0 else tight).sum()


@pytest.mark.parametrize("name", _names(C.PM_CASES, "masks"))
def test_correspondences_masks(name):
    x, want = _check_point_matching(name)
    case = C.PM_BY_NAME[name]
    counts = want[5].reshape(case.B, -1).sum(1)
    if case.kind == "masked_patch":
        mid = case.B // 2
        assert counts[mid] == 0 and counts[mid - 1] > 0 and counts[mid + 1] > 0
    else:                                                   # patch 1 has entries above the threshold, all on masked lines
        every = np.ones_like(x["ref_masks"]), np.ones_like(x["src_masks"])
        unmasked = F.correspondence_matrix(np.exp(x["score"].astype(np.float64)), *every, case.k, case.mutual, case.threshold)
        assert counts[1] == 0 and unmasked[1].sum() >= 12 and counts[0] > 0 and counts[2] > 0


def test_correspondences_scan_over_5000_patches():
    """5000 per-patch counts: the exclusive scan takes three blocks; offsets and order are checked against the reference."""
    x, want = _check_point_matching("scan_5000")
    assert want[6][-1] > 5000 and (np.diff(want[6]) > 0).sum() > 4000
