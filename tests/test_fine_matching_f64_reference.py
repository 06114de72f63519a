"""CPU: pin the float64 restatements of tests/fine_matching_f64.py against the goldens that the reference's own modules
produced (next_rows.npz, matching.npz, demo_shapes.npz) and against oracle/matching_np.py, pin the tie rule on a
hand-made example, and walk the whole case table of tests/fine_matching_cases.py through its admission rules."""
import sys

import numpy as np
import pytest

import fine_matching_cases as C
import fine_matching_f64 as F
from helpers import GOLDEN, assert_rel_scale, load_golden

sys.path.insert(0, GOLDEN)
import demo_inputs  # noqa: E402

A037 = float(np.float32(0.37))  # the reference's alpha is a float32 parameter


def _close_sinkhorn(got, want, rel):
    live = want > -1e6
    assert np.array_equal(got > -1e6, live)
    assert_rel_scale(got, want, rel, "sinkhorn", mask=live)
    np.testing.assert_allclose(got[~live], want[~live], rtol=1e-6)   # the -1e12 stand-ins


def test_sinkhorn_restatements_match_the_reference_golden():
    g = load_golden("next_rows.npz")
    for fn, rel in ((F.sinkhorn, 1e-5), (F.sinkhorn_fp32, 1e-5)):
        _close_sinkhorn(fn(g["sk_scores"], g["sk_row_masks"], g["sk_col_masks"], 1.0), g["sk_out_alpha1"], rel)
        _close_sinkhorn(fn(g["sk_scores"], g["sk_row_masks"], g["sk_col_masks"], A037), g["sk_out_alpha037"], rel)
        _close_sinkhorn(fn(g["sk_scores"], None, None, A037), g["sk_out_nomask_alpha037"], rel)
    assert F.sinkhorn(g["sk_scores"]).dtype == np.float64 and F.sinkhorn_fp32(g["sk_scores"]).dtype == np.float32


def test_sinkhorn_restatement_matches_the_reference_on_doubles_at_the_demo_shape():
    """demo_shapes.npz holds the reference module's output for four of the 256 matrices, in float32 and -- the same module
    on doubles -- in float64.  That module still builds norm, log_mu and log_nu in float32 (learnable_sinkhorn.py:49-61 use
    .float() and torch.empty's default type): three values below 8 rounded to float32, at most 2.4e-7 each, enter every
    entry additively, so the two agree to 7e-7 absolute = 4e-8 of the scale (17.5), not to float64 rounding."""
    d = load_golden("demo_shapes.npz")
    sc, rm, cm = (t.numpy() for t in demo_inputs.sinkhorn_inputs())
    assert abs(float(sc.astype(np.float64).sum()) - float(d["sk_scores_sum"])) <= 1e-11 * abs(float(d["sk_scores_sum"]))
    pick = d["sk_pick"]
    got = F.sinkhorn(sc[pick], rm[pick], cm[pick], float(d["sk_alpha"]), 100)
    _close_sinkhorn(got, d["sk_out64"], 1e-7)
    _close_sinkhorn(F.sinkhorn_fp32(sc[pick], rm[pick], cm[pick], float(d["sk_alpha"]), 100), d["sk_out32"], 1e-5)


def test_point_matching_restatement_matches_the_reference_golden():
    g = load_golden("matching.npz")
    args = [g[k] for k in ("pm_ref_points", "pm_src_points", "pm_ref_masks", "pm_src_masks", "pm_ref_idx", "pm_src_idx",
                           "pm_score", "pm_global")]
    rp, sp, ri, si, sc, corr, _ = F.point_matching(*args, k=3, mutual=True, threshold=0.05)
    assert np.array_equal(corr, g["pm_corr_mat"])
    assert np.array_equal(corr, F.correspondence_matrix(np.exp(g["pm_score"]), g["pm_ref_masks"], g["pm_src_masks"], 3, True, 0.05))
    assert np.array_equal(ri, g["pm_out_ref_idx"]) and np.array_equal(si, g["pm_out_src_idx"])
    assert np.array_equal(rp, g["pm_out_ref_points"]) and np.array_equal(sp, g["pm_out_src_points"])
    np.testing.assert_allclose(sc, g["pm_out_scores"], rtol=1e-6)
    rp, sp, ri, si, sc, corr, _ = F.point_matching(*args, k=2, mutual=False, threshold=0.1, use_global_score=True)
    assert np.array_equal(ri, g["pm2_out_ref_idx"]) and np.array_equal(si, g["pm2_out_src_idx"])
    np.testing.assert_allclose(sc, g["pm2_out_scores"], rtol=1e-6)


def test_point_matching_restatement_matches_the_reference_at_the_demo_shape():
    d = load_golden("demo_shapes.npz")
    x = {k: v.numpy() for k, v in demo_inputs.point_matching_inputs().items()}
    assert abs(float(x["score"].astype(np.float64).sum()) - float(d["pm_score_sum"])) <= 1e-11 * abs(float(d["pm_score_sum"]))
    want = np.unpackbits(d["pm_corr_bits"])[: 256 * 128 * 128].reshape(256, 128, 128).astype(bool)
    rp, sp, ri, si, sc, corr, off = F.point_matching(x["ref_points"], x["src_points"], x["ref_masks"], x["src_masks"],
                                                     x["ref_idx"], x["src_idx"], x["score"], x["global_scores"], 3, True, 0.05)
    assert np.array_equal(corr, want)
    assert np.array_equal(ri, d["pm_out_ref_idx"]) and np.array_equal(si, d["pm_out_src_idx"])
    assert np.array_equal(rp, d["pm_out_ref_points"]) and np.array_equal(sp, d["pm_out_src_points"])
    np.testing.assert_allclose(sc, d["pm_out_scores"], rtol=1e-6)
    assert off[0] == 0 and off[-1] + corr[-1].sum() == ri.shape[0]


@pytest.mark.parametrize("seed", [11, 12])
def test_restatements_match_the_numpy_oracle(seed):
    from oracle import matching_np as M
    rng = np.random.default_rng(seed)
    s = (rng.normal(size=(5, 37, 45)) * 2.0).astype(np.float32)
    rm, cm = rng.random((5, 37)) > 0.3, rng.random((5, 45)) > 0.3
    rm[:, 0], cm[:, 0] = True, True
    want = M.sinkhorn(s, rm, cm, alpha=0.5, num_iterations=50)
    _close_sinkhorn(F.sinkhorn(s, rm, cm, 0.5, 50), want, 1e-5)
    _close_sinkhorn(F.sinkhorn_fp32(s, rm, cm, 0.5, 50), want, 1e-5)
    # scores on the 2^-8 grid of the case table: no decision within fp32 noise, the two must agree exactly
    case = C._pm(f"oracle{seed}", "pin", 6, 33, 41, 3, mutual=(seed == 11), threshold=0.05, use_global=(seed == 12))
    x = C.build_point_matching(case)
    args = (x["ref_points"], x["src_points"], x["ref_masks"], x["src_masks"], x["ref_idx"], x["src_idx"], x["score"],
            x["global_scores"])
    w = M.point_matching(*args, k=3, mutual=case.mutual, confidence_threshold=0.05, use_global_score=case.use_global)
    g = F.point_matching(*args, k=3, mutual=case.mutual, threshold=0.05, use_global_score=case.use_global)
    assert w[4].shape[0] > 50
    assert np.array_equal(g[5], w[5])
    for a, b in zip(g[:4], w[:4]):
        assert np.array_equal(a, b)
    np.testing.assert_allclose(g[4], w[4], rtol=1e-6)
    assert np.array_equal(F.correspondence_matrix(x["exp32"], x["ref_masks"], x["src_masks"], 3, case.mutual, 0.05),
                          M.correspondence_matrix(x["exp32"], x["ref_masks"], x["src_masks"], 3, case.mutual, 0.05))


def test_tie_rule_on_a_hand_made_patch():
    assert np.array_equal(C.TIE_MUTUAL, C.TIE_ROWS & C.TIE_COLS) and np.array_equal(C.TIE_EITHER, C.TIE_ROWS | C.TIE_COLS)
    assert np.array_equal(F.topk_mask(C.TIE_E.astype(np.float64), 2, 2)[0], C.TIE_ROWS)
    assert np.array_equal(F.topk_mask(C.TIE_E.astype(np.float64), 2, 1)[0], C.TIE_COLS)
    on = np.ones((1, 4), bool), np.ones((1, 5), bool)
    assert np.array_equal(F.correspondence_matrix(C.TIE_E, *on, 2, True, 0.05)[0], C.TIE_MUTUAL)
    assert np.array_equal(F.correspondence_matrix(C.TIE_E, *on, 2, False, 0.05)[0], C.TIE_EITHER)
    # the masks come after the selection: masking column 0 does not hand its places in the rows to column 2
    cm = np.array([[0, 1, 1, 1, 1]], bool)
    assert np.array_equal(F.correspondence_matrix(C.TIE_E, on[0], cm, 2, False, 0.05)[0], C.TIE_EITHER & cm[0][None, :])
    gaps, ties, dist, on_thr = F.decision_margins(C.TIE_E, C.TIE_E.astype(np.float64), *on, 2, 0.05)
    assert ties == 5 and on_thr == 0          # every row and column 2: second and third value are equal
    assert gaps.min() > 0.2 and dist.min() > 0.19


def test_every_sinkhorn_case_is_admitted():
    """The float32 iteration lies within a quarter of the bound of the float64 one, for every case of the table."""
    worst = {}
    for case in C.SINKHORN_CASES:
        a = C.sinkhorn_admitted(case.name)
        worst[case.family] = max(worst.get(case.family, 0.0), a)
    print("\n" + "\n".join(f"FMF64-ADMIT sinkhorn {k}: float32 iteration at most {v * C.SK_BOUND:.2e} of the scale" for k, v in worst.items()))
    assert {c.family for c in C.SINKHORN_CASES} == {"scaling_512", "log_domain", "one_wave", "work_list", "iterations", "alpha"}


def test_every_correspondence_case_is_admitted():
    """Every top-k gap and every threshold distance is a planted tie or exceeds 1e-5 relative; no case is dropped."""
    gap = dist = np.inf
    ties = 0
    for case in C.PM_CASES:
        for g, d, t, _ in C.point_matching_admitted(case.name):
            gap, dist, ties = min(gap, g), min(dist, d), ties + t
    print(f"\nFMF64-ADMIT corr: smallest gap {gap:.2e}, smallest threshold distance {dist:.2e}, {ties} tied lines")
    assert ties > 1000
    assert {c.family for c in C.PM_CASES} == {"k<=4", "k>4", "ties", "thresholds", "masks", "scan"}


def test_case_tables_reach_the_paths_they_name():
    """Valid counts around the one-wave limit, more work items than workgroups, line loops that run twice, counts that
    leave one scan block."""
    x = C.build_sinkhorn(C.SINKHORN_BY_NAME["worklist_mixed24"])
    nr, nc = x["row_masks"].sum(1), x["col_masks"].sum(1)
    small = (nr <= 63) & (nc <= 63)
    assert small[0::4].all() and small[2::4].all() and not small[1::4].any() and not small[3::4].any() and (nr != nc).all()
    x = C.build_sinkhorn(C.SINKHORN_BY_NAME["worklist_520"])
    assert x["row_masks"].all() and x["scores"].shape == (520, 64, 64) and x["scores"].shape[0] > 512
    for name in ("onewave_63_prefix", "onewave_63_scatter"):
        x = C.build_sinkhorn(C.SINKHORN_BY_NAME[name])
        assert x["row_masks"].sum(1).tolist() == [63, 63, 40] and x["col_masks"].sum(1).tolist() == [63, 40, 63]
    assert any(c.K1 + c.K2 > 256 and c.k <= 4 for c in C.PM_CASES)
    assert sum(c.K1 * c.K2 == 16384 for c in C.PM_CASES if c.family == "k<=4") >= 3 * 8
    assert C.PM_BY_NAME["scan_5000"].B > 2 * 2048
    for c in C.PM_CASES:
        assert 3 <= c.B <= 24 or c.family == "scan"
    for c in C.SINKHORN_CASES:
        assert 3 <= c.B <= 24 or c.name == "worklist_520"
