"""CPU: (1) the float64 restatements of tests/kpconv_rpe_f64.py against outputs the reference's own modules produced
(tests/golden/next_rows.npz, rpe.npz) and against the fp32 NumPy oracle; (2) the KPConv case table of the GPU path tests
reaches every compiled variant gr_kpconv_forward can dispatch to, as reported by the host-only gr_kpconv_plan; (3) the
case generator keeps every feature row's sum away from the fp32 rounding of the `sum > 0` neighbour flag."""
import numpy as np
import pytest

import kpconv_cases
from helpers import assert_rel_scale, load_golden
from kpconv_rpe_f64 import kpconv_f64, rpe_attention_f64


def test_kpconv_f64_matches_reference_golden():
    g = load_golden("next_rows.npz")
    y = kpconv_f64(g["kp_s_feats"], g["kp_q_points"], g["kp_s_points"], g["kp_neighbors"], g["kp_kernel_points"],
                   g["kp_weights"], float(g["kp_sigma"]), g["kp_bias"])
    assert y.dtype == np.float64
    assert_rel_scale(y, g["kp_out"], 1e-5, "kpconv_f64 vs the reference's output")
    # the chunking over query rows is memory management only
    y1 = kpconv_f64(g["kp_s_feats"], g["kp_q_points"], g["kp_s_points"], g["kp_neighbors"], g["kp_kernel_points"],
                    g["kp_weights"], float(g["kp_sigma"]), g["kp_bias"], rows_per_chunk=7)
    assert np.abs(y1 - y).max() <= 1e-13 * np.abs(y).max()


@pytest.mark.parametrize("feats", ["relu", "mixed"])
def test_kpconv_f64_matches_fp32_oracle(feats):
    from oracle import matching_np as M
    c = kpconv_cases.case("pin-" + feats, 24, 40, 30, m=500, n=700, feats=feats, bias=True, special="shadow_rows")
    x = kpconv_cases.build(c)
    kpconv_cases.assert_flag_margin(x["f"])
    want = M.kpconv(x["f"], x["qp"], x["sp"], x["idx"], x["kp"], x["w"], c.sigma, x["b"])
    got = kpconv_f64(x["f"], x["qp"], x["sp"], x["idx"], x["kp"], x["w"], c.sigma, x["b"])
    assert (x["idx"] == c.n).all(1).any() and not (x["idx"] == c.n).all()
    assert_rel_scale(got, want, 1e-5, "kpconv_f64 vs oracle.matching_np.kpconv")
    assert np.array_equal(got[(x["idx"] == c.n).all(1)], np.broadcast_to(x["b"].astype(np.float64), (int((x["idx"] == c.n).all(1).sum()), 40)))


def _rpe_golden():
    g = load_golden("rpe.npz")
    sd = {k[len("rpe_sd_"):].replace("__", "."): v for k, v in g.items() if k.startswith("rpe_sd_")}
    return g, sd, int(g["rpe_cfg"][1])


def test_rpe_attention_f64_matches_reference_golden():
    g, sd, heads = _rpe_golden()
    q, k, e = g["rpe_q"][0], g["rpe_k"][0], g["rpe_emb"][0]
    hid, sc, _ = rpe_attention_f64(sd, q, k, k, e, num_heads=heads)
    assert hid.dtype == np.float64
    assert_rel_scale(hid, g["rpe_h0"][0], 1e-5, "rpe_attention_f64 hidden")
    assert_rel_scale(sc, g["rpe_s0"][0], 1e-5, "rpe_attention_f64 scores")
    hid, sc, _ = rpe_attention_f64(sd, q, k, k, e, g["rpe_weights"][0], g["rpe_masks"][0], g["rpe_factors"][0], num_heads=heads)
    assert_rel_scale(hid, g["rpe_h1"][0], 1e-5, "rpe_attention_f64 hidden (factors, weights, masks)")
    assert_rel_scale(sc, g["rpe_s1"][0], 1e-5, "rpe_attention_f64 scores (factors, weights, masks)")
    assert (sc[:, :, g["rpe_masks"][0].astype(bool)] == 0).all()
    # the float32 evaluation of the same formulas (the "reference's own error" side of the GPU bar) is close, not equal
    h32, s32, _ = rpe_attention_f64(sd, q, k, k, e, num_heads=heads, dtype=np.float32)
    assert h32.dtype == np.float32 and np.abs(h32 - rpe_attention_f64(sd, q, k, k, e, num_heads=heads)[0]).max() > 0
    assert_rel_scale(h32, g["rpe_h0"][0], 1e-5, "rpe_attention_f64(dtype=float32) hidden")
    assert_rel_scale(s32, g["rpe_s0"][0], 1e-5, "rpe_attention_f64(dtype=float32) scores")


def test_rpe_attention_f64_positional_term_and_masked_rows():
    """The third return value is the q . proj_p(emb) term alone: with k = 0 and proj_k.bias = 0 the scores are its softmax.
    Every key masked: NaN rows in hidden and scores, as softmax over a row of -inf gives in the reference."""
    g, sd, heads = _rpe_golden()
    q, k, e = g["rpe_q"][0], g["rpe_k"][0], g["rpe_emb"][0]
    sd0 = dict(sd)
    sd0["proj_k.weight"] = np.zeros_like(sd["proj_k.weight"])
    sd0["proj_k.bias"] = np.zeros_like(sd["proj_k.bias"])
    _, sc, pos = rpe_attention_f64(sd0, q, k, k, e, num_heads=heads)
    z = pos / np.sqrt(q.shape[1] // heads)
    z = np.exp(z - z.max(-1, keepdims=True))
    assert np.abs(sc - z / z.sum(-1, keepdims=True)).max() <= 1e-14
    _, _, pos1 = rpe_attention_f64(sd, q, k, k, e, num_heads=heads)
    assert np.array_equal(pos, pos1)                                    # does not depend on the keys
    hid, sc, _ = rpe_attention_f64(sd, q, k, k, e, key_masks=np.ones(k.shape[0], bool), num_heads=heads)
    assert np.isnan(hid).all() and np.isnan(sc).all()


# ---------------------------------------------------------------- dispatch coverage of the GPU case table
@pytest.fixture(scope="module")
def plan():
    from gaussreg_amd import _lib, build
    build.build()  # hipcc cross-compiles for gfx950 without a GPU; the query itself is host code
    L = _lib.lib()
    return lambda c, aligned=1: L.gr_kpconv_plan(c.n, c.m, c.h, c.cin, c.cout, c.k, aligned)


# include/gaussreg_hip.h
MFMA = {16: 0, 32: 1, 64: 2, 128: 3, 256: 4}
T64, T128, T256, KERNEL_MASK, FLUSH, CHUNKED = 5, 6, 7, 15, 16, 32
SMALL, P128X64, P64X128, P128X128, ALIGNED = 0, 1, 2, 3, 4


def test_kpconv_plan_follows_the_documented_rule(plan):
    c = kpconv_cases.case
    assert plan(c("a", 64, 64, 64, m=128)) == MFMA[64] | (P128X64 | ALIGNED) << 8
    assert plan(c("a", 64, 64, 65, m=128)) == T64 | (P128X64 | ALIGNED) << 8
    assert plan(c("a", 64, 64, 64, m=128, n=0)) == T64 | (P128X64 | ALIGNED) << 8     # no support points: generic kernel
    assert plan(c("a", 64, 64, 64, m=127)) == MFMA[64] | SMALL << 8
    assert plan(c("a", 64, 16, 64, m=128)) == MFMA[64] | SMALL << 8
    assert plan(c("a", 64, 64, 64, m=128), aligned=0) == MFMA[64] | P128X64 << 8
    assert plan(c("a", 65, 65, 257, m=128)) == T128 | CHUNKED | P64X128 << 8
    assert plan(c("a", 257, 68, 256, m=128)) == T256 | FLUSH | P64X128 << 8          # Kd = 3855
    assert plan(c("a", 16, 128, 4, m=128 * 768)) == MFMA[16] | (P128X128 | ALIGNED) << 8
    assert plan(c("a", 16, 128, 4, m=128 * 767)) == MFMA[16] | (P64X128 | ALIGNED) << 8
    assert plan(c("a", 16, 128, 4, m=0)) == -1 and plan(c("a", 16, 128, 4, k=17)) == -1


def test_kpconv_case_table_reaches_every_variant(plan):
    """Every gather kernel, both inner branches of the generic gather (alone and together) and every product kernel in both
    forms must be reached by a case of the GPU test's table.  A variant added to gr_kpconv_forward gets a code in the
    header and fails here until the table has a case for it."""
    reached = {}
    for c in kpconv_cases.CASES:
        p = plan(c)
        if c.m == 0:
            assert p == -1
            continue
        assert p >= 0, c.name
        reached.setdefault(("gather", p & KERNEL_MASK), []).append(c.name)
        reached.setdefault(("gather-branches", p & (FLUSH | CHUNKED)), []).append(c.name)
        reached.setdefault(("product", p >> 8), []).append(c.name)
        assert (p & 0xff) & ~(KERNEL_MASK | FLUSH | CHUNKED) == 0 and (p >> 8) <= (P128X128 | ALIGNED), (c.name, p)
    want = [("gather", code) for code in range(8)]
    want += [("gather-branches", b) for b in (0, FLUSH, CHUNKED, FLUSH | CHUNKED)]
    want += [("product", code) for code in (SMALL, P128X64, P64X128, P128X128, P128X64 | ALIGNED, P64X128 | ALIGNED,
                                            P128X128 | ALIGNED)]
    missing = [w for w in want if w not in reached]
    assert not missing, f"no case reaches {missing}"
    assert sorted(reached) == sorted(want)                      # and nothing the table above does not know
    # the generic kernel at each width without either branch, and the MFMA widths at H = 65 / n = 0 on the generic kernel
    by_name = {c.name: plan(c) for c in kpconv_cases.CASES if c.m > 0}
    assert by_name["generic-cin64-h65"] & 0xff == T64 and by_name["n0-bias"] & 0xff == T64
    assert by_name["flush-cin512"] & 0xff == T256 | FLUSH and by_name["chunked-h300-cin300"] & 0xff == T256 | FLUSH | CHUNKED
    assert by_name["chunked-h300-cin48"] & 0xff == T64 | CHUNKED


@pytest.mark.parametrize("c", kpconv_cases.CASES, ids=kpconv_cases.CASE_IDS)
def test_kpconv_case_inputs_keep_the_flag_margin(c):
    """All-zero rows or |sum_c f| >= 1e-3 sum_c |f|: no row's `sum > 0` flag depends on the fp32 summation order, so the GPU
    comparison excludes no output row.  Also: the table's special rows are really there."""
    x = kpconv_cases.build(c)
    kpconv_cases.assert_flag_margin(x["f"])
    assert x["f"].shape == (c.n, c.cin) and x["idx"].shape == (c.m, c.h) and x["w"].shape == (c.k, c.cin, c.cout)
    if c.n and c.m and c.h:
        assert x["idx"].min() >= 0 and x["idx"].max() <= c.n
        real = x["idx"] < c.n
        assert real.any()
        if c.feats == "mixed" and c.special is None:
            s = x["f"].astype(np.float64).sum(1)
            assert (s > 0).any() and (s < 0).any() and (s == 0).any()
    if c.special == "shadow_rows":
        assert (x["idx"] == c.n).all(1).sum() >= c.m // 7
    if c.special == "zero_rows":
        fz = np.concatenate([x["f"], np.zeros((1, c.cin), np.float32)])[x["idx"]]
        assert ((fz == 0).all((1, 2)) & (x["idx"] < c.n).any(1)).any()
