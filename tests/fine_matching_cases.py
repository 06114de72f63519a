"""Test helper (not collected): the seeded case table of tests/test_gpu_fine_matching_f64.py, shared with the CPU file
tests/test_fine_matching_f64_reference.py, which walks the whole table through the admission rules.

Sinkhorn (csrc/sinkhorn.hip).  The bound is max |gpu - f64| <= SK_BOUND * max |f64| over the live entries, the bound
tests/test_gpu_next.py applies to this kernel.  Admission: the reference's own arithmetic, the same iteration in float32
(fine_matching_f64.sinkhorn_fp32), must lie within SK_ADMIT = a quarter of that bound of the float64 result; a case where
float32 itself cannot do that would test the number format, not the kernel.  Measured on the CPU over this table: see
docs/fine_matching_f64_errors.md.  The work-list cases mix score ranges inside one call, so they are admitted and
compared matrix by matrix (`per_matrix`): the scale of a N(0, 40^2) matrix must not hide an error in its N(0, 1.5^2)
neighbour.

Which kernel a matrix takes (sinkhorn.hip, gr_sinkhorn): no masks and max(M, N) <= 63, or masks and at most 63 valid
rows and columns -> one wave; otherwise the 512-thread kernel, directly (no masks) or from the work list (masks).  Inside
either, scores whose range underflows K = exp(S - rowmax) or drives a sum out of [1e-30, 1e30] take the log-domain
iterations of the 512-thread kernel.  The 512-thread scaling form gives rows / columns 128..131 to side waves; larger
matrices iterate in the log domain.

Correspondences (csrc/point_matching.hip).  Decisions are exact, so the inputs are built to make them so: log scores are
multiples of 2^-8 (GRID), two different values then differ by at least 3.9e-3 relative after exp, and equal values are
bit-equal ties, which the tie rule (lowest index) decides.  Admission: every k-th / (k+1)-th gap of a live line and every
distance to the threshold is an exact tie or exceeds PM_MARGIN = 1e-5 relative -- far more than expf differs from exp.
"""
import functools
import zlib
from collections import namedtuple

import numpy as np

import fine_matching_f64 as F

SK_BOUND = 1e-5
SK_ADMIT = 2.5e-6
PM_MARGIN = 1e-5
PM_SCORE_RTOL = 1e-5
GRID = 256.0


def _seed(name):
    return zlib.crc32(name.encode())


# ================================================================================================== Sinkhorn
# masks: None, or one (row spec, column spec) per matrix; a spec is ("all",), ("prefix", n) or ("scatter", n)
# sigmas: one value, or one per matrix
SkCase = namedtuple("SkCase", "name family B M N sigmas masks alpha iters per_matrix special salt")


def _sk(name, family, B, M, N, sigmas, masks=None, alpha=1.0, iters=100, per_matrix=False, special=None, salt=""):
    return SkCase(name, family, B, M, N, sigmas, masks, alpha, iters, per_matrix, special, salt)


# where the side rows begin (129), where they end (131 | 132) and the maximum (143); rectangles on either side of each
SK_SHAPES_512 = [(64, 64), (128, 128), (129, 129), (131, 131), (132, 132), (143, 143), (143, 64), (64, 143), (131, 140),
                 (140, 90), (1, 143), (143, 1)]
P, S, ALL = "prefix", "scatter", ("all",)


# At sigma 40 the float32 iteration itself sits at 0.1 .. 0.3 of the bound.  Two cases missed the admission with the seed of
# their name (0.296 and 0.271 of the bound) and were reseeded, as the rule asks, by the float32 CPU figure alone: of 40
# further seeds 6 and 2 passed; these are the best.
RESEEDED = {"logdomain_131x140_s40": "/28", "worklist_mixed24": "/12"}


def _mixed24():
    """24 matrices of (140, 143): b % 4 = 0 one wave; 1 over the 63 limit; 2 one wave, rejected by its range guard
    (sigma 40); 3 over the limit and rejected by the 512-thread guard.  nr != nc everywhere."""
    rng = np.random.default_rng(_seed("mixed24"))
    masks, sigmas = [], []
    for b in range(24):
        kind = b % 4
        if kind in (0, 2):
            nr, nc = (int(v) for v in rng.choice(np.arange(30, 64), 2, replace=False))
        else:
            nr, nc = int(rng.integers(64, 141)), int(rng.integers(20, 144))
            if b % 8 == 5:
                nr, nc = nc % 60 + 2, int(rng.integers(64, 144))  # over the limit on the column side only
            if nr == nc:
                nc -= 1
        masks.append(((S, nr), (S, nc)))
        sigmas.append(40.0 if kind >= 2 else (1.5 if b % 8 < 4 else 6.0))
    return masks, sigmas


def _sinkhorn_table():
    t = []
    for M, N in SK_SHAPES_512:
        for sigma in (1.5, 6.0):
            t.append(_sk(f"scaling_{M}x{N}_s{sigma:g}", "scaling_512", 3, M, N, sigma))
        t.append(_sk(f"logdomain_{M}x{N}_s40", "log_domain", 3, M, N, 40.0, salt=RESEEDED.get(f"logdomain_{M}x{N}_s40", "")))
    # one entry of an otherwise narrow row at -200: K underflows there, the sums stay in range (the cnt[3] route)
    t.append(_sk("logdomain_underflow_entry", "log_domain", 3, 128, 128, 1.0, special="underflow"))
    for M, N in ((63, 63), (63, 1), (1, 1), (40, 50)):
        t.append(_sk(f"onewave_nomask_{M}x{N}", "one_wave", 4, M, N, [1.5, 6.0, 1.5, 6.0]))
    for kind in (P, S):
        t.append(_sk(f"onewave_63_{kind}", "one_wave", 3, 143, 143, [1.5, 6.0, 1.5],
                     masks=[((kind, 63), (kind, 63)), ((kind, 63), (kind, 40)), ((kind, 40), (kind, 63))]))
    t.append(_sk("onewave_63_vs_64", "one_wave", 4, 143, 143, [1.5, 6.0, 1.5, 6.0],
                 masks=[((S, 63), (S, 64)), ((S, 64), (S, 63)), ((P, 63), (P, 64)), ((P, 64), (P, 63))]))
    t.append(_sk("onewave_single_row", "one_wave", 3, 143, 143, [1.5, 6.0, 1.5],
                 masks=[((S, 1), (S, 50)), ((P, 1), (P, 63)), ((S, 1), (S, 2))]))
    t.append(_sk("onewave_single_col", "one_wave", 3, 143, 143, [1.5, 6.0, 1.5],
                 masks=[((S, 50), (S, 1)), ((P, 63), (P, 1)), ((S, 2), (S, 1))]))
    masks, sigmas = _mixed24()
    t.append(_sk("worklist_mixed24", "work_list", 24, 140, 143, sigmas, masks=masks, per_matrix=True,
                 salt=RESEEDED["worklist_mixed24"]))
    # masks, yet more than 63 valid: the scaling form of the 512-thread kernel from the work list, its side rows and columns
    # (128..130) valid in some matrices and masked in others
    t.append(_sk("worklist_sides_131x131", "work_list", 4, 131, 131, [1.5, 6.0, 1.5, 6.0], per_matrix=True,
                 masks=[(ALL, ALL), (ALL, (S, 80)), ((S, 80), ALL), ((S, 100), (S, 70))]))
    # 64 valid rows and columns: every matrix goes to the work list, 520 items on 512 workgroups, so eight workgroups run a
    # second matrix; every 13th matrix is rejected by the scaling form, so a second matrix can follow a rejected one
    t.append(_sk("worklist_520", "work_list", 520, 64, 64, [40.0 if b % 13 == 0 else 1.5 for b in range(520)],
                 masks=[(ALL, ALL)] * 520, iters=20, per_matrix=True))
    for M, N in ((128, 128), (40, 50)):
        for iters in (0, 1, 2, 100):
            t.append(_sk(f"iters{iters}_{M}x{N}", "iterations", 3, M, N, 1.5, iters=iters))
    for alpha in (1.0, 0.37, -3.0):
        t.append(_sk(f"alpha{alpha:g}_129x70", "alpha", 3, 129, 70, 1.5, alpha=alpha))
        t.append(_sk(f"alpha{alpha:g}_40x50", "alpha", 3, 40, 50, 1.5, alpha=alpha))
    return t


SINKHORN_CASES = _sinkhorn_table()
SINKHORN_BY_NAME = {c.name: c for c in SINKHORN_CASES}
assert len(SINKHORN_BY_NAME) == len(SINKHORN_CASES)


def _mask(spec, n, rng):
    if spec[0] == "all":
        return np.ones(n, bool)
    m = np.zeros(n, bool)
    if spec[0] == "prefix":
        m[:spec[1]] = True
    else:
        m[rng.choice(n, spec[1], replace=False)] = True
    assert m.sum() >= 1  # (no empty side: the reference takes log(0) there)
    return m


def build_sinkhorn(case):
    """-> dict(scores (B, M, N) float32, row_masks, col_masks (bool or None), alpha, iters)."""
    rng = np.random.default_rng(_seed(case.name + case.salt))
    B, M, N = case.B, case.M, case.N
    sig = np.broadcast_to(np.asarray(case.sigmas, np.float64), (B,))
    scores = (rng.normal(size=(B, M, N)) * sig[:, None, None]).astype(np.float32)
    if case.special == "underflow":
        for b in range(B):
            scores[b, 5 + b, 7] = -200.0
    rm = cm = None
    if case.masks is not None:
        rm = np.stack([_mask(r, M, rng) for r, _ in case.masks])
        cm = np.stack([_mask(c, N, rng) for _, c in case.masks])
    return dict(scores=scores, row_masks=rm, col_masks=cm, alpha=case.alpha, iters=case.iters)


def sinkhorn_ratio(got, want, live, per_matrix):
    """max |got - want| / (SK_BOUND * max |want|) over the live entries: of the whole tensor, or the largest over the
    matrices each with its own scale."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if not per_matrix:
        return float(np.abs(got - want)[live].max() / (SK_BOUND * np.abs(want[live]).max()))
    return max(float(np.abs(got[b] - want[b])[live[b]].max() / (SK_BOUND * np.abs(want[b][live[b]]).max()))
               for b in range(got.shape[0]))


@functools.lru_cache(maxsize=None)
def sinkhorn_reference(name):
    """-> (inputs, float64 result, live entries, admission figure = the float32 iteration's error / SK_BOUND)."""
    case = SINKHORN_BY_NAME[name]
    x = build_sinkhorn(case)
    args = (x["scores"], x["row_masks"], x["col_masks"], x["alpha"], x["iters"])
    want = F.sinkhorn(*args)
    live = F.live_entries(x["scores"].shape, x["row_masks"], x["col_masks"])
    admit = sinkhorn_ratio(F.sinkhorn_fp32(*args), want, live, case.per_matrix)
    for a in (x["scores"], want, live):
        a.setflags(write=False)
    return x, want, live, admit


def sinkhorn_admitted(name):
    admit = sinkhorn_reference(name)[3]
    assert admit <= SK_ADMIT / SK_BOUND, f"{name}: the float32 iteration is {admit:.3f} of the bound from float64 (> 0.25)"
    return admit


# ================================================================================================== correspondences
# kind: "dual" (dual-softmax of planted logits), "ties" (half-integer scores, patch 1 constant), "masked_patch" (the
# middle patch fully masked), "masked_lines" (patch 1: every entry above the threshold sits on a masked row or column)
PmCase = namedtuple("PmCase", "name family B K1 K2 k mutual threshold kind use_global")


def _pm(name, family, B, K1, K2, k, mutual=True, threshold=0.05, kind="dual", use_global=False):
    return PmCase(name, family, B, K1, K2, k, mutual, threshold, kind, use_global)


def _pm_table():
    t = []
    shapes = [(128, 128), (64, 256), (256, 64), (200, 136), (127, 130), (3, 6), (1, 7), (7, 1), (4, 4)]
    for K1, K2 in shapes:
        ks = [4] if (K1, K2) == (4, 4) else [k for k in (1, 2, 3, 4) if k <= min(K1, K2)]
        for k in ks:
            for mutual in (True, False):
                t.append(_pm(f"topk_{K1}x{K2}_k{k}_{'mutual' if mutual else 'either'}", "k<=4", 3 if K1 * K2 > 20000 else 5,
                             K1, K2, k, mutual, use_global=(k % 2 == 0)))
    for K1, K2 in ((128, 128), (40, 50), (127, 130)):
        for k in (5, 8):
            t.append(_pm(f"rounds_{K1}x{K2}_k{k}", "k>4", 4, K1, K2, k, mutual=(k == 5), use_global=(k == 8)))
    t.append(_pm("rounds_9x12_k9", "k>4", 5, 9, 12, 9, mutual=False))
    for K1, K2 in ((40, 50), (128, 128)):
        for k in (2, 4, 5, 8):
            for mutual in (True, False):
                t.append(_pm(f"ties_{K1}x{K2}_k{k}_{'mutual' if mutual else 'either'}", "ties", 4, K1, K2, k, mutual, kind="ties"))
    for k in (3, 6):
        t.append(_pm(f"thr0_k{k}", "thresholds", 4, 40, 50, k, threshold=0.0))
        t.append(_pm(f"thr0.05_k{k}", "thresholds", 4, 40, 50, k, mutual=False, threshold=0.05))
        t.append(_pm(f"thr_above_all_k{k}", "thresholds", 4, 40, 50, k, mutual=False, threshold=2.0))
        t.append(_pm(f"masked_patch_k{k}", "masks", 5, 128, 128, k, kind="masked_patch"))
        t.append(_pm(f"masked_lines_k{k}", "masks", 3, 40, 50, k, mutual=False, kind="masked_lines"))
    # 5000 counts: the exclusive scan of the per-patch counts takes three 2048-element blocks
    t.append(_pm("scan_5000", "scan", 5000, 8, 12, 2, mutual=False, use_global=True))
    return t


PM_CASES = _pm_table()
PM_BY_NAME = {c.name: c for c in PM_CASES}
assert len(PM_BY_NAME) == len(PM_CASES)


def _log_softmax(x, axis):
    m = x.max(axis=axis, keepdims=True)
    return x - (m + np.log(np.exp(x - m).sum(axis=axis, keepdims=True)))


def build_point_matching(case):
    """-> dict of the eight arguments of PointMatching.forward (NumPy), plus exp32 = float32(exp(score))."""
    rng = np.random.default_rng(_seed(case.name))
    B, K1, K2 = case.B, case.K1, case.K2
    if case.kind == "ties":
        score = np.round(rng.normal(size=(B, K1, K2)) * 1.2) * 0.5 - 1.0
        score[1] = -1.0
    else:
        logits = rng.normal(size=(B, K1, K2)) * 3.0
        n = min(K1, K2)
        for b in range(B):  # planted matches, so that a patch holds entries well above the threshold
            logits[b, rng.permutation(K1)[:n], rng.permutation(K2)[:n]] += 6.0
        score = 0.5 * (_log_softmax(logits, 2) + _log_softmax(logits, 1))
        score = np.round(score * GRID) / GRID
    rm, sm = rng.random((B, K1)) > 0.25, rng.random((B, K2)) > 0.25
    rm[:, rng.integers(K1)] = True
    sm[:, rng.integers(K2)] = True
    if case.kind == "masked_patch":
        rm[B // 2], sm[B // 2] = False, False
    if case.kind == "masked_lines":
        score[1] = np.round(rng.normal(size=(K1, K2)) * 0.3 * GRID) / GRID - 8.0
        rm[1], sm[1] = True, True
        for r in (2, 5):
            score[1, r, rng.choice(K2, 6, replace=False)] = -0.5
            rm[1, r] = False
        score[1, rng.choice(K1, 6, replace=False), 3] = -0.25
        sm[1, 3] = False
    score = score.astype(np.float32)
    assert np.array_equal(score.astype(np.float64) * GRID, np.round(score.astype(np.float64) * GRID)), "scores off the grid"
    return dict(score=score, exp32=np.exp(score.astype(np.float64)).astype(np.float32), ref_masks=rm, src_masks=sm,
                ref_points=rng.normal(size=(B, K1, 3)).astype(np.float32), src_points=rng.normal(size=(B, K2, 3)).astype(np.float32),
                ref_idx=rng.integers(0, 2 ** 40, (B, K1)), src_idx=rng.integers(0, 2 ** 40, (B, K2)),
                global_scores=(0.1 + rng.random(B)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def point_matching_reference(name):
    """-> (inputs, float64 point_matching result on the log scores, corr_mat for the exponentiated float32 entry,
    admission figures (smallest gap, smallest threshold distance, tied lines) of both entries)."""
    case = PM_BY_NAME[name]
    x = build_point_matching(case)
    want = F.point_matching(x["ref_points"], x["src_points"], x["ref_masks"], x["src_masks"], x["ref_idx"], x["src_idx"],
                            x["score"], x["global_scores"], case.k, case.mutual, case.threshold, case.use_global)
    corr_exp = F.correspondence_matrix(x["exp32"], x["ref_masks"], x["src_masks"], case.k, case.mutual, case.threshold)
    figures = []
    for values, E in ((x["score"], np.exp(x["score"].astype(np.float64))), (x["exp32"], x["exp32"].astype(np.float64))):
        gaps, ties, dist, on_thr = F.decision_margins(values, E, x["ref_masks"], x["src_masks"], case.k, case.threshold)
        figures.append((float(gaps.min()) if gaps.size else np.inf, float(dist.min()) if dist.size else np.inf, ties, on_thr))
    return x, want, corr_exp, figures


def point_matching_admitted(name):
    figures = point_matching_reference(name)[3]
    for gap, dist, _, _ in figures:
        assert gap > PM_MARGIN, f"{name}: a k-th / (k+1)-th gap of {gap:.3e} is neither a planted tie nor above {PM_MARGIN:g}"
        assert dist > PM_MARGIN, f"{name}: an entry lies {dist:.3e} (relative) from the threshold"
    if PM_BY_NAME[name].kind == "ties":
        assert figures[0][2] > 0 and figures[1][2] > 0, f"{name}: no line ties across its k-th boundary"
    return figures


# The tie rule on a hand-made patch, k = 2, threshold 0.05.  Row 1 holds 0.3 four times: columns 0 and 1 are taken.  Row 3
# and column 2 tie at 0.4 across the second place: the lower index wins (column 2; row 2).  Column 0 ties at 0.5 inside
# the top two: both are taken.
TIE_E = np.array([[[0.5, 0.5, 0.5, 0.1, 0.1],
                   [0.3, 0.3, 0.2, 0.3, 0.3],
                   [0.1, 0.4, 0.4, 0.4, 0.04],
                   [0.5, 0.2, 0.4, 0.4, 0.04]]], np.float32)
TIE_ROWS = np.array([[1, 1, 0, 0, 0], [1, 1, 0, 0, 0], [0, 1, 1, 0, 0], [1, 0, 1, 0, 0]], bool)
TIE_COLS = np.array([[1, 1, 1, 0, 1], [0, 0, 0, 0, 1], [0, 1, 1, 1, 0], [1, 0, 0, 1, 0]], bool)
TIE_MUTUAL = np.array([[1, 1, 0, 0, 0], [0, 0, 0, 0, 0], [0, 1, 1, 0, 0], [1, 0, 0, 0, 0]], bool)
TIE_EITHER = np.array([[1, 1, 1, 0, 1], [1, 1, 0, 0, 1], [0, 1, 1, 1, 0], [1, 0, 1, 1, 0]], bool)
