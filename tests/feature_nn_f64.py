"""Test helper (not collected): the float64 brute force for gr_feature_nn and the comparison against it.

A candidate's distance may be off by PD_BOUND * s (the pairwise bound of coarse_stage_cases, s = |x_i|^2 + |y_j|^2, or
2 + 2 |x_i| |y_j| when normalized).  A decision between the best candidate and the runner-up is therefore CLEAR when their
float64 gap exceeds 2 * PD_BOUND * s, s taken of the larger of the two candidates; a clear decision must be reproduced
exactly, an unclear one must pick a candidate whose float64 distance is within that threshold of the minimum."""
import functools

import numpy as np

import coarse_stage_f64 as F
from coarse_stage_cases import PD_BOUND


def brute_force(x, y, normalized):
    """-> dict: d64 (n, m), scale (n, m), and per direction the float64 argmin (ties: lowest index), the clear mask and the
    threshold 2 * PD_BOUND * s of the decision."""
    d = F.pairwise_distance(x, y, normalized)
    s = F.pairwise_scale(x, y, normalized)
    out = {"d64": d, "scale": s}
    for tag, dd, ss in (("row", d, s), ("col", d.T, s.T)):
        k = dd.shape[0]
        best = dd.argmin(1)
        if dd.shape[1] > 1:
            part = np.argpartition(dd, 1, axis=1)[:, :2]
            second = np.where(part[:, 0] == best, part[:, 1], part[:, 0])
            # (argpartition may put another holder of the minimum first: then that one is the runner-up, gap 0)
            rows = np.arange(k)
            thr = 2.0 * PD_BOUND * np.maximum(ss[rows, best], ss[rows, second])
            clear = dd[rows, second] - dd[rows, best] > thr
        else:
            thr = 2.0 * PD_BOUND * ss[np.arange(k), best] if dd.shape[1] else np.zeros(k)
            clear = np.ones(k, bool)
        out[tag + "_index"], out[tag + "_clear"], out[tag + "_thr"] = best, clear, thr
    return out


def compare(ref, got):
    """got = (row_index, row_dist2, col_index, col_dist2) as numpy.  -> dict of figures; raises AssertionError on a clear
    decision that differs, an unclear one outside its threshold, or a distance outside the bound."""
    d, s = ref["d64"], ref["scale"]
    figures = {}
    for tag, dd, ss, idx, dist in (("row", d, s, got[0], got[1]), ("col", d.T, s.T, got[2], got[3])):
        k = dd.shape[0]
        rows = np.arange(k)
        idx, dist = np.asarray(idx), np.asarray(dist, np.float64)
        assert idx.shape == (k,) and ((0 <= idx) & (idx < dd.shape[1])).all(), tag
        best, clear, thr = ref[tag + "_index"], ref[tag + "_clear"], ref[tag + "_thr"]
        assert np.array_equal(idx[clear], best[clear]), (tag, int((idx[clear] != best[clear]).sum()))
        excess = dd[rows, idx] - dd[rows, best]
        thr_picked = 2.0 * PD_BOUND * np.maximum(ss[rows, idx], ss[rows, best])
        assert (excess[~clear] <= thr_picked[~clear]).all(), tag
        ratio = np.abs(dist - dd[rows, idx]) / (PD_BOUND * ss[rows, idx])
        assert np.isfinite(dist).all() and (dist >= 0).all() and (ratio <= 1.0).all(), (tag, float(ratio.max()))
        figures[tag + "_unclear"] = float((~clear).mean()) if k else 0.0
        figures[tag + "_dist_ratio"] = float(ratio.max()) if k else 0.0
        figures[tag + "_differs"] = int((idx != best).sum())
    return figures


def fp32_restatement(x, y, normalized):
    """The reference's expression in torch float32 on the CPU, reduced: -> (row_index, row_dist2, col_index, col_dist2)."""
    from feature_nn_cases import reduce_matrix
    return reduce_matrix(F.pairwise_fp32_torch(x, y, normalized))


@functools.lru_cache(maxsize=None)
def reference(name, normalized):
    """The brute force of a case of feature_nn_cases (unit rows when normalized), computed once and shared."""
    import feature_nn_cases as C
    x, y = C.build(name)
    if normalized:
        x, y = C.unit_rows(x), C.unit_rows(y)
    ref = brute_force(x, y, normalized)
    for v in ref.values():
        v.setflags(write=False)
    return x, y, ref
