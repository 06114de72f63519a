"""Test helper (not collected): float64 NumPy restatement of get_node_correspondences
(geotransformer/modules/registration/matching.py:231-315) for tests/test_gpu_node_correspondences.py and
tests/test_training_targets_reference.py.

The result of the operator depends only on the decisions |p - (R q + t)|^2 < r^2 over the valid point pairs of valid node
pairs.  A float32 evaluation that takes differences first and squares second decides like float64 except in a band around
the threshold: with S the largest absolute coordinate among the reference points, the transformed source points and t, a
transformed coordinate carries at most 4 roundings (3 products summed, plus t), a difference 1 more, and the sum of squares
6: about 18 * 2^-24 * S * d on d^2 at d = r.  With a factor of about 2 as slack

    tau = 2^-19 * S * r.

The restatement therefore counts twice, at r^2 - tau and at r^2 + tau, and returns overlap_lo <= overlap_hi per node pair.
Where the two agree the operator's answer is decided and must be reproduced bit for bit; elsewhere it must lie between them.
(The reference's own expanded form x^2 - 2xy + y^2 has an error of about S^2 * 2^-22, far outside this band: intended.)
The enclosing-sphere test of the reference only prunes (a pair it rejects has overlap 0), so it is not restated; pairs whose
bounding boxes are farther apart than r are skipped, which is exact."""
import numpy as np


def overlap_f32(rc, rv, sc, sv):
    """(ref_count / ref_valid + src_count / src_valid) / 2 with every operation in float32, in this order."""
    f = np.float32
    with np.errstate(divide="ignore", invalid="ignore"):
        return (f(rc) / f(rv) + f(sc) / f(sv)) / f(2)


def radius_sq_f32(pos_radius):
    """float(pos_radius) ** 2 in double, rounded once to float32: what torch.lt(fp32 tensor, python scalar) compares against."""
    return np.float32(float(pos_radius) ** 2)


def node_correspondences_f64(ref_nodes, src_nodes, ref_knn_points, src_knn_points, transform, pos_radius, ref_masks=None,
                             src_masks=None, ref_knn_masks=None, src_knn_masks=None):
    """-> dict: ov_lo, ov_hi (M, N) float32 (the fp32 overlap formula on the float64 counts at r^2 - tau / r^2 + tau; 0 where a
    side has no valid point), decided (M, N) bool (all four counts agree), tau, S."""
    rp = np.asarray(ref_knn_points, np.float64)
    sp = np.asarray(src_knn_points, np.float64)
    T = np.asarray(transform, np.float64)
    M, K = rp.shape[:2]
    N = sp.shape[0]
    rm = np.ones(M, bool) if ref_masks is None else np.asarray(ref_masks, bool)
    sm = np.ones(N, bool) if src_masks is None else np.asarray(src_masks, bool)
    rkm = np.ones((M, K), bool) if ref_knn_masks is None else np.asarray(ref_knn_masks, bool)
    skm = np.ones((N, K), bool) if src_knn_masks is None else np.asarray(src_knn_masks, bool)
    rkm = rkm & rm[:, None]
    skm = skm & sm[:, None]
    tp = sp @ T[:3, :3].T + T[:3, 3]
    r2 = float(radius_sq_f32(pos_radius))
    S = max([np.abs(T[:3, 3]).max()] + [np.abs(a).max() for a in (rp, tp) if a.size])
    tau = 2.0 ** -19 * S * float(pos_radius)
    rv, sv = rkm.sum(1), skm.sum(1)
    big = 1e100
    rlo = np.where(rkm[..., None], rp, big).min(1) if K else np.zeros((M, 3))
    rhi = np.where(rkm[..., None], rp, -big).max(1) if K else np.zeros((M, 3))
    slo = np.where(skm[..., None], tp, big).min(1) if K else np.zeros((N, 3))
    shi = np.where(skm[..., None], tp, -big).max(1) if K else np.zeros((N, 3))
    reach = float(pos_radius) * 1.01 + 1e-6
    cnt = np.zeros((4, M, N), np.int64)   # rc_lo, sc_lo, rc_hi, sc_hi
    for i in range(M):
        if rv[i] == 0:
            continue
        gap = np.maximum(np.maximum(slo - rhi[i], rlo[i] - shi), 0.0)          # (N, 3) box-to-box gap per axis
        near = np.nonzero((sv > 0) & ((gap ** 2).sum(1) <= reach ** 2))[0]
        p = rp[i][rkm[i]]
        for j in near:
            q = tp[j][skm[j]]
            d = p[:, None, :] - q[None, :, :]
            d2 = (d * d).sum(-1)
            for h, thr in enumerate((r2 - tau, r2 + tau)):
                hit = d2 < thr
                cnt[2 * h, i, j] = hit.any(1).sum()
                cnt[2 * h + 1, i, j] = hit.any(0).sum()
    live = (rv[:, None] > 0) & (sv[None, :] > 0)
    rvm, svm = np.maximum(rv, 1)[:, None], np.maximum(sv, 1)[None, :]
    ov_lo = np.where(live, overlap_f32(cnt[0], rvm, cnt[1], svm), np.float32(0)).astype(np.float32)
    ov_hi = np.where(live, overlap_f32(cnt[2], rvm, cnt[3], svm), np.float32(0)).astype(np.float32)
    decided = (cnt[0] == cnt[2]) & (cnt[1] == cnt[3])
    return dict(ov_lo=ov_lo, ov_hi=ov_hi, decided=decided, tau=tau, S=S, counts=cnt, ref_valid=rv, src_valid=sv)


def emitted(ov):
    """(corr_indices (C, 2) int64, corr_overlaps (C,)) of an (M, N) overlap matrix: the entries > 0 in row-major order."""
    idx = np.argwhere(ov > 0).astype(np.int64)
    return idx, ov[idx[:, 0], idx[:, 1]]
