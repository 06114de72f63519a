"""Test helper (not collected): float64 restatements of the fine-matching stage, for tests/test_gpu_fine_matching_f64.py
(csrc/sinkhorn.hip, csrc/point_matching.hip) and the CPU file tests/test_fine_matching_f64_reference.py, which pins them
against the goldens that the reference's own modules produced.

  sinkhorn                geotransformer/modules/sinkhorn/learnable_sinkhorn.py:13-66, the log-domain iteration as written
  sinkhorn_fp32           the same with every array in float32: what the reference computes; used for admission only
  correspondence_matrix   geotransformer/modules/geotransformer/point_matching.py:32-66 (== local_global_registration.py:49-83)
  point_matching          point_matching.py:96-115 (use_dustbin=False)
  decision_margins        how far every top-k decision and every threshold decision of a patch batch is from flipping

Tie rule of the top-k (torch.topk leaves it open; the kernels promise it): among equal values the LOWEST index is taken --
a stable sort by descending value.  The true entries are emitted in (b, i, j) order (torch.nonzero), the score of an
entry is exp(score) * global_score.  The confidence threshold is the float32 value the kernel receives."""
import numpy as np
import torch


# ------------------------------------------------------------------------------------------------------- Sinkhorn
def padded_masks(row_masks, col_masks):
    """(B, M+1), (B, N+1): True at the masked rows / columns of the padded matrix (the dustbins are never masked)."""
    B, M = row_masks.shape
    N = col_masks.shape[1]
    prm = np.zeros((B, M + 1), bool)
    prm[:, :M] = ~row_masks
    pcm = np.zeros((B, N + 1), bool)
    pcm[:, :N] = ~col_masks
    return prm, pcm


def padded(scores, rm, cm, alpha, inf, dtype=np.float64):
    """learnable_sinkhorn.py:38-61 without the masking of log_mu / log_nu: padded scores, masks, marginals, norm."""
    scores = np.asarray(scores)
    B, M, N = scores.shape
    P = np.full((B, M + 1, N + 1), alpha, dtype)
    P[:, :M, :N] = scores
    prm, pcm = padded_masks(rm, cm)
    P[prm[:, :, None] | pcm[:, None, :]] = -inf
    nvr, nvc = rm.sum(1).astype(dtype), cm.sum(1).astype(dtype)
    norm = -np.log(nvr + nvc)
    log_mu = np.empty((B, M + 1), dtype)
    log_mu[:, :M] = norm[:, None]
    log_mu[:, M] = np.log(nvc) + norm
    log_nu = np.empty((B, N + 1), dtype)
    log_nu[:, :N] = norm[:, None]
    log_nu[:, N] = np.log(nvr) + norm
    return P, prm, pcm, log_mu, log_nu, norm


def _sinkhorn(scores, row_masks, col_masks, alpha, num_iterations, inf, dtype):
    scores = np.asarray(scores)
    B, M, N = scores.shape
    rm = np.ones((B, M), bool) if row_masks is None else np.asarray(row_masks, bool)
    cm = np.ones((B, N), bool) if col_masks is None else np.asarray(col_masks, bool)
    P, prm, pcm, log_mu, log_nu, norm = padded(scores, rm, cm, alpha, inf, dtype)
    log_mu = np.where(prm, dtype(-inf), log_mu)
    log_nu = np.where(pcm, dtype(-inf), log_nu)
    P, log_mu, log_nu, norm = (torch.from_numpy(np.ascontiguousarray(a)) for a in (P, log_mu, log_nu, norm))
    u, v = torch.zeros_like(log_mu), torch.zeros_like(log_nu)
    for _ in range(num_iterations):                                    # :13-18
        u = log_mu - torch.logsumexp(P + v.unsqueeze(1), dim=2)
        v = log_nu - torch.logsumexp(P + u.unsqueeze(2), dim=1)
    out = P + u.unsqueeze(2) + v.unsqueeze(1) - norm.reshape(-1, 1, 1)  # :18, :64
    assert out.dtype == (torch.float64 if dtype is np.float64 else torch.float32)
    return out.numpy()


def sinkhorn(scores, row_masks=None, col_masks=None, alpha=1.0, num_iterations=100, inf=1e12):
    """(B, M, N) scores -> (B, M+1, N+1) float64.  Masked entries hold -inf stand-ins (about -1e12)."""
    return _sinkhorn(scores, row_masks, col_masks, alpha, num_iterations, inf, np.float64)


def sinkhorn_fp32(scores, row_masks=None, col_masks=None, alpha=1.0, num_iterations=100, inf=1e12):
    """The same iteration with every array in float32."""
    return _sinkhorn(np.asarray(scores, np.float32), row_masks, col_masks, np.float32(alpha), num_iterations, inf, np.float32)


def live_entries(shape_bmn, row_masks, col_masks):
    """(B, M+1, N+1) bool: the entries of the padded matrix on no masked row or column."""
    B, M, N = shape_bmn
    rm = np.ones((B, M), bool) if row_masks is None else np.asarray(row_masks, bool)
    cm = np.ones((B, N), bool) if col_masks is None else np.asarray(col_masks, bool)
    prm, pcm = padded_masks(rm, cm)
    return ~(prm[:, :, None] | pcm[:, None, :])


# ------------------------------------------------------------------------------------------------- correspondences
def threshold_f32(threshold):
    return float(np.float32(threshold))


def topk_mask(a, k, axis):
    """True at the k largest entries along `axis`; among equal values the lowest index (stable descending sort)."""
    order = np.argsort(-a, axis=axis, kind="stable")
    take = np.take(order, np.arange(min(k, a.shape[axis])), axis=axis)
    m = np.zeros(a.shape, bool)
    np.put_along_axis(m, take, True, axis=axis)
    return m


def correspondence_matrix(exp_scores, ref_masks, src_masks, k, mutual, threshold):
    """point_matching.py:32-66: (row top-k and > thr) AND / OR (column top-k and > thr), AND the validity mask.  The
    masks are applied after the selection: the scores of masked slots take part in the top-k of the live lines."""
    E = np.asarray(exp_scores, np.float64)
    over = E > threshold_f32(threshold)
    ref = topk_mask(E, k, 2) & over      # :40-45
    src = topk_mask(E, k, 1) & over      # :48-53
    corr = (ref & src) if mutual else (ref | src)
    return corr & (np.asarray(ref_masks, bool)[:, :, None] & np.asarray(src_masks, bool)[:, None, :])  # :64


def point_matching(ref_points, src_points, ref_masks, src_masks, ref_indices, src_indices, score_mat, global_scores, k,
                   mutual=True, threshold=0.05, use_global_score=False):
    """point_matching.py:96-115 -> (ref points, src points, ref indices, src indices, float64 scores, corr_mat, the number
    of true entries in front of each patch)."""
    E = np.exp(np.asarray(score_mat, np.float64))
    corr = correspondence_matrix(E, ref_masks, src_masks, k, mutual, threshold)
    if use_global_score:
        E = E * np.asarray(global_scores, np.float64)[:, None, None]
    b, i, j = np.nonzero(corr)           # (b, i, j) order
    counts = corr.reshape(corr.shape[0], -1).sum(1)
    offsets = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    return ref_points[b, i], src_points[b, j], ref_indices[b, i], src_indices[b, j], E[b, i, j], corr, offsets


def decision_margins(values, exp_scores, ref_masks, src_masks, k, threshold):
    """How far the decisions are from flipping.  `values`: the array whose equal BITS count as a planted tie (the float32
    input of the kernel: log scores or their exponentials); `exp_scores`: the float64 matrix that is ranked and thresholded.
    -> (gaps, ties, dist, on_thr):
      gaps   relative gap (a_k - a_(k+1)) / a_k between the k-th and the (k+1)-th value of every live line that has a
             (k+1)-th value, rows then columns, where the two are no planted tie;  ties: the number of lines where they are
      dist   |E - thr| / thr of every entry that is not exactly on the threshold (inf for thr = 0);  on_thr: their number."""
    E = np.asarray(exp_scores, np.float64)
    V = np.asarray(values)
    thr = threshold_f32(threshold)
    gaps, ties = [], 0
    for axis, live in ((2, np.asarray(ref_masks, bool)), (1, np.asarray(src_masks, bool))):
        if E.shape[axis] <= k:
            continue
        order = np.argsort(-E, axis=axis, kind="stable")
        pick = np.take(order, [k - 1, k], axis=axis)
        e = np.take_along_axis(E, pick, axis=axis)
        w = np.take_along_axis(V, pick, axis=axis)
        ek, ek1 = np.take(e, 0, axis=axis)[live], np.take(e, 1, axis=axis)[live]
        same = (np.take(w, 0, axis=axis) == np.take(w, 1, axis=axis))[live]
        ties += int(same.sum())
        gaps.append(((ek - ek1) / ek)[~same])
    on = E == thr
    with np.errstate(divide="ignore", invalid="ignore"):
        dist = np.where(thr > 0, np.abs(E - thr) / thr, np.inf)[~on]
    return (np.concatenate(gaps) if gaps else np.zeros(0)), ties, dist, int(on.sum())
