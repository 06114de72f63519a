"""Test helper (not collected): float64 restatements of KPConv.forward (geotransformer/modules/kpconv/kpconv.py:90-120)
and RPEMultiHeadAttention.forward (geotransformer/modules/transformer/rpe_transformer.py:34-72), written from the
reference's formulas in the reference's association, in plain NumPy.  tests/test_kpconv_rpe_f64_reference.py pins both
against outputs the reference itself produced; the GPU path tests compare the HIP kernels with them.

`dtype` evaluates the same formulas in another precision (float32: the "reference's own rounding error" side of
helpers.assert_as_exact_as_reference).  Nothing here shares code with gaussreg_amd or oracle/.
"""
import numpy as np


def kpconv_f64(s_feats, q_points, s_points, neighbor_indices, kernel_points, weights, sigma, bias=None, inf=1e6,
               rows_per_chunk=None):
    """gather -> (M,K,H) x (M,H,C) -> (K,M,C) x (K,C,O) summed over K -> / max(num, 1) -> + bias, all in float64; the
    neighbour flag `sum_c feats > 0` is evaluated in float64 too.  Query rows are independent, so they are processed in
    chunks (memory only; the arithmetic of a row does not depend on the chunking)."""
    f64 = np.float64
    feats = np.concatenate([np.asarray(s_feats, f64), np.zeros((1, s_feats.shape[1]), f64)], 0)      # shadow row: zeros
    pts = np.concatenate([np.asarray(s_points, f64).reshape(-1, 3), np.full((1, 3), inf, f64)], 0)   # shadow point: +inf
    q = np.asarray(q_points, f64)
    nbr = np.asarray(neighbor_indices, np.int64)
    kp = np.asarray(kernel_points, f64)
    w = np.asarray(weights, f64)
    M, H = nbr.shape
    K, C, O = w.shape
    out = np.zeros((M, O), f64)
    if rows_per_chunk is None:
        rows_per_chunk = max(1, int(4e6 // max(1, H * max(C, 3 * K))))
    for r0 in range(0, M, rows_per_chunk):
        idx = nbr[r0:r0 + rows_per_chunk]
        nb = pts[idx] - q[r0:r0 + rows_per_chunk, None, :]                         # (m, H, 3)
        diff = nb[:, :, None, :] - kp[None, None]                                  # (m, H, K, 3)
        infl = np.maximum(1.0 - np.sqrt((diff ** 2).sum(3)) / sigma, 0.0)          # (m, H, K)
        nf = feats[idx]                                                            # (m, H, C)
        wf = np.matmul(infl.transpose(0, 2, 1), nf)                                # (m, K, C)
        o = np.matmul(wf.transpose(1, 0, 2), w).sum(0)                             # (K, m, O) -> (m, O)
        num = np.maximum((nf.sum(-1) > 0.0).sum(-1), 1)
        out[r0:r0 + rows_per_chunk] = o / num[:, None]
    if bias is not None:
        out = out + np.asarray(bias, f64)
    return out


def _linear(x, sd, name, dtype):
    return x @ np.asarray(sd[name + ".weight"], dtype).T + np.asarray(sd[name + ".bias"], dtype)


def rpe_attention_f64(state_dict, q, k, v, emb, key_weights=None, key_masks=None, attention_factors=None, *, num_heads,
                      dtype=np.float64, return_logits=False):
    """One batch element: q (N,C), k / v (M,C), emb (N,M,C), key_weights (M), key_masks (M; True = ignored),
    attention_factors (N,M).  The embedding is projected through proj_p FIRST and then contracted with q, as the reference
    does.  Returns hidden (N,C), softmax scores (H,N,M) and the positional term q . p alone (H,N,M).
    A fully masked row gives NaN, as softmax over a row of -inf does.  `return_logits` appends the scores as they enter the
    softmax (H,N,M)."""
    sd = {n: np.asarray(t) for n, t in state_dict.items()}
    h = num_heads
    q, k, v, emb = (np.asarray(a, dtype) for a in (q, k, v, emb))
    n, c = q.shape
    m = k.shape[0]
    ch = c // h
    qp = _linear(q, sd, "proj_q", dtype).reshape(n, h, ch).transpose(1, 0, 2)      # (H, N, ch)
    kp = _linear(k, sd, "proj_k", dtype).reshape(m, h, ch).transpose(1, 0, 2)      # (H, M, ch)
    vp = _linear(v, sd, "proj_v", dtype).reshape(m, h, ch).transpose(1, 0, 2)
    pp = _linear(emb.reshape(n * m, c), sd, "proj_p", dtype).reshape(n, m, h, ch).transpose(2, 0, 1, 3)  # (H, N, M, ch)
    s_p = np.matmul(pp, qp[:, :, :, None])[..., 0]                                 # (H, N, M): sum_c q[h,n,c] p[h,n,m,c]
    s_e = np.matmul(qp, kp.transpose(0, 2, 1))                                     # (H, N, M)
    s = (s_e + s_p) / np.asarray(ch, dtype) ** np.asarray(0.5, dtype)
    if attention_factors is not None:
        s = np.asarray(attention_factors, dtype)[None] * s
    if key_weights is not None:
        s = s * np.asarray(key_weights, dtype)[None, None, :]
    if key_masks is not None:
        s = np.where(np.asarray(key_masks).astype(bool)[None, None, :], np.asarray(-np.inf, dtype), s)
    with np.errstate(invalid="ignore"):
        e = np.exp(s - s.max(-1, keepdims=True))
        p = e / e.sum(-1, keepdims=True)
    hidden = np.matmul(p, vp).transpose(1, 0, 2).reshape(n, c)
    out = (hidden.astype(dtype), p.astype(dtype), s_p.astype(dtype))
    return out + (s,) if return_logits else out
