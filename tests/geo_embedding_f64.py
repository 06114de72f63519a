"""Test helper (not collected): GeometricStructureEmbedding restated in NumPy with a `dtype` argument.

Written from the reference's formulas (geotransformer.py:26-73, pairwise_distance.py:21-31, positional_embedding.py:25-32)
in the reference's association; it shares no code with gaussreg_amd or oracle/.  In float64 it is the exact answer the
GPU tests compare with, in float32 it is the reference's own rounding.  The parameters (weights, biases, div_term) are the
fp32 values the module holds, widened to `dtype`: both sides evaluate the same function.

Two choices the formulas leave open are made here the way the HIP kernel documents them:
  * ties in the neighbour sort: ascending distance, lowest index first (a stable sort), the first entry dropped;
  * angle_k = 0 (the reference's max / mean over an empty axis is undefined): the angular term is 0.
tests/test_geo_embedding_f64_reference.py pins everything else against the reference module itself in float64.
"""
import numpy as np


def squared_distances(points, dtype):
    """pairwise_distance.py:23-30: xy by matmul, x2 - 2 xy + y2, clamped at 0."""
    p = np.asarray(points, dtype)
    xy = p @ p.T
    x2 = np.sum(p * p, axis=1)
    return np.maximum(x2[:, None] - dtype(2) * xy + x2[None, :], dtype(0))


def embedding_indices(points, sigma_d, sigma_a, k, dtype):
    """geotransformer.py:38-53 for one cloud (N, 3) -> d_indices (N, N), a_indices (N, N, k), knn (N, k)."""
    p = np.asarray(points, dtype)
    n = p.shape[0]
    dist = np.sqrt(squared_distances(p, dtype))
    d_idx = dist / dtype(sigma_d)
    knn = np.argsort(dist, axis=1, kind="stable")[:, 1:k + 1]                  # (N, k)
    ref = p[knn] - p[:, None, :]                                               # (N, k, 3)
    anc = p[None, :, :] - p[:, None, :]                                        # (N, N, 3): anc[a, b] = p[b] - p[a]
    r = np.broadcast_to(ref[:, None, :, :], (n, n, k, 3))
    a = np.broadcast_to(anc[:, :, None, :], (n, n, k, 3))
    cr = np.stack([r[..., 1] * a[..., 2] - r[..., 2] * a[..., 1], r[..., 2] * a[..., 0] - r[..., 0] * a[..., 2],
                   r[..., 0] * a[..., 1] - r[..., 1] * a[..., 0]], axis=-1)
    sin = np.sqrt((cr[..., 0] * cr[..., 0] + cr[..., 1] * cr[..., 1]) + cr[..., 2] * cr[..., 2])
    pr = r * a
    cos = ((dtype(0) + pr[..., 0]) + pr[..., 1]) + pr[..., 2]                  # torch.sum starts from +0: (-0) + ... -> +0
    factor_a = 180.0 / (sigma_a * np.pi)
    a_idx = np.arctan2(sin, cos) * dtype(factor_a)
    return d_idx.astype(dtype), a_idx.astype(dtype), knn


def project(idx, div, w, b, dtype):
    """positional_embedding.py:25-32 then nn.Linear: idx (...) -> (..., C)."""
    om = np.asarray(idx, dtype)[..., None] * np.asarray(div, dtype)
    emb = np.stack([np.sin(om), np.cos(om)], axis=-1).reshape(*om.shape[:-1], -1)   # (sin, cos) interleaved
    return emb @ np.asarray(w, dtype).T + np.asarray(b, dtype)


def embedding(points, params, sigma_d, sigma_a, k, reduction, dtype, chunk_bytes=1 << 27):
    """points (N, 3), params = dict(w_d, b_d, w_a, b_a, div) -> (N, N, C) in `dtype`, rows evaluated in chunks."""
    assert reduction in ("max", "mean")
    d_idx, a_idx, _ = embedding_indices(points, sigma_d, sigma_a, k, dtype)
    n, c = d_idx.shape[0], np.asarray(params["w_d"]).shape[0]
    out = np.empty((n, n, c), dtype)
    rows = max(1, int(chunk_bytes // max(1, n * max(k, 1) * c * 8)))
    for a0 in range(0, n, rows):
        s = slice(a0, min(n, a0 + rows))
        d = project(d_idx[s], params["div"], params["w_d"], params["b_d"], dtype)
        if k == 0:
            out[s] = d
            continue
        a = project(a_idx[s], params["div"], params["w_a"], params["b_a"], dtype)   # (rows, N, k, C)
        a = a.max(axis=2) if reduction == "max" else a.sum(axis=2, dtype=dtype) / dtype(k)
        out[s] = d + a
    return out
