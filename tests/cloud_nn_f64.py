"""Brute-force restatements of gaussreg_amd.cloud_nn for the tests: every (query, support) pair, the order (d, j), nothing
excluded, rows padded with +inf / -1 where fewer than k points qualify.

knn_f64          float64, numpy: the definition.
knn_f32          fp32 numpy in the library's association ((dx*dx + dy*dy) + dz*dz, dx = s[j].x - q[i].x): what the kernels
                 must reproduce bit for bit.
knn_f32_torch    the same in torch, row chunks, on whatever device the clouds are on.
pairs_f32 / pairs_f32_torch / pairs_f64   every (i, j) with d <= r2, ordered by (i, j).
knn_loop / pairs_loop   the definition as a per-query Python loop (tiny clouds), float64 or an fp32 association.
The reference's registration.py functions in float64: *_f64.
Each selection takes k rounds of "smallest value, lowest index among equals", so ties cost nothing.
"""
import math

import numpy as np
import torch


def r2_of(radius):
    """The fp32 number a radius enters the library as."""
    return np.float32(float(radius) * float(radius))


def _dist_numpy(q, s):
    dx = s[None, :, 0] - q[:, None, 0]
    dy = s[None, :, 1] - q[:, None, 1]
    dz = s[None, :, 2] - q[:, None, 2]
    return (dx * dx + dy * dy) + dz * dz


def _knn_numpy(q, s, k, cap, chunk):
    nq = q.shape[0]
    dist = np.full((nq, k), np.inf, q.dtype)
    index = np.full((nq, k), -1, np.int64)
    for b in range(0, nq, chunk):
        d = _dist_numpy(q[b:b + chunk], s)
        ok = d <= cap
        r = np.arange(d.shape[0])
        masked = np.where(ok, d, np.inf)
        for t in range(min(k, s.shape[0])):
            j = np.argmin(masked, axis=1)  # the first occurrence: the lowest index among equals
            # a row without a qualifying point left: argmin of all-inf is 0, and ok[r, 0] is False by now
            have = ok[r, j]
            dist[b:b + chunk, t] = np.where(have, d[r, j], np.inf)
            index[b:b + chunk, t] = np.where(have, j, -1)
            ok[r, j] = False
            masked[r, j] = np.inf
    return dist, index


def knn_f64(query, support, k, max_dist2=np.inf, chunk=512):
    return _knn_numpy(np.asarray(query, np.float64), np.asarray(support, np.float64), k, float(max_dist2), chunk)


def knn_f32(query, support, k, max_dist2=np.inf, chunk=512):
    q, s = np.asarray(query), np.asarray(support)
    assert q.dtype == np.float32 and s.dtype == np.float32
    return _knn_numpy(q, s, k, np.float32(max_dist2), chunk)


def _dist_torch(q, s):
    dx = s[None, :, 0] - q[:, None, 0]
    dy = s[None, :, 1] - q[:, None, 1]
    dz = s[None, :, 2] - q[:, None, 2]
    dx = dx * dx
    dy = dy * dy
    dz = dz * dz
    d = dx + dy
    return d + dz


def knn_f32_torch(query, support, k, max_dist2=math.inf, chunk=1024):
    """fp32 tensors on any device -> (dist2, index) on that device, the bits of knn_f32."""
    assert query.dtype == torch.float32 and support.dtype == torch.float32
    nq, ns, dev = query.shape[0], support.shape[0], query.device
    dist = torch.full((nq, k), math.inf, dtype=torch.float32, device=dev)
    index = torch.full((nq, k), -1, dtype=torch.int64, device=dev)
    cols = torch.arange(ns, device=dev)
    cap = torch.tensor(max_dist2, dtype=torch.float32, device=dev)
    for b in range(0, nq, chunk):
        d = _dist_torch(query[b:b + chunk], support)
        ok = d <= cap
        r = torch.arange(d.shape[0], device=dev)
        for t in range(min(k, ns)):
            m = torch.where(ok, d, math.inf).min(dim=1).values
            j = torch.where(ok & (d == m[:, None]), cols[None, :], ns).min(dim=1).values  # the lowest index among equals
            have = j < ns
            jj = torch.where(have, j, 0)
            dist[b:b + chunk, t] = torch.where(have, d[r, jj], math.inf)
            index[b:b + chunk, t] = torch.where(have, j, -1)
            ok[r[have], j[have]] = False
    return dist, index


def pairs_f32_torch(query, support, r2, chunk=1024):
    assert query.dtype == torch.float32 and support.dtype == torch.float32
    cap = torch.tensor(float(r2), dtype=torch.float32, device=query.device)
    out = [torch.zeros((0, 2), dtype=torch.int64, device=query.device)]
    for b in range(0, query.shape[0], chunk):
        hit = torch.nonzero(_dist_torch(query[b:b + chunk], support) <= cap)  # row-major: (i, j) ascending
        hit[:, 0] += b
        out.append(hit)
    return torch.cat(out)


def _pairs_numpy(q, s, cap, chunk):
    out = [np.zeros((0, 2), np.int64)]
    for b in range(0, q.shape[0], chunk):
        hit = np.argwhere(_dist_numpy(q[b:b + chunk], s) <= cap).astype(np.int64)
        hit[:, 0] += b
        out.append(hit)
    return np.concatenate(out)


def pairs_f32(query, support, r2, chunk=512):
    q, s = np.asarray(query), np.asarray(support)
    assert q.dtype == np.float32 and s.dtype == np.float32
    return _pairs_numpy(q, s, np.float32(r2), chunk)


def pairs_f64(query, support, r2, chunk=512):
    return _pairs_numpy(np.asarray(query, np.float64), np.asarray(support, np.float64), float(r2), chunk)


def _loop_dist(a, b, dtype):
    dx, dy, dz = (dtype(b[c]) - dtype(a[c]) for c in range(3))
    return dtype(dtype(dtype(dx * dx) + dtype(dy * dy)) + dtype(dz * dz))


def knn_loop(query, support, k, max_dist2=math.inf, dtype=np.float64):
    """Per query: sort every qualifying (d, j), take k, pad."""
    dist, index = [], []
    for a in query:
        cand = sorted((_loop_dist(a, b, dtype), j) for j, b in enumerate(support))
        cand = [c for c in cand if c[0] <= dtype(max_dist2)][:k]
        dist.append([c[0] for c in cand] + [np.inf] * (k - len(cand)))
        index.append([c[1] for c in cand] + [-1] * (k - len(cand)))
    return np.array(dist, dtype=dtype).reshape(len(query), k), np.array(index, dtype=np.int64).reshape(len(query), k)


def pairs_loop(query, support, r2, dtype=np.float64):
    out = [(i, j) for i, a in enumerate(query) for j, b in enumerate(support) if _loop_dist(a, b, dtype) <= dtype(r2)]
    return np.array(out, dtype=np.int64).reshape(len(out), 2)


# ---- geotransformer/utils/registration.py in float64, brute force where the reference asks a k-d tree -----------------------

def apply_transform_f64(points, transform):
    t = np.asarray(transform, np.float64)
    return np.asarray(points, np.float64) @ t[:3, :3].T + t[:3, 3]


def nearest_f64(query, support):
    d, j = knn_f64(query, support, 1)
    return np.sqrt(d[:, 0]), j[:, 0]


def overlap_f64(ref, src, transform=None, positive_radius=0.1):
    src = np.asarray(src, np.float64) if transform is None else apply_transform_f64(src, transform)
    return float(np.mean(nearest_f64(ref, src)[0] < positive_radius))


def correspondences_f64(ref, src, transform, matching_radius):
    """-> (pairs ordered by (i, j), d (nq, ns) float64 squared distances for the margin checks)."""
    src = apply_transform_f64(src, transform)
    return pairs_f64(ref, src, matching_radius * matching_radius), _dist_numpy(np.asarray(ref, np.float64), src)


def chamfer_f64(raw, ref, src, gt_transform, est_transform):
    est, gt = np.asarray(est_transform, np.float64), np.asarray(gt_transform, np.float64)
    p_q = nearest_f64(apply_transform_f64(src, est), raw)[0].mean()
    q_p = nearest_f64(ref, apply_transform_f64(raw, est @ np.linalg.inv(gt)))[0].mean()
    return float(p_q + q_p)


def residuals_f64(ref_corr, src_corr, transform):
    return np.sqrt(((np.asarray(ref_corr, np.float64) - apply_transform_f64(src_corr, transform)) ** 2).sum(1))


def rmse_f64(src, gt_transform, est_transform):
    return float(np.linalg.norm(apply_transform_f64(src, gt_transform) - apply_transform_f64(src, est_transform), axis=1).mean())
