"""A float64 restatement of gaussreg_amd.normals (include/gaussreg_hip_icp_plane.h): the set of every query from its table
row, the covariance about its mean accumulated relative to the first point of the set in list order, numpy.linalg.eigh in
place of the kernel's Jacobi sweeps, the sign rule, one rounding to fp32.

normals_f64(query, support, neighbors, include_self, toward) -> dict(
    normal (N, 3) fp32, unit (N, 3) float64 (the signed normal before rounding), curvature (N,) float64, valid (N,) bool,
    lam (N, 3) float64 ascending, m (N,) the size of every set, gap (N,) = (l1 - l0) / l2, 0 where invalid)
"""
import numpy as np


def normals_f64(query, support, neighbors, include_self=False, toward=None):
    q = np.asarray(query, np.float32).astype(np.float64).reshape(-1, 3)
    s = np.asarray(support, np.float32).astype(np.float64).reshape(-1, 3)
    nb = np.asarray(neighbors, np.int64)
    N, K, M = q.shape[0], nb.shape[1], s.shape[0]
    first = np.zeros((N, 3))
    have = np.zeros(N, bool)
    m = np.zeros(N, np.int64)
    sd = np.zeros((N, 3))
    sdd = np.zeros((N, 3, 3))
    if include_self:
        first[:], have[:], m[:] = q, True, 1
    for k in range(K):                       # list order; entries outside [0, M) are padding
        j = nb[:, k]
        use = (j >= 0) & (j < M)
        p = s[np.where(use, j, 0)] if M else np.zeros((N, 3))
        take = use & ~have
        first[take] = p[take]
        have |= use
        d = np.where(use[:, None], p - first, 0.0)
        sd += d
        sdd += d[:, :, None] * d[:, None, :]
        m += use
    C = sdd - sd[:, :, None] * sd[:, None, :] / np.maximum(m, 1)[:, None, None]
    lam, vec = np.linalg.eigh(C) if N else (np.zeros((0, 3)), np.zeros((0, 3, 3)))
    valid = (m >= 3) & (lam[:, 1] > 1e-12 * lam[:, 2])
    unit = vec[:, :, 0] / np.maximum(np.linalg.norm(vec[:, :, 0], axis=1, keepdims=True), 1e-300)
    if toward is not None:
        dot = (unit * (np.asarray(toward, np.float32).astype(np.float64)[None] - q)).sum(1)
        flip = dot < 0.0
    else:
        big = np.argmax(np.abs(unit), axis=1)            # the first among equals
        flip = unit[np.arange(N), big] < 0.0
    unit = np.where(flip[:, None], -unit, unit)
    unit = np.where(valid[:, None], unit, 0.0)
    total = lam.sum(1)
    curvature = np.where(valid & (total != 0.0), lam[:, 0] / np.where(total != 0.0, total, 1.0), 0.0)
    gap = np.where(valid, (lam[:, 1] - lam[:, 0]) / np.where(lam[:, 2] > 0.0, lam[:, 2], 1.0), 0.0)
    return dict(normal=unit.astype(np.float32), unit=unit, curvature=curvature, valid=valid, lam=lam, m=m, gap=gap)

