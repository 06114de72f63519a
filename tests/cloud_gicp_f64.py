"""A float64 restatement of gaussreg_amd.icp.icp_generalized (include/gaussreg_hip_gicp.h) and the step-by-step replay the GPU
is judged by.  Evaluation, the fp32 transform and the stop rule are those of tests/cloud_icp_f64.py, the Euler rotation, the
eigen solve, the 4-ulp bound and the JUDGED floor those of tests/cloud_icp_plane_f64.py, imported.

full               (n, 6) upper triangles xx, xy, xz, yy, yz, zz -> (n, 3, 3) symmetric float64.
system             (H (6, 6), g (6,), singular (n,) bool) of the matched pairs: p = transform_f32(T, src), d = p - q,
                   M = Ct + A Cs A^T with A the 3x3 block of the fp32 T, W = M^-1, J = [-[p]x, I]; H = sum J^T W J,
                   g = sum J^T W d over the pairs with det M > 1e-12 (trace M / 3)^3.  The definition, as the header writes it.
rows               the same system in Open3D's written form, rows W^(1/2) J and residuals W^(1/2) d, for the eigen solve of
                   cloud_icp_plane_f64 (tests/test_cloud_gicp_reference.py: the two agree to 1e-12).
gicp_update        U: (T' (3, 4) float64 = dT . double(T), bound (3, 4), ratio) or (None, None, ratio), as plane_update.
icp_gicp_f64       the loop; every T_(t+1) is rounded once to fp32.  `variant` plants the errors the replay has to reject.
replay             for every recorded t: E(T_t) recomputed and compared, the stop decision against the rule, T_(t+1) against
                   gicp_update within the bound; raises AssertionError, returns (worst error / bound, smallest judged ratio).
covariances_from_normals_f64, gs_covariances_f64     the twins of csrc/cloud_covariances.hip, float64 throughout.
"""
import numpy as np

from cloud_icp_f64 import CONVERGED, DEGENERATE, GUARD, decide, evaluate, knn_numpy, transform_f32  # noqa: F401
from cloud_icp_plane_f64 import JUDGED, REFUSE, euler, solve

MIN_PAIRS = 3
SINGULAR = 1e-12        # a pair with det M <= SINGULAR (trace M / 3)^3 steers nothing
VARIANTS = ("source_cov_not_rotated", "source_cov_rotated_by_transpose", "reference_cov_only", "m_for_its_inverse",
            "x_not_negated", "wrong_order", "untransformed_source", "singular_not_counted")


def full(c6):
    c6 = np.asarray(c6, np.float64)
    out = np.empty(c6.shape[:-1] + (3, 3))
    for (r, c), k in zip(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)), range(6)):
        out[..., r, c] = out[..., c, r] = c6[..., k]
    return out


def cross_matrix(p):
    K = np.zeros(p.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0] = -p[..., 2], p[..., 1], p[..., 2]
    K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -p[..., 0], -p[..., 1], p[..., 0]
    return K


def pairs(T, src, ref, src_cov, ref_cov, ev, variant=None):
    """-> (p, d (n, 3), M (n, 3, 3), regular (n,) bool) of the matched pairs, float64."""
    m = ev["j"] >= 0
    moved = src[m].astype(np.float32) if variant == "untransformed_source" else transform_f32(T, src[m])
    p, q = moved.astype(np.float64), ref[ev["j"][m]].astype(np.float64)
    A = np.asarray(T, np.float32).astype(np.float64)[:3, :3]
    Cs, Ct = full(src_cov[m]), full(ref_cov[ev["j"][m]])
    if variant == "source_cov_not_rotated":
        M = Ct + Cs
    elif variant == "source_cov_rotated_by_transpose":
        M = Ct + A.T @ Cs @ A
    elif variant == "reference_cov_only":
        M = Ct.copy()
    else:
        M = Ct + A @ Cs @ A.T
    s = np.trace(M, axis1=1, axis2=2) / 3.0
    with np.errstate(invalid="ignore"):
        regular = np.linalg.det(M) > SINGULAR * s ** 3
    return p, p - q, M, regular


def system(T, src, ref, src_cov, ref_cov, ev, variant=None):
    p, d, M, regular = pairs(T, src, ref, src_cov, ref_cov, ev, variant)
    p, d, M = p[regular], d[regular], M[regular]
    W = M if variant == "m_for_its_inverse" else np.linalg.inv(M) if len(M) else M
    J = np.concatenate([-cross_matrix(p), np.broadcast_to(np.eye(3), (len(p), 3, 3))], axis=2)      # (n, 3, 6)
    JW = np.einsum("nij,nik->njk", J, W)                                                           # J^T W: (n, 6, 3)
    return np.einsum("nij,njk->ik", JW, J), np.einsum("nij,nj->i", JW, d), ~regular


def rows(T, src, ref, src_cov, ref_cov, ev, variant=None):
    """Open3D's written form, what cloud_icp_plane_f64.solve takes: (A (3 n, 6), r (3 n,)) with three rows W^(1/2) J and
    three residuals W^(1/2) d per regular pair, W^(1/2) the symmetric root by eigh; A^T A = H and A^T r = g of `system`."""
    p, d, M, regular = pairs(T, src, ref, src_cov, ref_cov, ev, variant)
    p, d, M = p[regular], d[regular], M[regular]
    if not len(M):
        return np.zeros((0, 6)), np.zeros(0)
    lam, V = np.linalg.eigh(M if variant == "m_for_its_inverse" else np.linalg.inv(M))
    half = np.einsum("nij,nj,nkj->nik", V, np.sqrt(lam), V)
    J = np.concatenate([-cross_matrix(p), np.broadcast_to(np.eye(3), (len(p), 3, 3))], axis=2)
    return (half @ J).reshape(-1, 6), np.einsum("nij,nj->ni", half, d).ravel()


def gicp_update(T, src, ref, src_cov, ref_cov, ev, variant=None):
    x, ratio = solve(*rows(T, src, ref, src_cov, ref_cov, ev, variant), variant)
    if x is None:
        return None, None, ratio
    d, cur = np.eye(4), np.eye(4)
    d[:3, :3], d[:3, 3] = euler(*x[:3]), x[3:]
    cur[:3] = np.asarray(T, np.float32).astype(np.float64)
    Tn = ((cur @ d) if variant == "wrong_order" else (d @ cur))[:3]
    if not np.isfinite(Tn).all():
        return None, None, ratio
    ulp = lambda v: float(np.spacing(np.float32(abs(v))))
    bound = np.empty((3, 4))
    bound[:, :3] = 4 * ulp(1.0)
    bound[:, 3] = 4 * ulp(np.linalg.norm(x[3:]) + np.linalg.norm(cur[:3, 3]))
    return Tn, bound, ratio


def decide_gicp(t, ev, prev, max_iterations, relative_fitness, relative_rmse):
    """The point-to-point rule; its floor of three pairs is this estimator's as well."""
    status = decide(t, ev, prev, max_iterations, relative_fitness, relative_rmse)
    return DEGENERATE if status is None and ev["n"] < MIN_PAIRS else status


def _evaluate(T, src, ref, src_cov, ref_cov, cap, knn, variant):
    ev = evaluate(T, src, ref, cap, knn)
    if variant == "singular_not_counted" and ev["n"]:
        regular = pairs(T, src, ref, src_cov, ref_cov, ev)[3]
        j = ev["j"].copy()
        j[np.flatnonzero(j >= 0)[~regular]] = -1
        d = np.where(j >= 0, ev["d"], np.float32(np.inf))
        n = int((j >= 0).sum())
        S = float(d[j >= 0].astype(np.float64).sum())
        ev = dict(j=j, d=d, n=n, S=S, fitness=n / src.shape[0], rmse=float(np.sqrt(S / n)) if n else 0.0)
    return ev


def icp_gicp_f64(src, ref, src_cov, ref_cov, T0, max_dist, max_iterations=30, relative_fitness=1e-6, relative_rmse=1e-6,
                 knn=knn_numpy, variant=None):
    """-> dict(transform (4, 4) fp32, status, iterations, history (iterations + 1, 16) float64, j, d, fitness, rmse, ratios)"""
    cap = np.float32(float(max_dist) * float(max_dist))
    T = np.asarray(T0, np.float32)[:3].copy()
    history, ratios, prev, t = [], [], None, 0
    while True:
        ev = _evaluate(T, src, ref, src_cov, ref_cov, cap, knn, variant)
        history.append(np.concatenate([T.ravel().astype(np.float64), [ev["n"], ev["S"], ev["fitness"], ev["rmse"]]]))
        status = DEGENERATE if src.shape[0] == 0 else decide_gicp(t, ev, prev, max_iterations, relative_fitness, relative_rmse)
        if status:
            break
        Tn, _, ratio = gicp_update(T, src, ref, src_cov, ref_cov, ev, variant)
        ratios.append(ratio)
        if Tn is None:
            status = DEGENERATE
            break
        T, prev, t = Tn.astype(np.float32), ev, t + 1
    whole = np.eye(4, dtype=np.float32)
    whole[:3] = T
    return dict(transform=whole, status=status, iterations=t, history=np.array(history), j=ev["j"], d=ev["d"],
                fitness=ev["fitness"], rmse=ev["rmse"], ratios=ratios)


def replay(src, ref, src_cov, ref_cov, max_dist, max_iterations, relative_fitness, relative_rmse, history, status, iterations,
           knn=knn_numpy, echo=None):
    """Judge a recorded run (history rows: T_t[12], n, S, fitness, rmse) step by step; -> (worst |T_(t+1) - U(T_t)| / bound,
    the smallest l_min / l_max of a judged step, 1.0 if none)."""
    cap = np.float32(float(max_dist) * float(max_dist))
    history = np.asarray(history, np.float64)
    assert history.shape == (iterations + 1, 16), (history.shape, iterations)
    N, worst, lowest, prev = src.shape[0], 0.0, 1.0, None
    rel = lambda a, b: abs(a - b) <= 1e-12 * max(abs(a), abs(b))
    for t in range(iterations + 1):
        T = history[t, :12].reshape(3, 4)
        assert (T == T.astype(np.float32)).all(), f"T_{t} is not fp32"
        ev = evaluate(T, src, ref, cap, knn)
        n, S, fitness, rmse = history[t, 12:]
        assert n == ev["n"], (t, n, ev["n"])
        assert rel(S, ev["S"]) and rel(fitness, ev["fitness"]) and rel(rmse, ev["rmse"]), (t, history[t, 12:], ev["S"], ev["fitness"], ev["rmse"])
        if t >= 1 and N:     # no iteration may sit inside the guard band of a stop threshold
            for now, before, tol in ((ev["fitness"], prev["fitness"], relative_fitness), (ev["rmse"], prev["rmse"], relative_rmse)):
                assert tol == 0.0 or abs(abs(now - before) - tol) > GUARD, (t, now, before, tol)
        want = DEGENERATE if N == 0 else decide_gicp(t, ev, prev, max_iterations, relative_fitness, relative_rmse)
        Tn = bound = None
        if want is None:      # n >= 3 is a comparison of integers; the eigenvalue test gets a guard band of a factor 10
            Tn, bound, ratio = gicp_update(T, src, ref, src_cov, ref_cov, ev)
            assert not REFUSE / 10 <= ratio <= REFUSE * 10, f"t = {t}: l_min / l_max = {ratio:.3g} is within a factor 10 of {REFUSE}"
            if Tn is None:
                want = DEGENERATE
        if t < iterations:
            assert want is None, f"the rule stops at t = {t} ({want}), the run went on to {iterations}"
            assert ratio >= JUDGED, f"t = {t}: l_min / l_max = {ratio:.3g} < {JUDGED}, the bound does not hold for this step"
            err = np.abs(history[t + 1, :12].reshape(3, 4) - Tn) / bound
            worst, lowest = max(worst, float(err.max())), min(lowest, ratio)
            if echo:
                echo(f"t = {t}: n = {ev['n']} rmse = {ev['rmse']:.6g} l_min / l_max = {ratio:.3g} |T' - U(T)| / bound = {err.max():.3f}")
            assert err.max() <= 1.0, (t, err)
        else:
            assert want == status, (t, want, status)
        prev = ev
    return worst, lowest


def covariances_from_normals_f64(normals, epsilon=1e-3):
    """-> (n, 6) float64: I - (1 - epsilon) v v^T, v = n / |n|; |n| = 0 -> I."""
    v = np.asarray(normals, np.float32).astype(np.float64)
    nn = np.sqrt((v * v).sum(1))
    with np.errstate(invalid="ignore", divide="ignore"):
        v = np.where(nn[:, None] != 0.0, v / nn[:, None], 0.0)
    k = np.where(nn != 0.0, 1.0 - epsilon, 0.0)
    out = np.empty((len(v), 6))
    for e, (r, c) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        out[:, e] = (1.0 if r == c else 0.0) - k * v[:, r] * v[:, c]
    return out


def quaternion_matrix(q):
    """R of unit quaternions (r, x, y, z): the rasterizer's convention."""
    r, x, y, z = (q[:, k] for k in range(4))
    R = np.empty((len(q), 3, 3))
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = 2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = 2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)
    return R


def gs_covariances_f64(scales, rotations, scale_modifier=1.0, mode="plane", epsilon=1e-3):
    """-> dict(cov (n, 6), normal (n, 3), valid (n,) bool), float64.  "raw": R S^2 R^T from the rotation AS GIVEN (the
    rasterizer does not normalise it); "plane": the prior about the axis of the smallest scale of R(q / |q|)."""
    sc = np.asarray(scales, np.float32).astype(np.float64)
    q = np.asarray(rotations, np.float32).astype(np.float64)
    n = len(sc)
    qn = np.sqrt((q * q).sum(1))
    valid = qn != 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        qh = np.where(valid[:, None], q / qn[:, None], 0.0)
    axis = np.argmin(sc, axis=1)                                   # the first among equals
    v = quaternion_matrix(qh)[np.arange(n), :, axis]
    with np.errstate(invalid="ignore", divide="ignore"):
        v = np.where(valid[:, None], v / np.sqrt((v * v).sum(1))[:, None], 0.0)
    big = v[np.arange(n), np.argmax(np.abs(v), axis=1)]            # the first among equals
    normal = np.where((big < 0.0)[:, None], -v, v)
    if mode == "raw":
        M = quaternion_matrix(q) * (scale_modifier * sc)[:, None, :]
        S = M @ M.transpose(0, 2, 1)
        cov = np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], axis=1)
    else:
        cov = covariances_from_normals_f64(np.zeros((n, 3)), epsilon)
        k = np.where(valid, 1.0 - epsilon, 0.0)
        for e, (r, c) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            cov[:, e] = (1.0 if r == c else 0.0) - k * v[:, r] * v[:, c]
    return dict(cov=cov, normal=normal, valid=valid)
