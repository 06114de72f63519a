"""A float64 restatement of gaussreg_amd.icp (include/gaussreg_hip_icp.h) and the step-by-step replay the GPU is judged by.

transform_f32      the fp32 transform in the library's association, ((A0 x + A1 y) + A2 z) + t.
evaluate           E(T): transform_f32, then a k = 1 capped search (`knn`: cloud_nn_f64.knn_f32 here, cloud_nn.knn on the
                   GPU -- both pinned to brute force), n, S, fitness, rmse with the sums in float64.
umeyama_f64        U: the float64 Umeyama fit in SVD form from the matched pairs -> (T (3, 4) float64, scale, bound) or None
                   where the library refuses.  bound (3, 4): 4 fp32 ulps of the scale for the 3x3 block, 4 fp32 ulps of
                   |c_ref| + s |R c_src| for the translation (docs/registration_f64_errors.md).
icp_f64            the loop; every T_(t+1) is rounded once to fp32.  `variant` plants the errors the replay has to reject.
replay             the yardstick: for every recorded t, E(T_t) recomputed and compared, U(T_t) against T_(t+1) within the
                   bound, the stop decision against the rule; raises AssertionError, returns the worst error / bound.
"""
import numpy as np

import cloud_nn_f64

CONVERGED, ITERATION_LIMIT, DEGENERATE = "converged", "iteration_limit", "degenerate"
GUARD = 1e-10      # around the two thresholds: fp64 summation order; no committed case may fall inside
VARIANTS = ("wrong_association", "strict_cap", "scale_in_rigid", "stop_on_fitness_only", "composed_increments")


def transform_f32(T, src, variant=None):
    T = np.asarray(T, np.float32)
    x, y, z = (src[:, k].astype(np.float32) for k in range(3))
    out = np.empty((src.shape[0], 3), np.float32)
    for r in range(3):
        if variant == "wrong_association":
            out[:, r] = (T[r, 0] * x + (T[r, 1] * y + T[r, 2] * z)) + T[r, 3]
        else:
            out[:, r] = ((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]
    return out


def knn_numpy(query, support, cap):
    d, j = cloud_nn_f64.knn_f32(query, support, 1, cap)
    return d[:, 0], j[:, 0]


def evaluate(T, src, ref, cap, knn=knn_numpy, variant=None):
    """-> dict(j (N,) int64, d (N,) fp32, n, S, fitness, rmse)"""
    N = src.shape[0]
    if N == 0:
        return dict(j=np.zeros(0, np.int64), d=np.zeros(0, np.float32), n=0, S=0.0, fitness=0.0, rmse=0.0)
    d, j = knn(transform_f32(T, src, variant), ref, np.float32(cap))
    if variant == "strict_cap":
        j = np.where(d < np.float32(cap), j, -1)
        d = np.where(j >= 0, d, np.float32(np.inf))
    m = j >= 0
    n = int(m.sum())
    S = float(d[m].astype(np.float64).sum())
    return dict(j=j, d=d, n=n, S=S, fitness=n / N, rmse=float(np.sqrt(S / n)) if n else 0.0)


def umeyama_f64(a, b, with_scale):
    """The similarity (rigid when not with_scale) that maps the rows of a (n, 3) onto those of b, least squares, float64."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    n = a.shape[0]
    if n < 3:
        return None
    ca, cb = a.mean(0), b.mean(0)
    da, db = a - ca, b - cb
    H = da.T @ db
    U, sv, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T)) or 1.0])
    R = Vt.T @ D @ U.T
    s = 1.0
    if with_scale:
        var = (da * da).sum()
        if not var > 1e-300:
            return None
        s = float(np.trace(R @ H)) / var        # sum_i db_i . (R da_i) / sum |da_i|^2
        if not (s > 0.0 and np.isfinite(s)):
            return None
    T = np.empty((3, 4))
    T[:, :3] = s * R
    T[:, 3] = cb - s * (R @ ca)
    ulp = lambda v: float(np.spacing(np.float32(abs(v))))
    bound = np.empty((3, 4))
    bound[:, :3] = 4 * ulp(s)
    bound[:, 3] = 4 * ulp(np.linalg.norm(cb) + s * np.linalg.norm(R @ ca))
    return T, s, bound


def update(ev, src, ref, with_scale, variant=None):
    m = ev["j"] >= 0
    return umeyama_f64(src[m], ref[ev["j"][m]], with_scale or variant == "scale_in_rigid")


def decide(t, ev, prev, max_iterations, relative_fitness, relative_rmse, variant=None):
    """The stop rule before the fit: -> a status or None (go on to the fit)."""
    if t >= 1:
        df, dr = abs(ev["fitness"] - prev["fitness"]) < relative_fitness, abs(ev["rmse"] - prev["rmse"]) < relative_rmse
        if df and (dr or variant == "stop_on_fitness_only"):
            return CONVERGED
    if t == max_iterations:
        return ITERATION_LIMIT
    if ev["n"] < 3:
        return DEGENERATE
    return None


def icp_f64(src, ref, T0, max_dist, with_scale, max_iterations=30, relative_fitness=1e-6, relative_rmse=1e-6, knn=knn_numpy,
            variant=None):
    """-> dict(transform (4, 4) fp32, status, iterations, history (iterations + 1, 16) float64, j, d, fitness, rmse)"""
    cap = np.float32(float(max_dist) * float(max_dist))
    T = np.asarray(T0, np.float32)[:3].copy()
    history, prev, t = [], None, 0
    moved = src                        # composed_increments: the fp32 points every step is fitted to
    if src.shape[0] == 0:
        ev = evaluate(T, src, ref, cap, knn)
        history.append(np.concatenate([T.ravel().astype(np.float64), [0, 0.0, 0.0, 0.0]]))
        status = DEGENERATE
    while src.shape[0]:
        ev = evaluate(T, src, ref, cap, knn, variant)
        history.append(np.concatenate([T.ravel().astype(np.float64), [ev["n"], ev["S"], ev["fitness"], ev["rmse"]]]))
        status = decide(t, ev, prev, max_iterations, relative_fitness, relative_rmse, variant)
        if status:
            break
        if variant == "composed_increments":
            moved = transform_f32(T, src)
            m = ev["j"] >= 0
            fit = umeyama_f64(moved[m], ref[ev["j"][m]], with_scale)
        else:
            fit = update(ev, src, ref, with_scale, variant)
        if fit is None:
            status = DEGENERATE
            break
        Tn = fit[0]
        if variant == "composed_increments":       # T <- increment o T, formed in fp32
            inc, cur = np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32)
            inc[:3], cur[:3] = Tn.astype(np.float32), T
            Tn = (inc @ cur)[:3]
        T, prev, t = Tn.astype(np.float32), ev, t + 1
    full = np.eye(4, dtype=np.float32)
    full[:3] = T
    return dict(transform=full, status=status, iterations=t, history=np.array(history), j=ev["j"], d=ev["d"],
                fitness=ev["fitness"], rmse=ev["rmse"])


def replay(src, ref, with_scale, max_dist, max_iterations, relative_fitness, relative_rmse, history, status, iterations,
           knn=knn_numpy, echo=None):
    """Judge a recorded run (history rows: T_t[12], n, S, fitness, rmse) step by step; -> worst |T_(t+1) - U(T_t)| / bound."""
    cap = np.float32(float(max_dist) * float(max_dist))
    history = np.asarray(history, np.float64)
    assert history.shape == (iterations + 1, 16), (history.shape, iterations)
    N, worst, prev = src.shape[0], 0.0, None
    rel = lambda a, b: abs(a - b) <= 1e-12 * max(abs(a), abs(b))
    for t in range(iterations + 1):
        T = history[t, :12].reshape(3, 4)
        assert (T == T.astype(np.float32)).all(), f"T_{t} is not fp32"
        ev = evaluate(T, src, ref, cap, knn)
        n, S, fitness, rmse = history[t, 12:]
        assert n == ev["n"], (t, n, ev["n"])
        assert rel(S, ev["S"]) and rel(fitness, ev["fitness"]) and rel(rmse, ev["rmse"]), (t, history[t, 12:], ev["S"], ev["fitness"], ev["rmse"])
        if t >= 1 and N:     # no iteration may sit inside the guard band of a threshold
            for now, before, tol in ((ev["fitness"], prev["fitness"], relative_fitness), (ev["rmse"], prev["rmse"], relative_rmse)):
                assert tol == 0.0 or abs(abs(now - before) - tol) > GUARD, (t, now, before, tol)   # tol 0: never below it
        want = DEGENERATE if N == 0 else decide(t, ev, prev, max_iterations, relative_fitness, relative_rmse)
        fit = update(ev, src, ref, with_scale) if want is None else None
        if want is None and fit is None:
            want = DEGENERATE
        if t < iterations:
            assert want is None, f"the rule stops at t = {t} ({want}), the run went on to {iterations}"
            err = np.abs(history[t + 1, :12].reshape(3, 4) - fit[0]) / fit[2]
            worst = max(worst, float(err.max()))
            if echo:
                echo(f"t = {t}: n = {ev['n']} rmse = {ev['rmse']:.6g} |T' - U(T)| / bound = {err.max():.3f}")
            assert err.max() <= 1.0, (t, err)
        elif status == DEGENERATE and want is None:
            # the library refused a fit that float64 accepts: only where the spread is at rounding level (collinear sets)
            raise AssertionError(f"degenerate at t = {t}, float64 fits it")
        else:
            assert want == status, (t, want, status)
        prev = ev
    return worst


def errors(T, T_gt):
    """-> (rotation angle in degrees, translation distance, |scale ratio - 1|) of T against T_gt"""
    T, T_gt = np.asarray(T, np.float64), np.asarray(T_gt, np.float64)
    s, sg = np.cbrt(np.linalg.det(T[:3, :3])), np.cbrt(np.linalg.det(T_gt[:3, :3]))
    R = (T[:3, :3] / s) @ (T_gt[:3, :3] / sg).T
    angle = np.degrees(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0)))
    return float(angle), float(np.linalg.norm(T[:3, 3] - T_gt[:3, 3])), float(abs(s / sg - 1.0))
