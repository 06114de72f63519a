/* gaussreg_hip_icp.h -- point-to-point ICP of libgaussreg_hip.so (csrc/cloud_icp.hip).  It came after
 * include/gaussreg_hip_cloud.h was closed at its five names.  Same library, same conventions (gaussreg_hip.h, top): device
 * pointers unless a name starts with h_, status codes GR_OK / GR_ERR_*, gr_last_error() for the text, work enqueued on
 * `stream`, no hidden allocation.  The binding reads this header with the parser that reads gaussreg_hip.h
 * (gaussreg_amd/_lib.py: ICP_SIGNATURES / ICP_DEFINES).
 *
 * src (n_src, 3) and ref (n_ref, 3) are fp32, contiguous and finite.  A transform T is a 3x4 fp32 matrix [A | t].
 *
 * Evaluation E(T): source point i is transformed in fp32, no FMA,
 *   p_i.r = ((A[r][0] x + A[r][1] y) + A[r][2] z) + t[r],
 * and j(i), d(i) are exactly row i of gr_cloud_knn(query = p, support = ref, k = 1, max_dist2) -- d = ((dx dx + dy dy) +
 * dz dz) in fp32, candidates ordered by (d, j), -1 / +inf when nothing qualifies.  n = #{i : j(i) >= 0}, S = sum of
 * double(d(i)) over the matched i, fitness = n / n_src, rmse = sqrt(S / n) (0 when n = 0).
 * Update U(T): over the pairs (src_i, ref_j(i)) -- the ORIGINAL source coordinates, no increments are composed -- fp64 sums
 * of fp32 values n, sum src, sum ref, sum src_a ref_b, sum |src|^2, then the fp64 Umeyama fit (rigid, or with_scale: rigid
 * plus uniform scale), rounded once to a 3x4 fp32 T'.
 * Loop, t = 0, 1, ...:  (1) E(T_t) is computed and recorded as history[t];  (2) t >= 1, |fitness_t - fitness_(t-1)| <
 * relative_fitness and |rmse_t - rmse_(t-1)| < relative_rmse: stop, GR_CLOUD_ICP_CONVERGED;  (3) t == max_iterations: stop,
 * GR_CLOUD_ICP_ITERATION_LIMIT;  (4) n_t < 3 or the fit refuses (no spread, a non-positive scale): stop,
 * GR_CLOUD_ICP_DEGENERATE;  (5) T_(t+1) = U(T_t).
 * The result is T_t at the stop with THAT evaluation; iterations = t.  max_iterations = 0 is a pure evaluation of T_0.  On
 * GR_CLOUD_ICP_DEGENERATE the transform is the last valid one (at t = 0: T_0, bit for bit).
 * The sums are taken in a fixed order (per-workgroup partials folded in block order, a fixed tree inside a workgroup, no
 * float atomics): two calls leave the same bits in every output.
 * These are the semantics of Open3D's registration_icp with TransformationEstimationPointToPoint(with_scaling) and
 * ICPConvergenceCriteria; PARITY UNPINNED (Open3D is not available to the tests).
 */
#ifndef GAUSSREG_HIP_ICP_H_
#define GAUSSREG_HIP_ICP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GR_CLOUD_ICP_MAX_ITERATIONS 256
#define GR_CLOUD_ICP_CONVERGED 1
#define GR_CLOUD_ICP_ITERATION_LIMIT 2
#define GR_CLOUD_ICP_DEGENERATE 3

/* host only; 0 for a shape the call refuses */
size_t gr_cloud_icp_workspace_bytes(int64_t n_src, int64_t n_ref, int max_iterations);

/* h_transform0: 12 fp32 on the host (3x4, row-major, finite).  max_dist2 finite and >= 0.  transform_out: 16 fp32 (4x4,
 * last row 0 0 0 1).  stats_out: 4 fp64 {fitness, rmse, n, S}.  index (n_src) int64 and dist2 (n_src) fp32: the
 * correspondences of the reported evaluation, -1 / +inf for an unmatched point.  history: (max_iterations + 1, 16) fp64,
 * row t = T_t[12], n, S, fitness, rmse; rows never reached are left untouched.  index, dist2 and history may be null.
 * h_status: int[2] {status, iterations} on the host, from the call's one read-back (the stream is synchronised once).
 * 1 <= n_ref < 2^31, 0 <= n_src < 2^31, 0 <= max_iterations <= GR_CLOUD_ICP_MAX_ITERATIONS.  A non-finite point:
 * GR_ERR_INVALID ("points must be finite"), no output is written.  n_src == 0: GR_OK, GR_CLOUD_ICP_DEGENERATE, n = 0, the
 * transform is T_0 (ref is not read).  gr_timing_* names: "cloud_icp_grid", "cloud_icp_iterate". */
int gr_cloud_icp(const float* src, int64_t n_src, const float* ref, int64_t n_ref, const float* h_transform0, float max_dist2,
                 int with_scale, int max_iterations, double relative_fitness, double relative_rmse, float* transform_out,
                 double* stats_out, int64_t* index, float* dist2, double* history, int* h_status, void* ws, size_t ws_bytes,
                 void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GAUSSREG_HIP_ICP_H_ */
