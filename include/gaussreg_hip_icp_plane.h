/* gaussreg_hip_icp_plane.h -- PCA normals from a neighbour table and point-to-plane ICP of libgaussreg_hip.so
 * (csrc/cloud_normals.hip, csrc/cloud_icp_plane.hip).  It came after include/gaussreg_hip_icp.h was
 * closed at its two names.  Same library, same conventions (gaussreg_hip.h, top): device pointers unless a name starts with
 * h_, status codes GR_OK / GR_ERR_*, gr_last_error() for the text, work enqueued on `stream`, no hidden allocation.  The
 * binding reads this header with the parser that reads gaussreg_hip.h (gaussreg_amd/_lib.py: ICP_PLANE_SIGNATURES /
 * ICP_PLANE_DEFINES).
 *
 * NORMALS.  Per query i: the set is support[neighbors[i][k]] for every k whose entry lies in [0, M), in list order -- any
 * other entry (-1, M, ...) is padding and is skipped -- preceded by query[i] itself when include_self.  m = its size.
 * Every point has the FIRST point of the set subtracted in fp64 (exact: the difference of two fp32 values); sum d and
 * sum d d^T are accumulated in fp64 in list order; C = sum d d^T - (sum d)(sum d)^T / m.  The eigenproblem of the symmetric
 * 3x3 C is solved by cyclic Jacobi in fp64, eigenvalues l0 <= l1 <= l2.  normal = the unit eigenvector of l0, rounded once to
 * fp32; curvature = l0 / (l0 + l1 + l2) (0 when the sum is 0); valid = 1.  m < 3 or l1 <= 1e-12 l2 (collinear, coincident):
 * valid = 0, normal (0, 0, 0), curvature 0.  Sign: with h_toward, flipped so that n . (toward - query[i]) >= 0, the dot
 * product in fp64; without, flipped so that the component of largest magnitude (the first among equals) is positive.
 *
 * POINT-TO-PLANE ICP.  Evaluation E(T), the stop rule, the status codes GR_CLOUD_ICP_*, the history row, max_iterations = 0
 * as a pure evaluation, the one read-back per call and bitwise reproducibility are those of include/gaussreg_hip_icp.h.  Only
 * the update differs.  U(T_t): for every matched i let p = the fp32-transformed source point of E (the same bits),
 * q = ref[j(i)], v = ref_normals[j(i)] -- used as given, not renormalised.  In fp64 on those fp32 values: r = (p - q) . v,
 * a = [p x v, v] in R^6, H = sum a a^T (21 distinct entries), g = sum a r, in the fixed order of the point-to-point sums.
 * n < 6: GR_CLOUD_ICP_DEGENERATE.  H = V diag(l) V^T by Jacobi in fp64; l_min <= 1e-12 l_max: degenerate.  Otherwise
 * x = -V diag(1 / l) V^T g = (alpha, beta, gamma, tx, ty, tz), dR = Rz(gamma) Ry(beta) Rx(alpha) (an exact rotation, Open3D's
 * TransformVector6dToMatrix4d), dt = (tx, ty, tz), and T_(t+1) = fl32(dT . double(T_t)): composed in fp64, rounded once, so
 * T_(t+1) is a function of the recorded fp32 T_t alone.  A non-finite result is degenerate.  A zero normal contributes a
 * zero row to a; its point still counts in n and S.
 * These are the semantics of Open3D's registration_icp with TransformationEstimationPointToPlane and no robust kernel;
 * PARITY UNPINNED (Open3D is not available to the tests).
 */
#ifndef GAUSSREG_HIP_ICP_PLANE_H_
#define GAUSSREG_HIP_ICP_PLANE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GR_CLOUD_NORMALS_MAX_K 64

/* host only; 0 for a shape the call refuses, 256 otherwise: the call carves nothing */
size_t gr_cloud_normals_workspace_bytes(int64_t n_query, int64_t n_support, int k);

/* query (n_query, 3) and support (n_support, 3) fp32, contiguous, finite; support may be query.  neighbors (n_query, k)
 * int64, 1 <= k <= GR_CLOUD_NORMALS_MAX_K.  include_self 0 or 1.  h_toward: 3 fp32 on the host, finite, or null.
 * normals (n_query, 3) fp32; curvature (n_query) fp32 and valid (n_query) uint8 may be null.  0 <= n_query < 2^31,
 * 0 <= n_support < 2^31.  Points that enter a set are not checked for finiteness: a non-finite one gives valid = 0 or a
 * non-finite normal in its own row only.  n_query == 0: GR_OK, nothing is read or written. */
int gr_cloud_normals(const float* query, int64_t n_query, const float* support, int64_t n_support, const int64_t* neighbors,
                     int k, int include_self, const float* h_toward, float* normals, float* curvature, uint8_t* valid, void* ws,
                     size_t ws_bytes, void* stream);

/* host only; 0 for a shape the call refuses */
size_t gr_cloud_icp_plane_workspace_bytes(int64_t n_src, int64_t n_ref, int max_iterations);

/* The arguments of gr_cloud_icp with ref_normals (n_ref, 3) fp32 after ref and without with_scale.  A non-finite point or
 * normal: GR_ERR_INVALID ("points must be finite" / "normals must be finite"), no output is written.  n_src == 0: GR_OK,
 * GR_CLOUD_ICP_DEGENERATE, the transform is T_0 (ref and ref_normals are not read).  gr_timing_* names:
 * "cloud_icp_plane_grid", "cloud_icp_plane_iterate". */
int gr_cloud_icp_plane(const float* src, int64_t n_src, const float* ref, const float* ref_normals, int64_t n_ref,
                       const float* h_transform0, float max_dist2, int max_iterations, double relative_fitness,
                       double relative_rmse, float* transform_out, double* stats_out, int64_t* index, float* dist2,
                       double* history, int* h_status, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GAUSSREG_HIP_ICP_PLANE_H_ */
