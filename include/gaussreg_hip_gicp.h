/* gaussreg_hip_gicp.h -- generalised ICP and the covariances it takes, of libgaussreg_hip.so (csrc/cloud_icp_gicp.hip,
 * csrc/cloud_covariances.hip).  It came after include/gaussreg_hip_icp_plane.h was closed at its four names.
 * Same library, same conventions (gaussreg_hip.h, top): device pointers unless a name starts with h_, status codes GR_OK /
 * GR_ERR_*, gr_last_error() for the text, work enqueued on `stream`, no hidden allocation.  The binding reads this header
 * with the parser that reads gaussreg_hip.h (gaussreg_amd/_lib.py: GICP_SIGNATURES / GICP_DEFINES).
 *
 * A covariance is six fp32 values, the upper triangle xx, xy, xz, yy, yz, zz: the order of the rasterizer's cov3D_precomp.
 *
 * GENERALISED ICP.  Evaluation E(T), the stop rule, the status codes GR_CLOUD_ICP_*, the history row, max_iterations = 0 as a
 * pure evaluation, the one read-back per call and bitwise reproducibility are those of include/gaussreg_hip_icp.h; fitness
 * and inlier RMSE are Euclidean.  Only the update differs.  U(T_t): for every matched i let p = the fp32-transformed source
 * point of E (the same bits), q = ref[j(i)], Cs = src_cov[i], Ct = ref_cov[j(i)] and A = the 3x3 block of the recorded fp32
 * T_t -- used as given, rigid or not.  In fp64 on those fp32 values: B = A Cs, M = Ct + B A^T (the upper triangle, every dot
 * product as ((a + b) + c)), W = M^-1 = adj(M) / det(M), d = p - q, J = [-[p]x, I] (3x6),
 *     H = sum J^T W J (21 distinct entries), g = sum J^T W d,
 * in the fixed order of the point-to-point sums.  A pair with !(det M > 1e-12 s^3), s = trace(M) / 3 -- two zero
 * covariances, a NaN -- adds nothing to H and g; it still counts in n and S.  n < 3: GR_CLOUD_ICP_DEGENERATE.
 * H = V diag(l) V^T by Jacobi in fp64; l_min <= 1e-12 l_max: degenerate.  Otherwise x = -V diag(1 / l) V^T g =
 * (alpha, beta, gamma, tx, ty, tz), dR = Rz(gamma) Ry(beta) Rx(alpha), dt = (tx, ty, tz) and T_(t+1) = fl32(dT . double(T_t)):
 * composed in fp64, rounded once, so T_(t+1) is a function of the recorded fp32 T_t alone.  A non-finite result is degenerate.
 * This is the system of Open3D's TransformationEstimationForGeneralizedICP, which writes the rows W^(1/2) J and the residual
 * W^(1/2) d: (W^(1/2))^T W^(1/2) = W, so no square root is taken here.  PARITY UNPINNED (Open3D is not available to the tests).
 *
 * COVARIANCES FROM NORMALS.  Per row, in fp64: v = n / |n|, C = I - (1 - epsilon) v v^T (eigenvalues epsilon, 1, 1: the plane
 * prior of generalised ICP), every entry rounded once.  |n| = 0: C = I exactly.  A non-finite component makes its own row
 * non-finite.
 *
 * COVARIANCES OF GAUSSIANS.  scales (n, 3), rotations (n, 4) as (r, x, y, z), fp32.  GR_GS_COV_RAW: the six floats the
 * rasterizer computes for itself from scale_modifier * scales and the rotation as given, in its fp32 arithmetic, bit for
 * bit; epsilon is not used.  GR_GS_COV_PLANE: a = the axis of the smallest scale (the first among equals), q^ = q / |q| in
 * fp64, v = column a of R(q^) divided by its norm, C = I - (1 - epsilon) v v^T, rounded once.  In both modes normals_out =
 * v with the sign of gr_cloud_normals without h_toward (the component of largest magnitude, the first among equals, is
 * positive) and valid_out = 1; |q| = 0: a zero normal and valid_out = 0, and in PLANE mode C = I.
 */
#ifndef GAUSSREG_HIP_GICP_H_
#define GAUSSREG_HIP_GICP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GR_GS_COV_RAW 0
#define GR_GS_COV_PLANE 1

/* host only; 0 for a shape the call refuses */
size_t gr_cloud_gicp_workspace_bytes(int64_t n_src, int64_t n_ref, int max_iterations);

/* The arguments of gr_cloud_icp_plane with src_cov (n_src, 6) fp32 after n_src and ref_cov (n_ref, 6) fp32 in place of
 * ref_normals.  A non-finite point or covariance entry: GR_ERR_INVALID ("points must be finite" / "covariances must be
 * finite"), no output is written.  n_src == 0: GR_OK, GR_CLOUD_ICP_DEGENERATE, the transform is T_0 (src_cov, ref and
 * ref_cov are not read; src_cov and ref_cov may then be null).  src_cov is read through the original source index every
 * round; the workspace is that of gr_cloud_icp_plane.  gr_timing_* names: "cloud_gicp_grid", "cloud_gicp_iterate". */
int gr_cloud_gicp(const float* src, int64_t n_src, const float* src_cov, const float* ref, const float* ref_cov, int64_t n_ref,
                  const float* h_transform0, float max_dist2, int max_iterations, double relative_fitness,
                  double relative_rmse, float* transform_out, double* stats_out, int64_t* index, float* dist2,
                  double* history, int* h_status, void* ws, size_t ws_bytes, void* stream);

/* normals (n, 3) fp32, cov_out (n, 6) fp32, 0 <= n < 2^31, epsilon finite and in [0, 1].  n == 0: GR_OK, nothing is read or
 * written.  Nothing is carved from the workspace, which may be null.  gr_timing_* name: "cloud_covariances". */
int gr_cloud_covariances_from_normals(const float* normals, int64_t n, double epsilon, float* cov_out, void* ws, size_t ws_bytes,
                                      void* stream);

/* scales (n, 3), rotations (n, 4) fp32; mode GR_GS_COV_RAW or GR_GS_COV_PLANE; scale_modifier finite; epsilon as above.
 * cov_out (n, 6) fp32; normals_out (n, 3) fp32 and valid_out (n) uint8 may be null.  gr_timing_* name: "gs_covariances". */
int gr_gs_covariances(const float* scales, const float* rotations, int64_t n, float scale_modifier, int mode, double epsilon,
                      float* cov_out, float* normals_out, uint8_t* valid_out, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GAUSSREG_HIP_GICP_H_ */
