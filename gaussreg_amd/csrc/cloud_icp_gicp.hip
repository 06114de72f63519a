// Generalised ICP (include/gaussreg_hip_gicp.h): the loop of cloud_icp_shared.hpp -- the grid over ref, the
// order of the source, the match, its fallback, the fold with the stop rule, the scatter and the host driver -- with the
// estimator below; this file adds
//
//   gicp_cov_kernel      one thread per covariance entry of either cloud: raises bit 2 of the finiteness flag for a
//                        non-finite one
//   Generalized::add     a matched pair in icp_sums_kernel: p = T_t src by the `apply` of the match (the same bits),
//                        q = ref[j], Cs = src_cov[i] through the original index in q_sorted[s].w, Ct = ref_cov[j], A = the
//                        3x3 block of T_t; in fp64 M = Ct + (A Cs) A^T (upper triangle), W = adj(M) / det(M), d = p - q;
//                        n, S = sum d^2, the 21 distinct entries of sum J^T W J and the 6 of sum J^T W d with
//                        J = [-[p]x, I] -> 29 sums in the layout of point-to-plane.  !(det M > 1e-12 (trace M / 3)^3):
//                        only n and S
//   Generalized::update  solve6_compose of cloud_icp_solve6.hpp, the code point-to-plane runs
#include "../../include/gaussreg_hip_gicp.h"
#include "cloud_icp_shared.hpp"
#include "cloud_icp_solve6.hpp"

namespace gr {
namespace {

constexpr int FLAG_COV = 4;

__global__ __launch_bounds__(THREADS) void gicp_cov_kernel(const float* __restrict__ cov, int64_t count,
                                                           int32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (i >= count) return;
  if (!isfinite(cov[i])) atomicOr(flag, FLAG_COV);
}

struct Generalized {
  static constexpr int NSUM = 29, I_N = 0, I_S = 1;  // n, S, H (21: the upper triangle row by row), g (6)
  static constexpr double MIN_PAIRS = 3.0;
  struct Args {
    const float* src_cov;
    const float* ref_cov;
    int64_t n_src;
  };
  static constexpr const char* ARG_NAMES = "src_cov, ref_cov, ";
  static bool args_ok(const Args& a) { return a.n_src == 0 || (a.src_cov != nullptr && a.ref_cov != nullptr); }  // n_src == 0: not read
  static void after_grid(const Args& a, int64_t ns, int32_t* misc, hipStream_t stream) {
    hipLaunchKernelGGL(gicp_cov_kernel, dim3((unsigned)((6 * a.n_src + THREADS - 1) / THREADS)), dim3(THREADS), 0, stream,
                       a.src_cov, 6 * a.n_src, misc);
    hipLaunchKernelGGL(gicp_cov_kernel, dim3((unsigned)((6 * ns + THREADS - 1) / THREADS)), dim3(THREADS), 0, stream, a.ref_cov,
                       6 * ns, misc);
  }
  static const char* flag_text(int32_t flag) {
    return (flag & FLAG_COV) ? "covariances must be finite" : "points must be finite";
  }

  __device__ static __forceinline__ void add(double (&v)[NSUM], float4 src, int32_t j, float d, const float* __restrict__ ref,
                                             const float* __restrict__ T, const Args& args) {
    const float* __restrict__ cs = args.src_cov + 6 * (int64_t)__float_as_int(src.w);
    const float* __restrict__ ct = args.ref_cov + 6 * (int64_t)j;
    float fx, fy, fz;
    apply(T, src.x, src.y, src.z, fx, fy, fz);
    v[0] += 1.0;
    v[1] += (double)d;
    // M = Ct + (A Cs) A^T, its upper triangle m = xx, xy, xz, yy, yz, zz
    const double sxx = (double)cs[0], sxy = (double)cs[1], sxz = (double)cs[2], syy = (double)cs[3], syz = (double)cs[4],
                 szz = (double)cs[5];
    double B[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const double a0 = (double)T[4 * r], a1 = (double)T[4 * r + 1], a2 = (double)T[4 * r + 2];
      B[r][0] = (a0 * sxx + a1 * sxy) + a2 * sxz;
      B[r][1] = (a0 * sxy + a1 * syy) + a2 * syz;
      B[r][2] = (a0 * sxz + a1 * syz) + a2 * szz;
    }
    double m[6];
    {
      int e = 0;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = r; c < 3; ++c, ++e)
          m[e] = (double)ct[e] + ((B[r][0] * (double)T[4 * c] + B[r][1] * (double)T[4 * c + 1]) + B[r][2] * (double)T[4 * c + 2]);
      }
    }
    // W = adj(M) / det(M)
    const double c00 = m[3] * m[5] - m[4] * m[4], c01 = m[2] * m[4] - m[1] * m[5], c02 = m[1] * m[4] - m[2] * m[3];
    const double det = (m[0] * c00 + m[1] * c01) + m[2] * c02;
    const double s = ((m[0] + m[3]) + m[5]) / 3.0;
    if (!(det > 1e-12 * ((s * s) * s))) return;  // a NaN as well: the pair counts, it does not steer
    const double inv = 1.0 / det;
    const double w[3][3] = {{c00 * inv, c01 * inv, c02 * inv},
                            {c01 * inv, (m[0] * m[5] - m[2] * m[2]) * inv, (m[1] * m[2] - m[0] * m[4]) * inv},
                            {c02 * inv, (m[1] * m[2] - m[0] * m[4]) * inv, (m[0] * m[3] - m[1] * m[1]) * inv}};
    const double px = (double)fx, py = (double)fy, pz = (double)fz;
    const double dx = px - (double)ref[3 * (int64_t)j], dy = py - (double)ref[3 * (int64_t)j + 1],
                 dz = pz - (double)ref[3 * (int64_t)j + 2];
    // J^T = [[p]x; I]: row r of K = [p]x W is (p x W[:, c])_r over c; the rotation block is K [p]x^T, its entry (r, c) is
    // (p x K[r, :])_c
    double K[3][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      K[0][c] = py * w[2][c] - pz * w[1][c];
      K[1][c] = pz * w[0][c] - px * w[2][c];
      K[2][c] = px * w[1][c] - py * w[0][c];
    }
    const double wd[3] = {(w[0][0] * dx + w[0][1] * dy) + w[0][2] * dz, (w[1][0] * dx + w[1][1] * dy) + w[1][2] * dz,
                          (w[2][0] * dx + w[2][1] * dy) + w[2][2] * dz};
    // the 6x6 rows in order: rows 0..2 are [K [p]x^T | K], rows 3..5 are [. | W]
    int e = P_H;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const double h[3] = {py * K[r][2] - pz * K[r][1], pz * K[r][0] - px * K[r][2], px * K[r][1] - py * K[r][0]};
#pragma unroll
      for (int c = r; c < 3; ++c) v[e++] += h[c];
#pragma unroll
      for (int c = 0; c < 3; ++c) v[e++] += K[r][c];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = r; c < 3; ++c) v[e++] += w[r][c];
    }
    v[P_G] += py * wd[2] - pz * wd[1];
    v[P_G + 1] += pz * wd[0] - px * wd[2];
    v[P_G + 2] += px * wd[1] - py * wd[0];
    v[P_G + 3] += wd[0];
    v[P_G + 4] += wd[1];
    v[P_G + 5] += wd[2];
  }

  __device__ static __forceinline__ bool update(const double* sum, const float* T, const Args&, float* Tn) {
    return solve6_compose(sum, T, Tn);
  }
};

}  // namespace
}  // namespace gr

using namespace gr;

extern "C" size_t gr_cloud_gicp_workspace_bytes(int64_t n_src, int64_t n_ref, int max_iterations) {
  return icp_workspace_bytes<Generalized>(n_src, n_ref, max_iterations);
}

extern "C" int gr_cloud_gicp(const float* src, int64_t nq, const float* src_cov, const float* ref, const float* ref_cov,
                             int64_t ns, const float* h_transform0, float max_dist2, int max_iterations, double relative_fitness,
                             double relative_rmse, float* transform_out, double* stats_out, int64_t* index, float* dist2,
                             double* history, int* h_status, void* ws, size_t ws_bytes, void* stream) {
  return icp_run<Generalized>("cloud gicp", "cloud_gicp_grid", "cloud_gicp_iterate", src, nq, ref, ns, h_transform0, max_dist2,
                              {src_cov, ref_cov, nq}, max_iterations, relative_fitness, relative_rmse, transform_out, stats_out,
                              index, dist2, history, h_status, ws, ws_bytes, static_cast<hipStream_t>(stream));
}
