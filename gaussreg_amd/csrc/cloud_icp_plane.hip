// Point-to-plane ICP (include/gaussreg_hip_icp_plane.h): the loop of cloud_icp_shared.hpp -- the grid over
// ref, the order of the source, the match, its fallback, the fold with the stop rule, the scatter and the host driver -- with
// the estimator below; this file adds
//
//   icpp_normals_kernel   one thread per reference normal: raises bit 1 of the finiteness flag for a non-finite component
//   PointToPlane::add     a matched pair in icp_sums_kernel: p = T_t src by the `apply` of the match (the same bits),
//                         q = ref[j], v = ref_normals[j]; in fp64 r = (p - q) . v, a = [p x v, v]; n, S = sum d, the 21
//                         distinct entries of sum a a^T and the 6 of sum a r -> 29 sums
//   PointToPlane::update  thread 0 of icp_fold_kernel, after the stop rule has refused n < 6: solve6_compose of
//                         cloud_icp_solve6.hpp, which generalised ICP shares -- the 6x6 Jacobi eigen-solve, the refusal
//                         l_min <= 1e-12 l_max, dR = Rz Ry Rx composed with double(T_t); the fold stores T_(t+1) rounded once
#include "../../include/gaussreg_hip_icp_plane.h"
#include "cloud_icp_shared.hpp"
#include "cloud_icp_solve6.hpp"

namespace gr {
namespace {

constexpr int FLAG_NORMALS = 2;

__global__ __launch_bounds__(THREADS) void icpp_normals_kernel(const float* __restrict__ normals, int64_t count,
                                                               int32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (i >= count) return;
  if (!isfinite(normals[i])) atomicOr(flag, FLAG_NORMALS);
}

struct PointToPlane {
  static constexpr int NSUM = 29, I_N = 0, I_S = 1;  // n, S, H (21: the upper triangle row by row), g (6)
  static constexpr double MIN_PAIRS = 6.0;
  struct Args {
    const float* ref_normals;
  };
  static constexpr const char* ARG_NAMES = "ref_normals, ";
  static bool args_ok(const Args& a) { return a.ref_normals != nullptr; }
  static void after_grid(const Args& a, int64_t ns, int32_t* misc, hipStream_t stream) {
    hipLaunchKernelGGL(icpp_normals_kernel, dim3((unsigned)((3 * ns + THREADS - 1) / THREADS)), dim3(THREADS), 0, stream,
                       a.ref_normals, 3 * ns, misc);
  }
  static const char* flag_text(int32_t flag) {
    return (flag & FLAG_NORMALS) ? "normals must be finite" : "points must be finite";
  }

  __device__ static __forceinline__ void add(double (&v)[NSUM], float4 src, int32_t j, float d, const float* __restrict__ ref,
                                             const float* __restrict__ T, const Args& args) {
    const float* __restrict__ ref_normals = args.ref_normals;
    float fx, fy, fz;
    apply(T, src.x, src.y, src.z, fx, fy, fz);
    const double px = (double)fx, py = (double)fy, pz = (double)fz;
    const double qx = (double)ref[3 * (int64_t)j], qy = (double)ref[3 * (int64_t)j + 1], qz = (double)ref[3 * (int64_t)j + 2];
    const double nx = (double)ref_normals[3 * (int64_t)j], ny = (double)ref_normals[3 * (int64_t)j + 1],
                 nz = (double)ref_normals[3 * (int64_t)j + 2];
    const double r = ((px - qx) * nx + (py - qy) * ny) + (pz - qz) * nz;
    const double a[6] = {py * nz - pz * ny, pz * nx - px * nz, px * ny - py * nx, nx, ny, nz};
    v[0] += 1.0;
    v[1] += (double)d;
    int e = P_H;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
#pragma unroll
      for (int dd = c; dd < 6; ++dd) v[e++] += a[c] * a[dd];
      v[P_G + c] += a[c] * r;
    }
  }

  __device__ static __forceinline__ bool update(const double* sum, const float* T, const Args&, float* Tn) {
    return solve6_compose(sum, T, Tn);
  }
};

}  // namespace
}  // namespace gr

using namespace gr;

extern "C" size_t gr_cloud_icp_plane_workspace_bytes(int64_t n_src, int64_t n_ref, int max_iterations) {
  return icp_workspace_bytes<PointToPlane>(n_src, n_ref, max_iterations);
}

extern "C" int gr_cloud_icp_plane(const float* src, int64_t nq, const float* ref, const float* ref_normals, int64_t ns,
                                  const float* h_transform0, float max_dist2, int max_iterations, double relative_fitness,
                                  double relative_rmse, float* transform_out, double* stats_out, int64_t* index, float* dist2,
                                  double* history, int* h_status, void* ws, size_t ws_bytes, void* stream) {
  return icp_run<PointToPlane>("cloud icp plane", "cloud_icp_plane_grid", "cloud_icp_plane_iterate", src, nq, ref, ns,
                               h_transform0, max_dist2, {ref_normals}, max_iterations, relative_fitness, relative_rmse,
                               transform_out, stats_out, index, dist2, history, h_status, ws, ws_bytes,
                               static_cast<hipStream_t>(stream));
}
