// Point-to-plane ICP (include/gaussreg_hip_icp_plane.h): the loop of cloud_icp_shared.hpp -- the grid over
// ref, the order of the source, the match, its fallback, the fold with the stop rule, the scatter and the host driver -- with
// the estimator below; this file adds
//
//   icpp_normals_kernel   one thread per reference normal: raises bit 1 of the finiteness flag for a non-finite component
//   PointToPlane::add     a matched pair in icp_sums_kernel: p = T_t src by the `apply` of the match (the same bits),
//                         q = ref[j], v = ref_normals[j]; in fp64 r = (p - q) . v, a = [p x v, v]; n, S = sum d, the 21
//                         distinct entries of sum a a^T and the 6 of sum a r -> 29 sums
//   PointToPlane::update  thread 0 of icp_fold_kernel, after the stop rule has refused n < 6: solves the 6x6 system by a
//                         cyclic Jacobi eigen-decomposition whose matrices live in LDS (run-time row and column indices,
//                         so not in registers), refuses l_min <= 1e-12 l_max, forms dR = Rz Ry Rx and composes with
//                         double(T_t); the fold stores T_(t+1) rounded once
#include "../../include/gaussreg_hip_icp_plane.h"
#include "cloud_icp_shared.hpp"

namespace gr {
namespace {

constexpr int P_H = 2, P_G = 23;
constexpr int PLANE_SWEEPS = 32;
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

  __device__ static bool update(const double* sum, const float* T, const Args&, float* Tn) {
    __shared__ double Hm[36], Vm[36], ys[6], xs[6];  // thread 0's 6x6 solve: indexed at run time, so in LDS
    // H and V = I
    int e = P_H;
    double fro2 = 0.0;
    for (int c = 0; c < 6; ++c)
      for (int d = c; d < 6; ++d) {
        const double h = sum[e++];
        Hm[c * 6 + d] = Hm[d * 6 + c] = h;
        fro2 += (c == d ? 1.0 : 2.0) * h * h;
      }
    for (int k = 0; k < 36; ++k) Vm[k] = (k % 7 == 0) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < PLANE_SWEEPS; ++sweep) {
      double off = 0.0;
      for (int p = 0; p < 5; ++p)
        for (int r = p + 1; r < 6; ++r) off += Hm[p * 6 + r] * Hm[p * 6 + r];
      if (off <= 1e-30 * fro2) break;
#pragma unroll 1
      for (int p = 0; p < 5; ++p) {
#pragma unroll 1
        for (int r = p + 1; r < 6; ++r) {
          const double hpr = Hm[p * 6 + r];
          if (fabs(hpr) < 1e-300) continue;
          const double theta = (Hm[r * 6 + r] - Hm[p * 6 + p]) / (2.0 * hpr);
          const double tt = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
          const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
          for (int k = 0; k < 6; ++k) {
            const double a = Hm[k * 6 + p], b = Hm[k * 6 + r];
            Hm[k * 6 + p] = c * a - s * b;
            Hm[k * 6 + r] = s * a + c * b;
          }
          for (int k = 0; k < 6; ++k) {
            const double a = Hm[p * 6 + k], b = Hm[r * 6 + k];
            Hm[p * 6 + k] = c * a - s * b;
            Hm[r * 6 + k] = s * a + c * b;
          }
          for (int k = 0; k < 6; ++k) {
            const double a = Vm[k * 6 + p], b = Vm[k * 6 + r];
            Vm[k * 6 + p] = c * a - s * b;
            Vm[k * 6 + r] = s * a + c * b;
          }
        }
      }
    }
    double lmin = Hm[0], lmax = Hm[0];
    for (int k = 1; k < 6; ++k) {
      lmin = fmin(lmin, Hm[k * 7]);
      lmax = fmax(lmax, Hm[k * 7]);
    }
    if (!(lmin > 1e-12 * lmax)) return false;  // a NaN as well
    for (int k = 0; k < 6; ++k) {  // y = diag(1 / l) V^T g
      double a = 0.0;
      for (int j = 0; j < 6; ++j) a += Vm[j * 6 + k] * sum[P_G + j];
      ys[k] = a / Hm[k * 7];
    }
    for (int i = 0; i < 6; ++i) {  // x = -V y
      double a = 0.0;
      for (int k = 0; k < 6; ++k) a += Vm[i * 6 + k] * ys[k];
      xs[i] = -a;
    }
    const double ca = cos(xs[0]), sa = sin(xs[0]), cb = cos(xs[1]), sb = sin(xs[1]), cg = cos(xs[2]), sg = sin(xs[2]);
    // dR = Rz(gamma) Ry(beta) Rx(alpha)
    const double dR[9] = {cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa,
                          sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa,
                          -sb,     cb * sa,                cb * ca};
    const double dt[3] = {xs[3], xs[4], xs[5]};
    double A[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) A[k] = (double)T[k];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        double a = (dR[r * 3] * A[c] + dR[r * 3 + 1] * A[4 + c]) + dR[r * 3 + 2] * A[8 + c];
        if (c == 3) a += dt[r];
        Tn[r * 4 + c] = (float)a;
      }
    }
    return true;
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
