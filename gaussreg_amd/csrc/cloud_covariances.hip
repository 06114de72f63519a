// The covariances generalised ICP takes (include/gaussreg_hip_gicp.h).  No search happens here.
//
//   cov_normals_kernel   one thread per normal: v = n / |n| in fp64, C = I - (1 - epsilon) v v^T, each entry rounded once;
//                        |n| = 0 -> I
//   gs_cov_kernel        one thread per Gaussian.  RAW: cov3d_from_scale_rot of raster_shared.hpp, the rasterizer's own fp32
//                        arithmetic.  PLANE: the plane prior about the axis of the smallest scale.  Both: that axis as a
//                        unit normal with the sign rule of normals_kernel, and whether the quaternion has a length
// Both move 36 B (normals) or 52 to 65 B (Gaussians) per row and do a few dozen fp64 operations: bound by memory.
#include <cmath>

#include "../../include/gaussreg_hip_gicp.h"
#include "raster_shared.hpp"

namespace gr {
namespace {

constexpr int COV_THREADS = 256;

// C = I - k v v^T, rounded once per entry
__device__ __forceinline__ void plane_prior(const double* v, double k, float* __restrict__ c6) {
  c6[0] = (float)(1.0 - k * (v[0] * v[0]));
  c6[1] = (float)(0.0 - k * (v[0] * v[1]));
  c6[2] = (float)(0.0 - k * (v[0] * v[2]));
  c6[3] = (float)(1.0 - k * (v[1] * v[1]));
  c6[4] = (float)(0.0 - k * (v[1] * v[2]));
  c6[5] = (float)(1.0 - k * (v[2] * v[2]));
}

__global__ __launch_bounds__(COV_THREADS) void cov_normals_kernel(const float* __restrict__ normals, int64_t n, double epsilon,
                                                                  float* __restrict__ cov) {
  const int64_t i = (int64_t)blockIdx.x * COV_THREADS + threadIdx.x;
  if (i >= n) return;
  double v[3] = {(double)normals[3 * i], (double)normals[3 * i + 1], (double)normals[3 * i + 2]};
  const double nn = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
  double k = 0.0;  // |n| = 0: C = I
  if (nn != 0.0) {
    k = 1.0 - epsilon;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] /= nn;
  }
  plane_prior(v, k, cov + 6 * i);
}

__global__ __launch_bounds__(COV_THREADS) void gs_cov_kernel(const float* __restrict__ scales, const float* __restrict__ rotations,
                                                             int64_t n, float scale_modifier, int mode, double epsilon,
                                                             float* __restrict__ cov, float* __restrict__ normals,
                                                             uint8_t* __restrict__ valid) {
  const int64_t i = (int64_t)blockIdx.x * COV_THREADS + threadIdx.x;
  if (i >= n) return;
  float sc[3], rot[4];
#pragma unroll
  for (int k = 0; k < 3; ++k) sc[k] = scales[3 * i + k];
#pragma unroll
  for (int k = 0; k < 4; ++k) rot[k] = rotations[4 * i + k];
  // the axis of the smallest scale, the first among equals, as column `axis` of R(q / |q|) in the rasterizer's convention
  const int axis = (sc[0] <= sc[1] && sc[0] <= sc[2]) ? 0 : (sc[1] <= sc[2] ? 1 : 2);
  double q[4] = {(double)rot[0], (double)rot[1], (double)rot[2], (double)rot[3]};
  const double qn = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
  double v[3] = {0.0, 0.0, 0.0};
  const bool ok = qn != 0.0;
  if (ok && (mode == GR_GS_COV_PLANE || normals)) {  // RAW without normals_out needs the length of q only
    const double r = q[0] / qn, x = q[1] / qn, y = q[2] / qn, z = q[3] / qn;
    const double c0[3] = {1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y + r * z), 2.0 * (x * z - r * y)};
    const double c1[3] = {2.0 * (x * y - r * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z + r * x)};
    const double c2[3] = {2.0 * (x * z + r * y), 2.0 * (y * z - r * x), 1.0 - 2.0 * (x * x + y * y)};
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = axis == 0 ? c0[k] : axis == 1 ? c1[k] : c2[k];
    const double vn = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] /= vn;
  }
  if (mode == GR_GS_COV_RAW) {
    float c6[6];
    cov3d_from_scale_rot(sc, scale_modifier, rot, c6);
#pragma unroll
    for (int k = 0; k < 6; ++k) cov[6 * i + k] = c6[k];
  } else {
    plane_prior(v, ok ? 1.0 - epsilon : 0.0, cov + 6 * i);
  }
  if (normals) {
    const double a0 = fabs(v[0]), a1 = fabs(v[1]), a2 = fabs(v[2]);
    const double big = (a0 >= a1 && a0 >= a2) ? v[0] : (a1 >= a2 ? v[1] : v[2]);
    const bool flip = big < 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) normals[3 * i + k] = (float)(flip ? -v[k] : v[k]);
  }
  if (valid) valid[i] = ok ? 1 : 0;
}

}  // namespace
}  // namespace gr

using namespace gr;

extern "C" int gr_cloud_covariances_from_normals(const float* normals, int64_t n, double epsilon, float* cov_out, void* ws,
                                                 size_t ws_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  GR_REQUIRE(n >= 0 && n < (1ll << 31), "cloud covariances: n = %lld outside [0, 2^31)", (long long)n);
  GR_REQUIRE(epsilon >= 0.0 && epsilon <= 1.0, "cloud covariances: epsilon = %g outside [0, 1]", epsilon);
  if (n == 0) return GR_OK;
  GR_REQUIRE(normals && cov_out, "cloud covariances: null normals or cov_out");
  (void)ws;
  (void)ws_bytes;
  KernelTimer timer("cloud_covariances", stream);
  hipLaunchKernelGGL(cov_normals_kernel, dim3((unsigned)((n + COV_THREADS - 1) / COV_THREADS)), dim3(COV_THREADS), 0, stream,
                     normals, n, epsilon, cov_out);
  GR_LAUNCH_CHECK();
  return GR_OK;
}

extern "C" int gr_gs_covariances(const float* scales, const float* rotations, int64_t n, float scale_modifier, int mode,
                                 double epsilon, float* cov_out, float* normals_out, uint8_t* valid_out, void* ws,
                                 size_t ws_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  GR_REQUIRE(n >= 0 && n < (1ll << 31), "gs covariances: n = %lld outside [0, 2^31)", (long long)n);
  GR_REQUIRE(mode == GR_GS_COV_RAW || mode == GR_GS_COV_PLANE, "gs covariances: mode = %d, must be GR_GS_COV_RAW or GR_GS_COV_PLANE",
             mode);
  GR_REQUIRE(epsilon >= 0.0 && epsilon <= 1.0, "gs covariances: epsilon = %g outside [0, 1]", epsilon);
  GR_REQUIRE(std::isfinite(scale_modifier), "gs covariances: scale_modifier = %g is not finite", (double)scale_modifier);
  if (n == 0) return GR_OK;
  GR_REQUIRE(scales && rotations && cov_out, "gs covariances: null scales, rotations or cov_out");
  (void)ws;
  (void)ws_bytes;
  KernelTimer timer("gs_covariances", stream);
  hipLaunchKernelGGL(gs_cov_kernel, dim3((unsigned)((n + COV_THREADS - 1) / COV_THREADS)), dim3(COV_THREADS), 0, stream, scales,
                     rotations, n, scale_modifier, mode, epsilon, cov_out, normals_out, valid_out);
  GR_LAUNCH_CHECK();
  return GR_OK;
}
