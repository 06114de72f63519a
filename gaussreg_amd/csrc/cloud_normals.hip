// PCA normals from a neighbour table (include/gaussreg_hip_icp_plane.h).  No search happens here: the table
// comes from scene_init.knn, cloud_nn.knn, radius_search or the caller.
//
//   normals_kernel   one thread per query: gathers the listed support points (an entry outside [0, M) is padding), the
//                    query first when include_self; every point minus the FIRST of the set in fp64 (exact), sum d and
//                    sum d d^T in list order, C = sum d d^T - (sum d)(sum d)^T / m; cyclic Jacobi of the 3x3 in fp64
//                    (jacobi_sym, umeyama.hpp: compile-time indices only); the eigenvector of the smallest eigenvalue
//                    by selects, the sign, one rounding to fp32.
// The gather dominates: per query K indices of 8 B and up to K + 1 scattered points of 12 B.
#include <cmath>

#include "../../include/gaussreg_hip_icp_plane.h"
#include "umeyama.hpp"

namespace gr {
namespace {

constexpr int NORMALS_THREADS = 256;
constexpr int NORMALS_SWEEPS = 12;

struct Toward {
  float p[3];
  int given;
};

__global__ __launch_bounds__(NORMALS_THREADS) void normals_kernel(const float* __restrict__ query, int64_t n,
                                                                  const float* support, int64_t M,
                                                                  const int64_t* __restrict__ neighbors, int K, int include_self,
                                                                  Toward toward, float* __restrict__ normals,
                                                                  float* __restrict__ curvature, uint8_t* __restrict__ valid) {
  const int64_t i = (int64_t)blockIdx.x * NORMALS_THREADS + threadIdx.x;
  if (i >= n) return;
  const float qx = query[3 * i], qy = query[3 * i + 1], qz = query[3 * i + 2];
  double o[3] = {0.0, 0.0, 0.0}, s[3] = {0.0, 0.0, 0.0};
  double xx = 0.0, xy = 0.0, xz = 0.0, yy = 0.0, yz = 0.0, zz = 0.0;
  int m = 0;
  if (include_self) {  // the first point of the set: d = 0, nothing to add
    o[0] = (double)qx, o[1] = (double)qy, o[2] = (double)qz;
    m = 1;
  }
  const int64_t* row = neighbors + i * K;
  for (int k = 0; k < K; ++k) {
    const int64_t j = row[k];
    if ((uint64_t)j >= (uint64_t)M) continue;  // padding
    const double x = (double)support[3 * j], y = (double)support[3 * j + 1], z = (double)support[3 * j + 2];
    if (m == 0) o[0] = x, o[1] = y, o[2] = z;
    const double dx = x - o[0], dy = y - o[1], dz = z - o[2];
    s[0] += dx, s[1] += dy, s[2] += dz;
    xx += dx * dx, xy += dx * dy, xz += dx * dz, yy += dy * dy, yz += dy * dz, zz += dz * dz;
    ++m;
  }
  float out[3] = {0.f, 0.f, 0.f}, curv = 0.f;
  uint8_t ok = 0;
  if (m >= 3) {
    const double mm = (double)m;
    double A[3][3], V[3][3];
    A[0][0] = xx - s[0] * s[0] / mm;
    A[0][1] = A[1][0] = xy - s[0] * s[1] / mm;
    A[0][2] = A[2][0] = xz - s[0] * s[2] / mm;
    A[1][1] = yy - s[1] * s[1] / mm;
    A[1][2] = A[2][1] = yz - s[1] * s[2] / mm;
    A[2][2] = zz - s[2] * s[2] / mm;
    jacobi_sym<3, NORMALS_SWEEPS>(A, V);
    const double e0 = A[0][0], e1 = A[1][1], e2 = A[2][2];
    // the smallest (the first among equals), the largest (the last among equals), and the one left over
    const int lo = (e0 <= e1 && e0 <= e2) ? 0 : (e1 <= e2 ? 1 : 2);
    const int hi = (e2 >= e0 && e2 >= e1) ? 2 : (e1 >= e0 ? 1 : 0);
    const int mid = 3 - lo - hi;  // lo == hi only when all three are equal: then mid is 3 - 2 lo, caught just below
    const double l0 = lo == 0 ? e0 : lo == 1 ? e1 : e2, l2 = hi == 0 ? e0 : hi == 1 ? e1 : e2;
    const double l1 = lo == hi ? l0 : (mid == 0 ? e0 : mid == 1 ? e1 : e2);
    if (l1 > 1e-12 * l2) {
      double v[3], nn = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        v[k] = lo == 0 ? V[k][0] : lo == 1 ? V[k][1] : V[k][2];
        nn += v[k] * v[k];
      }
      nn = sqrt(nn);
#pragma unroll
      for (int k = 0; k < 3; ++k) v[k] /= nn;
      bool flip;
      if (toward.given) {
        const double dot = (v[0] * ((double)toward.p[0] - (double)qx) + v[1] * ((double)toward.p[1] - (double)qy)) +
                           v[2] * ((double)toward.p[2] - (double)qz);
        flip = dot < 0.0;
      } else {
        const double a0 = fabs(v[0]), a1 = fabs(v[1]), a2 = fabs(v[2]);
        const double big = (a0 >= a1 && a0 >= a2) ? v[0] : (a1 >= a2 ? v[1] : v[2]);
        flip = big < 0.0;
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) out[k] = (float)(flip ? -v[k] : v[k]);
      const double sum = (l0 + l1) + l2;
      curv = sum != 0.0 ? (float)(l0 / sum) : 0.f;
      ok = 1;
    }
  }
  normals[3 * i] = out[0];
  normals[3 * i + 1] = out[1];
  normals[3 * i + 2] = out[2];
  if (curvature) curvature[i] = curv;
  if (valid) valid[i] = ok;
}

bool normals_shape_ok(int64_t n, int64_t M, int k) {
  return n >= 0 && n < (1ll << 31) && M >= 0 && M < (1ll << 31) && k >= 1 && k <= GR_CLOUD_NORMALS_MAX_K;
}

}  // namespace
}  // namespace gr

using namespace gr;

extern "C" size_t gr_cloud_normals_workspace_bytes(int64_t n_query, int64_t n_support, int k) {
  return normals_shape_ok(n_query, n_support, k) ? 256 : 0;  // nothing is carved; 0 is the refusal
}

extern "C" int gr_cloud_normals(const float* query, int64_t n, const float* support, int64_t M, const int64_t* neighbors, int k,
                                int include_self, const float* h_toward, float* normals, float* curvature, uint8_t* valid,
                                void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  GR_REQUIRE(n >= 0 && n < (1ll << 31), "cloud normals: n_query = %lld outside [0, 2^31)", (long long)n);
  GR_REQUIRE(M >= 0 && M < (1ll << 31), "cloud normals: n_support = %lld outside [0, 2^31)", (long long)M);
  GR_REQUIRE(k >= 1 && k <= GR_CLOUD_NORMALS_MAX_K, "cloud normals: k = %d outside [1, %d]", k, GR_CLOUD_NORMALS_MAX_K);
  GR_REQUIRE(include_self == 0 || include_self == 1, "cloud normals: include_self = %d, must be 0 or 1", include_self);
  Toward toward = {{0.f, 0.f, 0.f}, 0};
  if (h_toward) {
    for (int c = 0; c < 3; ++c) {
      GR_REQUIRE(std::isfinite(h_toward[c]), "cloud normals: h_toward[%d] is not finite", c);
      toward.p[c] = h_toward[c];
    }
    toward.given = 1;
  }
  if (n == 0) return GR_OK;
  GR_REQUIRE(query && neighbors && normals && (support || M == 0), "cloud normals: null query, support, neighbors or normals");
  (void)ws;
  (void)ws_bytes;
  KernelTimer timer("cloud_normals", stream);
  const unsigned blocks = (unsigned)((n + NORMALS_THREADS - 1) / NORMALS_THREADS);
  hipLaunchKernelGGL(normals_kernel, dim3(blocks), dim3(NORMALS_THREADS), 0, stream, query, n, support, M, neighbors, k,
                     include_self, toward, normals, curvature, valid);
  GR_LAUNCH_CHECK();
  return GR_OK;
}
