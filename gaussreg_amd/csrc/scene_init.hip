// Scene initialisation from a point cloud: the exact k nearest neighbours of every point of ONE cloud,
// what upstream 3DGS's create_from_pcd takes from simple_knn.distCUDA2.
//
// The result is defined by exhaustive enumeration (include/gaussreg_hip.h): d(i, j) = ((dx*dx + dy*dy) + dz*dz) in fp32,
// neighbours = the k smallest j != i under the order (d, j).  That order is total, so the k smallest do not depend on the
// order in which candidates are met: any search that meets every point that can be among them gives the same bits.
//
// Search structure: a rectilinear grid of D x D x D cells whose cell boundaries are, per axis, quantiles of a fixed
// sample of the coordinates (D ~ cbrt(n / 3), at most 128).  A uniform cloud gets a uniform grid; a clustered cloud or
// one with far outliers still gets a few points per occupied cell, where a uniform grid over the bounding box would put
// the bulk into one cell.  Boundaries are coordinates, cells are found by comparing floats, so there is no rounding
// between a point and its cell:  cell_a(x) = #{c in 1 .. D-1 : B_a[c] <= x}.
//
//   gs_knn_boundaries_kernel  one workgroup per axis: 4096 strided samples, bitonic sort in LDS, B_a[c] = sample[c 4096 / D];
//   gs_knn_count_kernel       one thread per point: its cell (binary search in LDS), the cell's count (integer atomic),
//                             the finiteness flag;
//   (exclusive_scan_i32 of the counts)
//   gs_knn_scatter_kernel     one thread per point: (x, y, z, index) into cell order (integer atomic cursor; the order
//                             inside a cell varies from run to run and the result does not depend on it);
//   gs_knn_query_kernel<CAP>  one thread per cell-ordered point: scans Chebyshev shells of cells around its own cell,
//                             keeps the CAP best in registers, stops when the CAP-th best is below the stopping bound.
//
// Stopping bound, exact in fp32 without any slack.  After shell r the scanned block is cells [c - r, c + r] per axis.
// A point outside it differs by more than r cells on some axis, say x upwards: then x_p >= B[cx + r + 1] >= x_q, and
// because fp32 subtraction, multiplication and addition of non-negative terms are monotone,
//   fl(x_p - x_q) >= g = fl(B[cx + r + 1] - x_q),  fl(dx dx) >= fl(g g),  d(q, p) >= fl(dx dx) >= fl(g g).
// Downwards x_p < B[cx - r] <= x_q gives the same with g = fl(x_q - B[cx - r]).  bound = min over the (at most six) faces
// that have cells behind them; the search stops iff best[CAP - 1].d < bound, strictly, since a point at the same distance
// with a lower index would displace it.  Shells are clamped to the grid; a query that has not stopped after MAX_SHELLS
// shells (an outlier among empty cells, a cloud of identical points) starts over and scans every point.
#include <cmath>

#include "common.hpp"

namespace gr {
namespace {

constexpr int THREADS = 256;
constexpr int QUERY_THREADS = 128;
constexpr int DMAX = 128;            // cells per axis, at most
constexpr int SAMPLES = 4096;        // per axis, for the quantiles
constexpr int SORT_THREADS = 1024;
constexpr int MAX_SHELLS = 8;
constexpr double POINTS_PER_CELL = 3.0;

int grid_dim(int64_t n) {
  int d = (int)std::floor(std::cbrt((double)n / POINTS_PER_CELL));
  return d < 1 ? 1 : d > DMAX ? DMAX : d;
}

// B: (3, DMAX) floats; B[a * DMAX + c], c in 1 .. D-1, ascending
__global__ __launch_bounds__(SORT_THREADS) void gs_knn_boundaries_kernel(const float* __restrict__ points, int64_t n, int D,
                                                                         float* __restrict__ B) {
  __shared__ uint32_t key[SAMPLES];
  const int a = blockIdx.x;
  for (int t = threadIdx.x; t < SAMPLES; t += SORT_THREADS) {
    const int64_t i = (int64_t)t * n / SAMPLES;
    key[t] = f2ord(points[3 * i + a]);
  }
  __syncthreads();
  for (int k = 2; k <= SAMPLES; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < SAMPLES; t += SORT_THREADS) {
        const int u = t ^ j;
        if (u > t) {
          const uint32_t x = key[t], y = key[u];
          if ((x > y) == ((t & k) == 0)) {
            key[t] = y;
            key[u] = x;
          }
        }
      }
      __syncthreads();
    }
  }
  for (int c = 1 + threadIdx.x; c < D; c += SORT_THREADS) B[a * DMAX + c] = ord2f(key[(int64_t)c * SAMPLES / D]);
}

// #{c in 1 .. D-1 : b[c] <= x}
__device__ __forceinline__ int axis_cell(const float* b, int D, float x) {
  int lo = 0, hi = D - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (b[mid] <= x) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(THREADS) void gs_knn_count_kernel(const float* __restrict__ points, int64_t n, int D,
                                                               const float* __restrict__ B, int32_t* __restrict__ cell,
                                                               int32_t* __restrict__ count, int32_t* __restrict__ flag) {
  __shared__ float b[3 * DMAX];
  for (int t = threadIdx.x; t < 3 * DMAX; t += THREADS) b[t] = (t % DMAX) >= 1 && (t % DMAX) < D ? B[t] : 0.f;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (i >= n) return;
  const float x = points[3 * i], y = points[3 * i + 1], z = points[3 * i + 2];
  if (!(isfinite(x) && isfinite(y) && isfinite(z))) atomicOr(flag, 1);
  const int cx = axis_cell(b, D, x), cy = axis_cell(b + DMAX, D, y), cz = axis_cell(b + 2 * DMAX, D, z);
  const int32_t c = (cz * D + cy) * D + cx;
  cell[i] = c;
  atomicAdd(&count[c], 1);
}

__global__ __launch_bounds__(THREADS) void gs_knn_scatter_kernel(const float* __restrict__ points, int64_t n,
                                                                 const int32_t* __restrict__ cell,
                                                                 const int32_t* __restrict__ start, int32_t* __restrict__ cursor,
                                                                 float4* __restrict__ sorted, int32_t* __restrict__ sorted_cell) {
  const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (i >= n) return;
  const int32_t c = cell[i];
  const int32_t pos = start[c] + atomicAdd(&cursor[c], 1);
  sorted[pos] = make_float4(points[3 * i], points[3 * i + 1], points[3 * i + 2], __int_as_float((int32_t)i));
  sorted_cell[pos] = c;
}

// insert (d, j) into the ascending list of the CAP best under the order (d, j); indices are compile-time after unrolling
template <int CAP>
__device__ __forceinline__ void consider(float (&bd)[CAP], int32_t (&bj)[CAP], float d, int32_t j) {
  if (d < bd[CAP - 1] || (d == bd[CAP - 1] && j < bj[CAP - 1])) {
    bd[CAP - 1] = d;
    bj[CAP - 1] = j;
#pragma unroll
    for (int t = CAP - 1; t > 0; --t) {
      const bool up = bd[t] < bd[t - 1] || (bd[t] == bd[t - 1] && bj[t] < bj[t - 1]);
      const float d0 = bd[t - 1], d1 = bd[t];
      const int32_t j0 = bj[t - 1], j1 = bj[t];
      bd[t - 1] = up ? d1 : d0;
      bd[t] = up ? d0 : d1;
      bj[t - 1] = up ? j1 : j0;
      bj[t] = up ? j0 : j1;
    }
  }
}

template <int CAP>
__device__ __forceinline__ void scan_range(const float4* __restrict__ sorted, int32_t begin, int32_t end, float qx, float qy,
                                           float qz, int32_t qi, float (&bd)[CAP], int32_t (&bj)[CAP]) {
  for (int32_t s = begin; s < end; ++s) {
    const float4 p = sorted[s];
    const int32_t j = __float_as_int(p.w);
    const float dx = p.x - qx, dy = p.y - qy, dz = p.z - qz;
    const float d = (dx * dx + dy * dy) + dz * dz;
    if (j != qi) consider<CAP>(bd, bj, d, j);
  }
}

// fl(g g) of the two faces of one axis behind which there are cells
__device__ __forceinline__ float axis_bound(const float* __restrict__ b, int D, int c, int r, float q) {
  float bound = INFINITY;
  if (c + r + 1 <= D - 1) {
    const float g = b[c + r + 1] - q;
    bound = g * g;
  }
  if (c - r >= 1) {
    const float g = q - b[c - r];
    bound = fminf(bound, g * g);
  }
  return bound;
}

template <int CAP>
__global__ __launch_bounds__(QUERY_THREADS) void gs_knn_query_kernel(const float4* __restrict__ sorted,
                                                                     const int32_t* __restrict__ sorted_cell,
                                                                     const int32_t* __restrict__ start, const float* __restrict__ B,
                                                                     int32_t n, int D, int k, float* __restrict__ dist2,
                                                                     int64_t* __restrict__ index, float* __restrict__ mean) {
  const int64_t s = (int64_t)blockIdx.x * QUERY_THREADS + threadIdx.x;
  if (s >= n) return;
  const float4 q = sorted[s];
  const int32_t qi = __float_as_int(q.w);
  const int32_t c = sorted_cell[s];
  const int cx = c % D, cy = (c / D) % D, cz = c / (D * D);
  float bd[CAP];
  int32_t bj[CAP];
#pragma unroll
  for (int t = 0; t < CAP; ++t) {
    bd[t] = INFINITY;
    bj[t] = 0x7fffffff;
  }
  for (int r = 0;; ++r) {
    const int x0 = max(cx - r, 0), x1 = min(cx + r, D - 1);
    const int y0 = max(cy - r, 0), y1 = min(cy + r, D - 1);
    const int z0 = max(cz - r, 0), z1 = min(cz + r, D - 1);
    for (int z = z0; z <= z1; ++z) {
      for (int y = y0; y <= y1; ++y) {
        const int32_t row = (z * D + y) * D;
        if (z == cz - r || z == cz + r || y == cy - r || y == cy + r) {  // a face of the shell: cells x0 .. x1 are contiguous
          scan_range<CAP>(sorted, start[row + x0], start[row + x1 + 1], q.x, q.y, q.z, qi, bd, bj);
        } else {  // inside: the two end cells (r > 0 here)
          if (cx - r >= 0) scan_range<CAP>(sorted, start[row + cx - r], start[row + cx - r + 1], q.x, q.y, q.z, qi, bd, bj);
          if (cx + r <= D - 1) scan_range<CAP>(sorted, start[row + cx + r], start[row + cx + r + 1], q.x, q.y, q.z, qi, bd, bj);
        }
      }
    }
    const float bound = fminf(axis_bound(B, D, cx, r, q.x), fminf(axis_bound(B + DMAX, D, cy, r, q.y), axis_bound(B + 2 * DMAX, D, cz, r, q.z)));
    if (bd[CAP - 1] < bound) break;
    if (x1 - x0 == D - 1 && y1 - y0 == D - 1 && z1 - z0 == D - 1) break;  // the whole grid has been scanned
    if (r + 1 == MAX_SHELLS) {  // start over, every point
#pragma unroll
      for (int t = 0; t < CAP; ++t) {
        bd[t] = INFINITY;
        bj[t] = 0x7fffffff;
      }
      scan_range<CAP>(sorted, 0, n, q.x, q.y, q.z, qi, bd, bj);
      break;
    }
  }
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < CAP; ++t) {
    if (t < k) {
      if (dist2) dist2[(int64_t)qi * k + t] = bd[t];
      if (index) index[(int64_t)qi * k + t] = bj[t];
      sum = t == 0 ? bd[0] : sum + bd[t];
    }
  }
  if (mean) mean[qi] = sum / (float)k;
}

struct KnnWorkspace {
  float* B;             // (3, DMAX)
  int32_t* count;       // cells + 1, then the exclusive prefix in place
  int32_t* cursor;      // cells
  int32_t* flag;        // 1; count, cursor and flag are contiguous for one memset
  int32_t* scan_ws;
  int32_t* cell;        // n
  int32_t* sorted_cell; // n
  float4* sorted;       // n
  size_t zero_bytes;    // from count
  size_t bytes;
};

KnnWorkspace carve_knn(void* ws, int64_t n) {
  const int D = grid_dim(n);
  const size_t cells = (size_t)D * D * D;
  Carver c(ws);
  KnnWorkspace w;
  w.B = c.take<float>(3 * DMAX);
  w.count = c.take<int32_t>(2 * cells + 2);
  w.cursor = w.count + cells + 1;
  w.flag = w.cursor + cells;
  w.zero_bytes = (2 * cells + 2) * sizeof(int32_t);
  w.scan_ws = c.take<int32_t>(scan_ws_ints((int64_t)cells + 1));
  w.cell = c.take<int32_t>((size_t)n);
  w.sorted_cell = c.take<int32_t>((size_t)n);
  w.sorted = c.take<float4>((size_t)n);
  w.bytes = c.used();
  return w;
}

bool knn_shape_ok(int64_t n, int k) { return k >= 1 && k <= GR_GS_KNN_MAX_K && n > k && n < (1ll << 31); }

}  // namespace
}  // namespace gr

using namespace gr;

extern "C" size_t gr_gs_knn_workspace_bytes(int64_t n, int k) {
  if (!knn_shape_ok(n, k)) return 0;
  return carve_knn(nullptr, n).bytes;
}

extern "C" int gr_gs_knn(const float* points, int64_t n, int k, float* dist2, int64_t* index, float* mean, void* ws,
                         size_t ws_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  GR_REQUIRE(k >= 1 && k <= GR_GS_KNN_MAX_K, "gs knn: k = %d outside [1, %d]", k, GR_GS_KNN_MAX_K);
  GR_REQUIRE(n > k && n < (1ll << 31), "gs knn: n = %lld outside (k, 2^31)", (long long)n);
  GR_REQUIRE(points, "gs knn: null points");
  const KnnWorkspace w = carve_knn(ws, n);
  if (!ws || ws_bytes < w.bytes) {
    set_error("gs knn: workspace of %zu bytes, %zu needed", ws_bytes, w.bytes);
    return GR_ERR_WORKSPACE;
  }
  const int D = grid_dim(n);
  const int64_t cells = (int64_t)D * D * D;
  const unsigned blocks = (unsigned)((n + THREADS - 1) / THREADS);
  int32_t h_flag = 0;
  {
    KernelTimer timer("gs_knn_grid", stream);
    GR_HIP(hipMemsetAsync(w.count, 0, w.zero_bytes, stream));
    if (D > 1) {
      hipLaunchKernelGGL(gs_knn_boundaries_kernel, dim3(3), dim3(SORT_THREADS), 0, stream, points, n, D, w.B);
      GR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(gs_knn_count_kernel, dim3(blocks), dim3(THREADS), 0, stream, points, n, D, w.B, w.cell, w.count, w.flag);
    GR_LAUNCH_CHECK();
    const int rc = exclusive_scan_i32(w.count, w.count, cells + 1, 1, cells + 1, w.scan_ws, nullptr, stream);
    if (rc != GR_OK) return rc;
    hipLaunchKernelGGL(gs_knn_scatter_kernel, dim3(blocks), dim3(THREADS), 0, stream, points, n, w.cell, w.count, w.cursor,
                       w.sorted, w.sorted_cell);
    GR_LAUNCH_CHECK();
  }
  // the one host read-back of a call
  GR_HIP(hipMemcpyAsync(&h_flag, w.flag, sizeof h_flag, hipMemcpyDeviceToHost, stream));
  GR_HIP(hipStreamSynchronize(stream));
  GR_REQUIRE(h_flag == 0, "gs knn: points must be finite");
  if (!dist2 && !index && !mean) return GR_OK;
  const unsigned qblocks = (unsigned)((n + QUERY_THREADS - 1) / QUERY_THREADS);
  KernelTimer timer("gs_knn_query", stream);
#define GR_KNN_LAUNCH(CAP)                                                                                                  \
  hipLaunchKernelGGL(gs_knn_query_kernel<CAP>, dim3(qblocks), dim3(QUERY_THREADS), 0, stream, w.sorted, w.sorted_cell, w.count, \
                     w.B, (int32_t)n, D, k, dist2, index, mean)
  if (k == 1) GR_KNN_LAUNCH(1);
  else if (k <= 3) GR_KNN_LAUNCH(3);
  else if (k <= 5) GR_KNN_LAUNCH(5);
  else GR_KNN_LAUNCH(8);
#undef GR_KNN_LAUNCH
  GR_LAUNCH_CHECK();
  return GR_OK;
}
