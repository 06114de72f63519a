// Cross-cloud nearest neighbours: for every point of a QUERY cloud the nearest points of a SUPPORT cloud,
// and every (query, support) pair within a radius -- what the reference takes from scipy's cKDTree for overlap,
// ground-truth correspondences and the evaluation metrics.
//
// The result is defined by exhaustive enumeration (include/gaussreg_hip_cloud.h): d(i, j) = ((dx*dx + dy*dy) + dz*dz) in
// fp32, candidates ordered by (d, j), nothing excluded.  The order is total, so any search that meets every point that
// can be among the answer gives the same bits.
//
// Search structure: the per-axis quantile grid of cloud_grid.hpp (where the shell loop, the face bound and its proof are),
// built over the SUPPORT.  The outermost cells are unbounded, so a query that lies outside the support's bulk still lies
// INSIDE its cell and the face bound needs no special case for it.  The queries are put into cell order too (the same
// count / scan / scatter), so the lanes of a wave walk neighbouring cells.
//
//   cloud_boundaries_kernel   one workgroup per axis: 4096 strided samples of the support, bitonic sort in LDS,
//                             B_a[c] = sample[c 4096 / D];
//   cloud_box_kernel          the support's exact bounding box (integer atomic max of order-preserving words);
//   cloud_cell_kernel         one thread per point (either cloud): its cell, the cell's count, the finiteness flag;
//   (exclusive_scan_i32 of the counts)
//   cloud_scatter_kernel      one thread per point: (x, y, z, index) into cell order (integer atomic cursor; the order
//                             inside a cell varies from run to run and the result does not depend on it);
//   cloud_knn_query_kernel<CAP>     one thread per cell-ordered query: Chebyshev shells of cells around its cell, CAP best
//                                   in registers; a query that no rule stops within MAX_SHELLS shells is appended to a list;
//   cloud_knn_fallback_kernel<CAP>  one WAVE per listed query: the 64 lanes walk strided parts of the whole support, each
//                                   keeps its own CAP best, merged by CAP wave-wide minima of the 64-bit key (d bits, j);
//   cloud_radius_kernel<EMIT>       one thread per cell-ordered query: scans the block of cells the radius can reach,
//                                   counts (EMIT = false) or writes the j of its hits in scan order (EMIT = true);
//   cloud_radius_order_kernel       one lane per short row, the wave per long row: rank of every hit by j, (i, j) written.
//
// What this search adds to the face bound (the query need not be a support point):
//   * the cap: cells [L_a, H_a] per axis are those a point with d <= cap can lie in (walk outwards from the query's cell
//     while fl(g g) <= cap: g grows with the distance, so the first failure ends the walk).  Everything outside that block
//     is beyond the cap.  Without a cap the block is the whole grid.  "The bound exceeds the cap" needs no rule of its own:
//     a face beyond the cap has no cell of the block behind it.
//   * the box term: each face's fl(g g) is added -- in d's own association -- to the squared distance of the query from the
//     support's bounding box on the two OTHER axes (0 for a query inside it): a point behind an x face is at least the
//     face away in x and at least the box away in y and z.  For a query beside the support (the non-overlapping part of
//     a pair) that term is what ends the search after the shell that holds its neighbours; the faces alone never would.
#include <cmath>

#include "../../include/gaussreg_hip_cloud.h"
#include "cloud_grid.hpp"

namespace gr {
namespace {

constexpr int SAMPLES = 4096;        // per axis, for the quantiles
constexpr int SORT_THREADS = 1024;
constexpr int SHORT_ROW = 32;        // radius rows of at most this many hits are ordered by one lane
constexpr int BOX_BLOCKS = 256;
constexpr double POINTS_PER_CELL = 3.0;

// B: (3, DMAX) floats; B[a * DMAX + c], c in 1 .. D-1, ascending
__global__ __launch_bounds__(SORT_THREADS) void cloud_boundaries_kernel(const float* __restrict__ points, int64_t n, int D,
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

__global__ __launch_bounds__(THREADS) void cloud_cell_kernel(const float* __restrict__ points, int64_t n, int D,
                                                             const float* __restrict__ B, int32_t* __restrict__ cell,
                                                             int32_t* __restrict__ count, int32_t* __restrict__ flag) {
  __shared__ float b[3 * DMAX];
  stage_boundaries(B, D, b);
  const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (i >= n) return;
  const float x = points[3 * i], y = points[3 * i + 1], z = points[3 * i + 2];
  if (!(isfinite(x) && isfinite(y) && isfinite(z))) atomicOr(flag, 1);
  const int cx = axis_cell(b, D, x), cy = axis_cell(b + DMAX, D, y), cz = axis_cell(b + 2 * DMAX, D, z);
  const int32_t c = (cz * D + cy) * D + cx;
  cell[i] = c;
  atomicAdd(&count[c], 1);
}

// The support's bounding box, exact: box[a] = max of ~f2ord(coordinate a) (the minimum, complemented so that a zeroed word
// is the identity), box[3 + a] = max of f2ord.  Integer atomics, one set per wave.
__global__ __launch_bounds__(THREADS) void cloud_box_kernel(const float* __restrict__ points, int64_t n, uint32_t* __restrict__ box) {
  uint32_t v[6] = {0u, 0u, 0u, 0u, 0u, 0u};
  for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * THREADS) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const uint32_t o = f2ord(points[3 * i + a]);
      v[a] = max(v[a], ~o);
      v[3 + a] = max(v[3 + a], o);
    }
  }
#pragma unroll
  for (int a = 0; a < 6; ++a) {  // every lane of the wave is here
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[a] = max(v[a], (uint32_t)__shfl_xor((int)v[a], o));
    if ((threadIdx.x & (WAVE - 1)) == 0) atomicMax(&box[a], v[a]);
  }
}

// sorted_cell: null for a support whose cells nobody asks for again
__global__ __launch_bounds__(THREADS) void cloud_scatter_kernel(const float* __restrict__ points, int64_t n,
                                                                const int32_t* __restrict__ cell,
                                                                const int32_t* __restrict__ start, int32_t* __restrict__ cursor,
                                                                float4* __restrict__ sorted, int32_t* __restrict__ sorted_cell) {
  const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (i >= n) return;
  const int32_t c = cell[i];
  const int32_t pos = start[c] + atomicAdd(&cursor[c], 1);
  sorted[pos] = make_float4(points[3 * i], points[3 * i + 1], points[3 * i + 2], __int_as_float((int32_t)i));
  if (sorted_cell) sorted_cell[pos] = c;
}

template <int CAP>
__device__ __forceinline__ void write_row(float* __restrict__ dist2, int64_t* __restrict__ index, int64_t qi, int k, int t,
                                          float d, int32_t j) {
  if (t < k) {
    if (dist2) dist2[qi * k + t] = j == NONE ? INFINITY : d;
    if (index) index[qi * k + t] = j == NONE ? -1 : (int64_t)j;
  }
}

template <int CAP>
__global__ __launch_bounds__(QUERY_THREADS) void cloud_knn_query_kernel(
    const float4* __restrict__ s_sorted, const int32_t* __restrict__ s_start, const float4* __restrict__ q_sorted,
    const int32_t* __restrict__ q_sorted_cell, const float* __restrict__ B, const uint32_t* __restrict__ box, int32_t nq, int D,
    int k, float cap, float* __restrict__ dist2, int64_t* __restrict__ index, int32_t* __restrict__ list,
    int32_t* __restrict__ list_count) {
  const int64_t s = (int64_t)blockIdx.x * QUERY_THREADS + threadIdx.x;
  if (s >= nq) return;
  const float4 q = q_sorted[s];
  const int32_t c = q_sorted_cell[s];
  float bd[CAP];
  int32_t bj[CAP];
  clear_best<CAP>(bd, bj);
  if (!shell_search<CAP>(s_sorted, s_start, B, box, D, c, q.x, q.y, q.z, cap, bd, bj)) {
    list[atomicAdd(list_count, 1)] = (int32_t)s;  // a wave of the second launch starts over and scans every point
    return;
  }
  const int64_t qi = __float_as_int(q.w);
#pragma unroll
  for (int t = 0; t < CAP; ++t) write_row<CAP>(dist2, index, qi, k, t, bd[t], bj[t]);
}

template <int CAP>
__global__ __launch_bounds__(THREADS) void cloud_knn_fallback_kernel(const float4* __restrict__ s_sorted, int32_t ns,
                                                                     const float4* __restrict__ q_sorted,
                                                                     const int32_t* __restrict__ list,
                                                                     const int32_t* __restrict__ list_count, int k, float cap,
                                                                     float* __restrict__ dist2, int64_t* __restrict__ index) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int nlist = *list_count;
  constexpr int WAVES = THREADS / WAVE;
  for (int w = blockIdx.x * WAVES + (threadIdx.x / WAVE); w < nlist; w += gridDim.x * WAVES) {  // uniform in the wave
    const float4 q = q_sorted[list[w]];
    float bd[CAP];
    int32_t bj[CAP];
    clear_best<CAP>(bd, bj);
    for (int64_t s = lane; s < ns; s += WAVE) {
      const float4 p = s_sorted[s];
      const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
      const float d = (dx * dx + dy * dy) + dz * dz;
      if (d <= cap) consider<CAP>(bd, bj, d, __float_as_int(p.w));
    }
    // d >= +0, so its bits order as it does; every support point is in one lane's list at most, so the keys of real
    // candidates are distinct and exactly one lane owns the minimum
    const int64_t qi = __float_as_int(q.w);
#pragma unroll
    for (int t = 0; t < CAP; ++t) {
      const uint64_t key = ((uint64_t)__float_as_uint(bd[0]) << 32) | (uint32_t)bj[0];
      const uint64_t m = wave_min_u64(key);
      if (lane == 0) write_row<CAP>(dist2, index, qi, k, t, __uint_as_float((uint32_t)(m >> 32)), (int32_t)(uint32_t)m);
      if (key == m && bj[0] != NONE) {  // the owner pops its head
#pragma unroll
        for (int u = 0; u + 1 < CAP; ++u) {
          bd[u] = bd[u + 1];
          bj[u] = bj[u + 1];
        }
        bd[CAP - 1] = INFINITY;
        bj[CAP - 1] = NONE;
      }
    }
  }
}

// EMIT = false: count[qi] (and user_count[qi]) = #{j : d <= r2}, *total += it.  EMIT = true: count holds the exclusive
// prefix; the j of the hits go to row_scratch[count[qi] ..] in scan order.
template <bool EMIT>
__global__ __launch_bounds__(QUERY_THREADS) void cloud_radius_kernel(
    const float4* __restrict__ s_sorted, const int32_t* __restrict__ s_start, const float4* __restrict__ q_sorted,
    const int32_t* __restrict__ q_sorted_cell, const float* __restrict__ B, int32_t nq, int D, float r2,
    int32_t* __restrict__ count, int32_t* __restrict__ user_count, unsigned long long* __restrict__ total,
    int32_t* __restrict__ row_scratch) {
  const int64_t s = (int64_t)blockIdx.x * QUERY_THREADS + threadIdx.x;
  int32_t hits = 0;
  if (s < nq) {
    const float4 q = q_sorted[s];
    const int32_t qi = __float_as_int(q.w);
    const int32_t c = q_sorted_cell[s];
    const int cx = c % D, cy = (c / D) % D, cz = c / (D * D);
    int Lx, Hx, Ly, Hy, Lz, Hz;
    axis_reach(B, D, cx, q.x, r2, Lx, Hx);
    axis_reach(B + DMAX, D, cy, q.y, r2, Ly, Hy);
    axis_reach(B + 2 * DMAX, D, cz, q.z, r2, Lz, Hz);
    int32_t out = EMIT ? count[qi] : 0;
    for (int z = Lz; z <= Hz; ++z) {
      for (int y = Ly; y <= Hy; ++y) {
        const int32_t row = (z * D + y) * D;
        const int32_t end = s_start[row + Hx + 1];
        for (int32_t t = s_start[row + Lx]; t < end; ++t) {
          const float4 p = s_sorted[t];
          const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
          const float d = (dx * dx + dy * dy) + dz * dz;
          if (d <= r2) {
            if (EMIT) row_scratch[out++] = __float_as_int(p.w);
            else ++hits;
          }
        }
      }
    }
    if (!EMIT) {
      count[qi] = hits;
      if (user_count) user_count[qi] = hits;
    }
  }
  if (!EMIT) {  // every lane is still here: one 64-bit integer atomic per wave
    unsigned long long v = (unsigned long long)hits;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & (WAVE - 1)) == 0 && v) atomicAdd(total, v);
  }
}

// off: the exclusive prefix of the counts (nq + 1).  The j of a row are distinct, so the rank of one among them is its
// place in ascending order.
__global__ __launch_bounds__(THREADS) void cloud_radius_order_kernel(const int32_t* __restrict__ off,
                                                                     const int32_t* __restrict__ row_scratch, int32_t nq,
                                                                     int64_t* __restrict__ pairs) {
  const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  const int lane = threadIdx.x & (WAVE - 1);
  int32_t o = 0, h = 0;
  if (i < nq) {
    o = off[i];
    h = off[i + 1] - o;
  }
  if (h <= SHORT_ROW) {
    for (int32_t a = 0; a < h; ++a) {
      const int32_t ja = row_scratch[o + a];
      int32_t rank = 0;
      for (int32_t b = 0; b < h; ++b) rank += row_scratch[o + b] < ja;
      pairs[2 * (int64_t)(o + rank)] = i;
      pairs[2 * (int64_t)(o + rank) + 1] = ja;
    }
  }
  unsigned long long big = __ballot(h > SHORT_ROW);
  while (big) {  // uniform in the wave
    const int l = __ffsll(big) - 1;
    big &= big - 1;
    const int32_t ro = __shfl(o, l), rh = __shfl(h, l);
    const int64_t ri = i - lane + l;
    for (int32_t a = lane; a < rh; a += WAVE) {
      const int32_t ja = row_scratch[ro + a];
      int32_t rank = 0;
      for (int32_t b = 0; b < rh; ++b) rank += row_scratch[ro + b] < ja;
      pairs[2 * (int64_t)(ro + rank)] = ri;
      pairs[2 * (int64_t)(ro + rank) + 1] = ja;
    }
  }
}

struct CloudWorkspace {
  float* B;               // (3, DMAX)
  int32_t* s_count;       // cells + 1, then the exclusive prefix in place
  int32_t* q_count;       // cells + 1, likewise
  int32_t* s_cursor;      // cells
  int32_t* q_cursor;      // cells
  int32_t* misc;          // [0] finiteness flag, [1] length of the fallback list, [2..3] the 64-bit total of the radius count,
                          // [4..9] the support's bounding box (cloud_box_kernel)
  int32_t* scan_ws;
  int32_t* s_cell;        // ns
  int32_t* q_cell;        // nq
  int32_t* q_sorted_cell; // nq
  int32_t* list;          // nq: cell-order positions of the queries left to the fallback
  int32_t* row_count;     // nq + 1: hits per query, then the exclusive prefix in place
  float4* s_sorted;       // ns
  float4* q_sorted;       // nq
  size_t zero_bytes;      // from s_count: counts, cursors and misc are contiguous for one memset
  size_t bytes;
};

CloudWorkspace carve_cloud(void* ws, int64_t nq, int64_t ns) {
  const int D = cloud_grid_dim(ns);
  const size_t cells = (size_t)D * D * D;
  Carver c(ws);
  CloudWorkspace w;
  w.B = c.take<float>(3 * DMAX);
  w.s_count = c.take<int32_t>(4 * cells + 2 + MISC);
  w.q_count = w.s_count + cells + 1;
  w.s_cursor = w.q_count + cells + 1;
  w.q_cursor = w.s_cursor + cells;
  w.misc = w.q_cursor + cells;  // an even number of ints from a 256-byte boundary: misc + 2 is 8-byte aligned
  w.zero_bytes = (4 * cells + 2 + MISC) * sizeof(int32_t);
  const int64_t longest = (int64_t)cells + 1 > nq + 1 ? (int64_t)cells + 1 : nq + 1;
  w.scan_ws = c.take<int32_t>(scan_ws_ints(longest));
  w.s_cell = c.take<int32_t>((size_t)ns);
  w.q_cell = c.take<int32_t>((size_t)nq);
  w.q_sorted_cell = c.take<int32_t>((size_t)nq);
  w.list = c.take<int32_t>((size_t)nq);
  w.row_count = c.take<int32_t>((size_t)nq + 1);
  w.s_sorted = c.take<float4>((size_t)ns);
  w.q_sorted = c.take<float4>((size_t)nq);
  w.bytes = c.used();
  return w;
}

bool clouds_ok(int64_t nq, int64_t ns) { return nq >= 0 && nq < (1ll << 31) && ns >= 1 && ns < (1ll << 31); }

// grid over the support, both clouds in cell order, the finiteness flag raised in w.misc[0]; nq >= 1
int build_grids(const float* query, int64_t nq, const float* support, int64_t ns, const CloudWorkspace& w, hipStream_t stream) {
  const int D = cloud_grid_dim(ns);
  const int64_t cells = (int64_t)D * D * D;
  const unsigned qblocks = (unsigned)((nq + THREADS - 1) / THREADS);
  KernelTimer timer("cloud_nn_grid", stream);
  const SupportGrid g = {w.B, w.s_count, w.s_cursor, w.misc, w.scan_ws, w.s_cell, w.s_sorted};
  int rc = cloud_build_support_grid(support, ns, g, w.s_count, w.zero_bytes, stream);
  if (rc != GR_OK) return rc;
  hipLaunchKernelGGL(cloud_cell_kernel, dim3(qblocks), dim3(THREADS), 0, stream, query, nq, D, w.B, w.q_cell, w.q_count, w.misc);
  GR_LAUNCH_CHECK();
  rc = exclusive_scan_i32(w.q_count, w.q_count, cells + 1, 1, cells + 1, w.scan_ws, nullptr, stream);
  if (rc != GR_OK) return rc;
  hipLaunchKernelGGL(cloud_scatter_kernel, dim3(qblocks), dim3(THREADS), 0, stream, query, nq, w.q_cell, w.q_count, w.q_cursor,
                     w.q_sorted, w.q_sorted_cell);
  GR_LAUNCH_CHECK();
  return GR_OK;
}

}  // namespace

int cloud_grid_dim(int64_t n) {
  int d = (int)std::floor(std::cbrt((double)n / POINTS_PER_CELL));
  return d < 1 ? 1 : d > DMAX ? DMAX : d;
}

int cloud_build_support_grid(const float* support, int64_t ns, const SupportGrid& g, void* zero_from, size_t zero_bytes,
                             hipStream_t stream, bool with_box) {
  const int D = cloud_grid_dim(ns);
  const int64_t cells = (int64_t)D * D * D;
  const unsigned sblocks = (unsigned)((ns + THREADS - 1) / THREADS);
  GR_HIP(hipMemsetAsync(zero_from, 0, zero_bytes, stream));
  if (D > 1) {
    hipLaunchKernelGGL(cloud_boundaries_kernel, dim3(3), dim3(SORT_THREADS), 0, stream, support, ns, D, g.B);
    GR_LAUNCH_CHECK();
  }
  if (with_box) {
    hipLaunchKernelGGL(cloud_box_kernel, dim3(sblocks < BOX_BLOCKS ? sblocks : BOX_BLOCKS), dim3(THREADS), 0, stream, support,
                       ns, reinterpret_cast<uint32_t*>(g.misc + 4));
    GR_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(cloud_cell_kernel, dim3(sblocks), dim3(THREADS), 0, stream, support, ns, D, g.B, g.cell, g.count, g.misc);
  GR_LAUNCH_CHECK();
  const int rc = exclusive_scan_i32(g.count, g.count, cells + 1, 1, cells + 1, g.scan_ws, nullptr, stream);
  if (rc != GR_OK) return rc;
  hipLaunchKernelGGL(cloud_scatter_kernel, dim3(sblocks), dim3(THREADS), 0, stream, support, ns, g.cell, g.count, g.cursor,
                     g.sorted, g.sorted_cell);
  GR_LAUNCH_CHECK();
  return GR_OK;
}

}  // namespace gr

using namespace gr;

extern "C" size_t gr_cloud_knn_workspace_bytes(int64_t nq, int64_t ns, int k) {
  if (!clouds_ok(nq, ns) || k < 1 || k > GR_CLOUD_KNN_MAX_K) return 0;
  return carve_cloud(nullptr, nq, ns).bytes;
}

extern "C" int gr_cloud_knn(const float* query, int64_t nq, const float* support, int64_t ns, int k, float max_dist2,
                            float* dist2, int64_t* index, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  GR_REQUIRE(k >= 1 && k <= GR_CLOUD_KNN_MAX_K, "cloud knn: k = %d outside [1, %d]", k, GR_CLOUD_KNN_MAX_K);
  GR_REQUIRE(nq >= 0 && nq < (1ll << 31), "cloud knn: nq = %lld outside [0, 2^31)", (long long)nq);
  GR_REQUIRE(ns >= 1 && ns < (1ll << 31), "cloud knn: ns = %lld outside [1, 2^31)", (long long)ns);
  GR_REQUIRE(max_dist2 >= 0.f, "cloud knn: max_dist2 = %g must be >= 0 (+inf: no cap)", (double)max_dist2);
  GR_REQUIRE(support && (query || nq == 0), "cloud knn: null points");
  const CloudWorkspace w = carve_cloud(ws, nq, ns);
  if (!ws || ws_bytes < w.bytes) {
    set_error("cloud knn: workspace of %zu bytes, %zu needed", ws_bytes, w.bytes);
    return GR_ERR_WORKSPACE;
  }
  if (nq == 0) return GR_OK;
  const int rc = build_grids(query, nq, support, ns, w, stream);
  if (rc != GR_OK) return rc;
  // the one host read-back of a call
  int32_t h_flag = 0;
  GR_HIP(hipMemcpyAsync(&h_flag, w.misc, sizeof h_flag, hipMemcpyDeviceToHost, stream));
  GR_HIP(hipStreamSynchronize(stream));
  GR_REQUIRE(h_flag == 0, "cloud knn: points must be finite");
  if (!dist2 && !index) return GR_OK;
  const int D = cloud_grid_dim(ns);
  const unsigned qblocks = (unsigned)((nq + QUERY_THREADS - 1) / QUERY_THREADS);
  const int64_t waves = (nq + (THREADS / WAVE) - 1) / (THREADS / WAVE);
  const unsigned fblocks = (unsigned)(waves < FALLBACK_BLOCKS ? waves : FALLBACK_BLOCKS);
  KernelTimer timer("cloud_nn_query", stream);
#define GR_CLOUD_KNN_LAUNCH(CAP)                                                                                             \
  do {                                                                                                                       \
    hipLaunchKernelGGL(cloud_knn_query_kernel<CAP>, dim3(qblocks), dim3(QUERY_THREADS), 0, stream, w.s_sorted, w.s_count,    \
                       w.q_sorted, w.q_sorted_cell, w.B, reinterpret_cast<const uint32_t*>(w.misc + 4), (int32_t)nq, D, k,    \
                       max_dist2, dist2, index, w.list, w.misc + 1);                                                        \
    hipLaunchKernelGGL(cloud_knn_fallback_kernel<CAP>, dim3(fblocks), dim3(THREADS), 0, stream, w.s_sorted, (int32_t)ns,     \
                       w.q_sorted, w.list, w.misc + 1, k, max_dist2, dist2, index);                                          \
  } while (0)
  if (k == 1) GR_CLOUD_KNN_LAUNCH(1);
  else if (k <= 3) GR_CLOUD_KNN_LAUNCH(3);
  else if (k <= 5) GR_CLOUD_KNN_LAUNCH(5);
  else GR_CLOUD_KNN_LAUNCH(8);
#undef GR_CLOUD_KNN_LAUNCH
  GR_LAUNCH_CHECK();
  return GR_OK;
}

extern "C" size_t gr_cloud_radius_workspace_bytes(int64_t nq, int64_t ns) {
  if (!clouds_ok(nq, ns)) return 0;
  return carve_cloud(nullptr, nq, ns).bytes;
}

extern "C" int gr_cloud_radius_count(const float* query, int64_t nq, const float* support, int64_t ns, float r2,
                                     int32_t* count, int64_t* h_total, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  GR_REQUIRE(nq >= 0 && nq < (1ll << 31), "cloud radius: nq = %lld outside [0, 2^31)", (long long)nq);
  GR_REQUIRE(ns >= 1 && ns < (1ll << 31), "cloud radius: ns = %lld outside [1, 2^31)", (long long)ns);
  GR_REQUIRE(r2 >= 0.f, "cloud radius: r2 = %g must be >= 0", (double)r2);
  GR_REQUIRE(support && (query || nq == 0) && h_total, "cloud radius: null points or null h_total");
  const CloudWorkspace w = carve_cloud(ws, nq, ns);
  if (!ws || ws_bytes < w.bytes) {
    set_error("cloud radius: workspace of %zu bytes, %zu needed", ws_bytes, w.bytes);
    return GR_ERR_WORKSPACE;
  }
  *h_total = 0;
  if (nq == 0) return GR_OK;
  const int rc = build_grids(query, nq, support, ns, w, stream);
  if (rc != GR_OK) return rc;
  const int D = cloud_grid_dim(ns);
  const unsigned qblocks = (unsigned)((nq + QUERY_THREADS - 1) / QUERY_THREADS);
  {
    KernelTimer timer("cloud_nn_radius", stream);
    GR_HIP(hipMemsetAsync(w.row_count + nq, 0, sizeof(int32_t), stream));
    hipLaunchKernelGGL(cloud_radius_kernel<false>, dim3(qblocks), dim3(QUERY_THREADS), 0, stream, w.s_sorted, w.s_count,
                       w.q_sorted, w.q_sorted_cell, w.B, (int32_t)nq, D, r2, w.row_count, count,
                       reinterpret_cast<unsigned long long*>(w.misc + 2), (int32_t*)nullptr);
    GR_LAUNCH_CHECK();
  }
  // the one host read-back of a call: flag, list length (unused here), total
  int32_t h_misc[4] = {0, 0, 0, 0};
  GR_HIP(hipMemcpyAsync(h_misc, w.misc, sizeof h_misc, hipMemcpyDeviceToHost, stream));
  GR_HIP(hipStreamSynchronize(stream));
  GR_REQUIRE(h_misc[0] == 0, "cloud radius: points must be finite");
  uint64_t total;
  memcpy(&total, h_misc + 2, sizeof total);
  GR_REQUIRE(total < (1ull << 31), "cloud radius: %llu pairs, at most 2^31 - 1", (unsigned long long)total);
  const int rc2 = exclusive_scan_i32(w.row_count, w.row_count, nq + 1, 1, nq + 1, w.scan_ws, nullptr, stream);
  if (rc2 != GR_OK) return rc2;
  *h_total = (int64_t)total;
  return GR_OK;
}

extern "C" int gr_cloud_radius_pairs(const float* query, int64_t nq, const float* support, int64_t ns, float r2, int64_t total,
                                     int32_t* row_scratch, int64_t* pairs, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  GR_REQUIRE(nq >= 0 && nq < (1ll << 31), "cloud radius: nq = %lld outside [0, 2^31)", (long long)nq);
  GR_REQUIRE(ns >= 1 && ns < (1ll << 31), "cloud radius: ns = %lld outside [1, 2^31)", (long long)ns);
  GR_REQUIRE(r2 >= 0.f, "cloud radius: r2 = %g must be >= 0", (double)r2);
  GR_REQUIRE(total >= 0 && total < (1ll << 31), "cloud radius: total = %lld outside [0, 2^31)", (long long)total);
  const CloudWorkspace w = carve_cloud(ws, nq, ns);
  if (!ws || ws_bytes < w.bytes) {
    set_error("cloud radius: workspace of %zu bytes, %zu needed", ws_bytes, w.bytes);
    return GR_ERR_WORKSPACE;
  }
  if (nq == 0) {
    GR_REQUIRE(total == 0, "cloud radius: total = %lld without queries", (long long)total);
    return GR_OK;
  }
  // the emit pass writes total entries: the workspace must be the one the count left, for this very total
  int32_t h_last = -1;
  GR_HIP(hipMemcpyAsync(&h_last, w.row_count + nq, sizeof h_last, hipMemcpyDeviceToHost, stream));
  GR_HIP(hipStreamSynchronize(stream));
  GR_REQUIRE((int64_t)h_last == total, "cloud radius: total = %lld, the workspace holds a count of %d", (long long)total, h_last);
  if (total == 0) return GR_OK;
  GR_REQUIRE(row_scratch && pairs, "cloud radius: null row_scratch or pairs");
  const int D = cloud_grid_dim(ns);
  const unsigned qblocks = (unsigned)((nq + QUERY_THREADS - 1) / QUERY_THREADS);
  const unsigned oblocks = (unsigned)((nq + THREADS - 1) / THREADS);
  KernelTimer timer("cloud_nn_radius", stream);
  hipLaunchKernelGGL(cloud_radius_kernel<true>, dim3(qblocks), dim3(QUERY_THREADS), 0, stream, w.s_sorted, w.s_count, w.q_sorted,
                     w.q_sorted_cell, w.B, (int32_t)nq, D, r2, w.row_count, (int32_t*)nullptr, (unsigned long long*)nullptr,
                     row_scratch);
  GR_LAUNCH_CHECK();
  hipLaunchKernelGGL(cloud_radius_order_kernel, dim3(oblocks), dim3(THREADS), 0, stream, w.row_count, row_scratch, (int32_t)nq,
                     pairs);
  GR_LAUNCH_CHECK();
  return GR_OK;
}
