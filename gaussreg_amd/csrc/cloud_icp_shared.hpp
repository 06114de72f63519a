// What the two ICP loops share (cloud_icp.hip: point-to-point; cloud_icp_plane.hip: point-to-plane, 3.14):
// the fp32 transform, the kernels that order the source once and match it every round, the scatter of the reported
// matches and the workspace.  Each loop adds its own sums and fold kernels.  Everything is in the anonymous namespace, so
// each of the two files compiles its own copy of the kernels.
#pragma once
#include <cmath>

#include "../../include/gaussreg_hip_icp.h"
#include "cloud_grid.hpp"

namespace gr {
namespace {

constexpr int SUM_ITEMS = 8;
constexpr int SUM_CHUNK = THREADS * SUM_ITEMS;  // ordered source points per partial row
constexpr int HISTORY_ROW = 16;
// misc: [0] finiteness flag, [1] length of the fallback list, [2] done, [3] t, [4..9] the support's box, [10] status
constexpr int M_FLAG = 0, M_LIST = 1, M_DONE = 2, M_ITER = 3, M_BOX = 4, M_STATUS = 10;

struct Transform0 {
  float m[12];
};

// p = T x in fp32: ((A[r][0] x + A[r][1] y) + A[r][2] z) + t[r]; the library is built with -ffp-contract=off
__device__ __forceinline__ void apply(const float* __restrict__ T, float x, float y, float z, float& px, float& py, float& pz) {
  px = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
  py = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
  pz = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
}

__global__ __launch_bounds__(WAVE) void icp_init_kernel(Transform0 T0, float* __restrict__ T) {
  if (threadIdx.x < 12) T[threadIdx.x] = T0.m[threadIdx.x];
}

__global__ __launch_bounds__(THREADS) void icp_key_kernel(const float* __restrict__ src, int64_t n, Transform0 T0, int D,
                                                          const float* __restrict__ B, uint64_t* __restrict__ keys,
                                                          int32_t* __restrict__ flag) {
  __shared__ float b[3 * DMAX];
  stage_boundaries(B, D, b);
  const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (i >= n) return;
  const float x = src[3 * i], y = src[3 * i + 1], z = src[3 * i + 2];
  if (!(isfinite(x) && isfinite(y) && isfinite(z))) atomicOr(flag, 1);
  float px, py, pz;
  apply(T0.m, x, y, z, px, py, pz);
  const int cx = axis_cell(b, D, px), cy = axis_cell(b + DMAX, D, py), cz = axis_cell(b + 2 * DMAX, D, pz);
  keys[i] = (uint64_t)((cz * D + cy) * D + cx);
}

__global__ __launch_bounds__(THREADS) void icp_gather_kernel(const float* __restrict__ src, const int32_t* __restrict__ order,
                                                             int64_t n, float4* __restrict__ q_sorted) {
  const int64_t s = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (s >= n) return;
  const int64_t i = order[s];
  q_sorted[s] = make_float4(src[3 * i], src[3 * i + 1], src[3 * i + 2], __int_as_float((int32_t)i));
}

// misc is read (flag, done) and its list length is advanced here, so it is not __restrict__
__global__ __launch_bounds__(QUERY_THREADS) void icp_match_kernel(
    const float4* __restrict__ r_sorted, const int32_t* __restrict__ r_start, const float4* __restrict__ q_sorted,
    const float* __restrict__ B, int32_t* misc, const float* __restrict__ T, int32_t nq, int D, float cap,
    int32_t* __restrict__ match_j, float* __restrict__ match_d, int32_t* __restrict__ list) {
  if (misc[M_FLAG] | misc[M_DONE]) return;
  const int64_t s = (int64_t)blockIdx.x * QUERY_THREADS + threadIdx.x;
  if (s >= nq) return;
  const float4 q = q_sorted[s];
  float px, py, pz;
  apply(T, q.x, q.y, q.z, px, py, pz);
  const int cx = axis_cell(B, D, px), cy = axis_cell(B + DMAX, D, py), cz = axis_cell(B + 2 * DMAX, D, pz);
  float bd[1] = {INFINITY};
  int32_t bj[1] = {NONE};
  if (!shell_search<1>(r_sorted, r_start, B, reinterpret_cast<const uint32_t*>(misc + M_BOX), D, (cz * D + cy) * D + cx, px, py,
                       pz, cap, bd, bj)) {
    list[atomicAdd(&misc[M_LIST], 1)] = (int32_t)s;  // at most nq entries: one per thread
    return;
  }
  match_j[s] = bj[0] == NONE ? -1 : bj[0];
  match_d[s] = bj[0] == NONE ? INFINITY : bd[0];
}

__global__ __launch_bounds__(THREADS) void icp_fallback_kernel(const float4* __restrict__ r_sorted, int32_t ns,
                                                               const float4* __restrict__ q_sorted,
                                                               const int32_t* __restrict__ list,
                                                               const int32_t* __restrict__ misc, const float* __restrict__ T,
                                                               float cap, int32_t* __restrict__ match_j,
                                                               float* __restrict__ match_d) {
  if (misc[M_FLAG] | misc[M_DONE]) return;
  const int lane = threadIdx.x & (WAVE - 1);
  const int nlist = misc[M_LIST];
  constexpr int WAVES = THREADS / WAVE;
  for (int w = blockIdx.x * WAVES + (threadIdx.x / WAVE); w < nlist; w += gridDim.x * WAVES) {  // uniform in the wave
    const int32_t pos = list[w];
    const float4 q = q_sorted[pos];
    float px, py, pz;
    apply(T, q.x, q.y, q.z, px, py, pz);
    float bd[1] = {INFINITY};
    int32_t bj[1] = {NONE};
    for (int64_t s = lane; s < ns; s += WAVE) {
      const float4 p = r_sorted[s];
      const float dx = p.x - px, dy = p.y - py, dz = p.z - pz;
      const float d = (dx * dx + dy * dy) + dz * dz;
      if (d <= cap) consider<1>(bd, bj, d, __float_as_int(p.w));
    }
    // d >= +0, so its bits order as it does; the keys of real candidates are distinct (cloud_nn.hip)
    const uint64_t m = wave_min_u64(((uint64_t)__float_as_uint(bd[0]) << 32) | (uint32_t)bj[0]);
    if (lane == 0) {
      const int32_t j = (int32_t)(uint32_t)m;
      match_j[pos] = j == NONE ? -1 : j;
      match_d[pos] = j == NONE ? INFINITY : __uint_as_float((uint32_t)(m >> 32));
    }
  }
}

__global__ __launch_bounds__(THREADS) void icp_scatter_kernel(const float4* __restrict__ q_sorted,
                                                              const int32_t* __restrict__ match_j,
                                                              const float* __restrict__ match_d, int32_t nq,
                                                              const int32_t* __restrict__ misc, int64_t* __restrict__ index,
                                                              float* __restrict__ dist2) {
  if (misc[M_FLAG]) return;
  const int64_t s = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (s >= nq) return;
  const int64_t i = __float_as_int(q_sorted[s].w);
  if (index) index[i] = (int64_t)match_j[s];
  if (dist2) dist2[i] = match_d[s];
}

struct IcpWorkspace {
  SupportGrid g;          // over ref
  float* T;               // 12: T_t
  double* prev;           // fitness and rmse of round t - 1
  uint64_t* keys_in;      // nq
  uint64_t* keys_out;     // nq
  int32_t* order;         // nq: source indices, ascending (cell under T_0, i)
  void* sort_temp;
  size_t sort_bytes;
  float4* q_sorted;       // nq
  int32_t* match_j;       // nq, by position in q_sorted
  float* match_d;         // nq
  int32_t* list;          // nq
  double* partial;        // (rows, nsum)
  int32_t rows;
  size_t zero_bytes;      // from g.count: counts, cursors and misc
  size_t bytes;
};

IcpWorkspace carve_icp(void* ws, int64_t nq, int64_t ns, int nsum) {
  const int D = cloud_grid_dim(ns);
  const size_t cells = (size_t)D * D * D;
  Carver c(ws);
  IcpWorkspace w;
  w.g.B = c.take<float>(3 * DMAX);
  w.g.count = c.take<int32_t>(2 * cells + 1 + MISC);
  w.g.cursor = w.g.count + cells + 1;
  w.g.misc = w.g.cursor + cells;
  w.zero_bytes = (2 * cells + 1 + MISC) * sizeof(int32_t);
  w.g.scan_ws = c.take<int32_t>(scan_ws_ints((int64_t)cells + 1));
  w.g.cell = c.take<int32_t>((size_t)ns);
  w.g.sorted = c.take<float4>((size_t)ns);
  w.T = c.take<float>(12);
  w.prev = c.take<double>(2);
  w.keys_in = c.take<uint64_t>((size_t)nq);
  w.keys_out = c.take<uint64_t>((size_t)nq);
  w.order = c.take<int32_t>((size_t)nq);
  w.sort_bytes = sort_pairs_temp_bytes(nq);
  w.sort_temp = c.take<char>(w.sort_bytes);
  w.q_sorted = c.take<float4>((size_t)nq);
  w.match_j = c.take<int32_t>((size_t)nq);
  w.match_d = c.take<float>((size_t)nq);
  w.list = c.take<int32_t>((size_t)nq);
  w.rows = (int32_t)((nq + SUM_CHUNK - 1) / SUM_CHUNK);
  w.partial = c.take<double>((size_t)w.rows * nsum);
  w.bytes = c.used();
  return w;
}

bool icp_shape_ok(int64_t nq, int64_t ns, int max_iterations) {
  return nq >= 0 && nq < (1ll << 31) && ns >= 1 && ns < (1ll << 31) && max_iterations >= 0 &&
         max_iterations <= GR_CLOUD_ICP_MAX_ITERATIONS;
}

}  // namespace
}  // namespace gr
