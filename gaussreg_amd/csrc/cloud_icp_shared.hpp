// The ICP loop (DESIGN.md 3.11 point-to-point, 3.14 point-to-plane, 3.15 generalised): the fp32 transform, the kernels that
// order the source once and match it every round, the block sum, the fold kernel with the history row, the stop rule and the
// epilogue, the scatter of the reported matches, the workspace and the host driver.  cloud_icp.hip, cloud_icp_plane.hip and
// cloud_icp_gicp.hip each add an estimator -- its sums, what a matched pair adds to them and its update -- and instantiate the
// loop with it.  Everything is in the anonymous namespace, so each of the three files compiles its own copy of the kernels.
//
// An estimator E provides
//   NSUM, I_N, I_S     the number of fp64 sums of a partial row and where n and S = sum d sit among them
//   MIN_PAIRS          fewer matched pairs are GR_CLOUD_ICP_DEGENERATE
//   Args               what its kernels need beyond the loop's own arguments, passed by value
//   ARG_NAMES, args_ok the part of the null-pointer check and of its message that Args adds
//   add                device: one matched pair (the source point, j, d) into a thread's sums
//   update             thread 0 of the fold: sums, T_t -> Tn, false if there is no fit
//   after_grid         host: launches of its own behind the grid build (they may raise bits of the finiteness flag)
//   flag_text          host: the message for a raised flag
#pragma once
#include <cmath>

#include "../../include/gaussreg_hip_icp.h"
#include "cloud_grid.hpp"
#include "umeyama.hpp"

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

// v[N] of every thread -> out[N]: the DPP wave sum, then the wave totals in wave order
template <int N>
__device__ __forceinline__ void block_sum(double (&v)[N], double* __restrict__ red, double* __restrict__ out) {
  const int wave = threadIdx.x / WAVE;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const double w = wave_sum_f64_dpp(v[k]);
    if ((threadIdx.x & (WAVE - 1)) == 0) red[wave * N + k] = w;
  }
  __syncthreads();
  if (threadIdx.x < N) {
    double a = red[threadIdx.x];
    for (int w = 1; w < THREADS / WAVE; ++w) a += red[w * N + threadIdx.x];
    out[threadIdx.x] = a;
  }
}

// workgroup b: positions [b SUM_CHUNK, (b + 1) SUM_CHUNK) of the ordered source, thread t takes t, t + 256, .. of the chunk
// in order and adds each matched pair to its sums by the estimator's `add`, then the DPP wave sum and the four wave totals
// in wave order -> row b of partial.  The walk is unrolled by the pragma: left to itself the compiler unrolls it when the
// body is written out here and not when it is a call, which costs point-to-point 8 VGPRs and a wave per SIMD.
template <class E>
__global__ __launch_bounds__(THREADS) void icp_sums_kernel(const float4* __restrict__ q_sorted, const float* __restrict__ ref,
                                const int32_t* __restrict__ match_j, const float* __restrict__ match_d, int32_t nq,
                                const int32_t* __restrict__ misc, const float* __restrict__ T, typename E::Args args,
                                double* __restrict__ partial) {
  constexpr int N = E::NSUM;
  __shared__ double red[(THREADS / WAVE) * N];
  if (misc[M_FLAG] | misc[M_DONE]) return;
  double v[N];
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = 0.0;
  const int64_t base = (int64_t)blockIdx.x * SUM_CHUNK + threadIdx.x;
#pragma unroll
  for (int it = 0; it < SUM_ITEMS; ++it) {
    const int64_t s = base + (int64_t)it * THREADS;
    if (s >= nq) break;
    const int32_t j = match_j[s];
    if (j < 0) continue;
    E::add(v, q_sorted[s], j, match_d[s], ref, T, args);
  }
  block_sum(v, red, partial + (int64_t)blockIdx.x * N);
}

// ONE workgroup: thread t adds rows t, t + 256, .. in order, the tree of block_sum; thread 0 records history[t], applies the
// stop rule, runs the estimator's update and stores T_(t+1), t + 1 -- or done, the status, transform_out and stats_out
template <class E>
__global__ __launch_bounds__(THREADS) void icp_fold_kernel(const double* __restrict__ partial, int32_t rows, int32_t nq,
                                                           int32_t* __restrict__ misc, float* __restrict__ T,
                                                           double* __restrict__ prev, typename E::Args args,
                                                           int max_iterations, double relative_fitness, double relative_rmse,
                                                           double* __restrict__ history, float* __restrict__ transform_out,
                                                           double* __restrict__ stats_out) {
  constexpr int N = E::NSUM;
  __shared__ double red[(THREADS / WAVE) * N];
  __shared__ double sum[N];
  if (misc[M_FLAG] | misc[M_DONE]) return;
  double v[N];
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = 0.0;
  for (int32_t r = threadIdx.x; r < rows; r += THREADS) {
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] += partial[(int64_t)r * N + k];
  }
  block_sum(v, red, sum);
  __syncthreads();
  if (threadIdx.x != 0) return;
  const int t = misc[M_ITER];
  const double n = sum[E::I_N], S = sum[E::I_S];
  const double fitness = nq > 0 ? n / (double)nq : 0.0, rmse = n > 0.0 ? sqrt(S / n) : 0.0;
  if (history) {
    double* h = history + (int64_t)t * HISTORY_ROW;
    for (int k = 0; k < 12; ++k) h[k] = (double)T[k];
    h[12] = n;
    h[13] = S;
    h[14] = fitness;
    h[15] = rmse;
  }
  int status = 0;
  if (nq == 0) {
    status = GR_CLOUD_ICP_DEGENERATE;
  } else if (t >= 1 && fabs(fitness - prev[0]) < relative_fitness && fabs(rmse - prev[1]) < relative_rmse) {
    status = GR_CLOUD_ICP_CONVERGED;
  } else if (t == max_iterations) {
    status = GR_CLOUD_ICP_ITERATION_LIMIT;
  } else if (n < E::MIN_PAIRS) {
    status = GR_CLOUD_ICP_DEGENERATE;
  } else {
    float Tn[12];
    bool ok = E::update(sum, T, args, Tn);
    for (int k = 0; k < 12; ++k) ok = ok && isfinite(Tn[k]);
    if (ok) {
      for (int k = 0; k < 12; ++k) T[k] = Tn[k];
    } else {
      status = GR_CLOUD_ICP_DEGENERATE;
    }
  }
  if (status) {
    for (int k = 0; k < 12; ++k) transform_out[k] = T[k];
    transform_out[12] = transform_out[13] = transform_out[14] = 0.f;
    transform_out[15] = 1.f;
    stats_out[0] = fitness;
    stats_out[1] = rmse;
    stats_out[2] = n;
    stats_out[3] = S;
    misc[M_STATUS] = status;
    misc[M_DONE] = 1;
  } else {
    prev[0] = fitness;
    prev[1] = rmse;
    misc[M_LIST] = 0;  // the list of this round has been consumed
    misc[M_ITER] = t + 1;
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

template <class E>
size_t icp_workspace_bytes(int64_t nq, int64_t ns, int max_iterations) {
  const bool ok = nq >= 0 && nq < (1ll << 31) && ns >= 1 && ns < (1ll << 31) && max_iterations >= 0 &&
                  max_iterations <= GR_CLOUD_ICP_MAX_ITERATIONS;
  return ok ? carve_icp(nullptr, nq, ns, E::NSUM).bytes : 0;
}

// The host side of a call: the checks, the grid over ref and the order of the source, max_iterations + 1 rounds enqueued
// blindly -- round max_iterations always stops -- the scatter, and the call's one read-back: flag, status, iteration count.
// `name` opens every message ("cloud icp"); the two timers cover the set-up and the rounds.
template <class E>
int icp_run(const char* name, const char* grid_timer, const char* iterate_timer, const float* src, int64_t nq, const float* ref,
            int64_t ns, const float* h_transform0, float max_dist2, typename E::Args args, int max_iterations,
            double relative_fitness, double relative_rmse, float* transform_out, double* stats_out, int64_t* index,
            float* dist2, double* history, int* h_status, void* ws, size_t ws_bytes, hipStream_t stream) {
  GR_REQUIRE(nq >= 0 && nq < (1ll << 31), "%s: n_src = %lld outside [0, 2^31)", name, (long long)nq);
  GR_REQUIRE(ns >= 1 && ns < (1ll << 31), "%s: n_ref = %lld outside [1, 2^31)", name, (long long)ns);
  GR_REQUIRE(max_iterations >= 0 && max_iterations <= GR_CLOUD_ICP_MAX_ITERATIONS, "%s: max_iterations = %d outside [0, %d]",
             name, max_iterations, GR_CLOUD_ICP_MAX_ITERATIONS);
  GR_REQUIRE(max_dist2 >= 0.f && std::isfinite(max_dist2), "%s: max_dist2 = %g must be finite and >= 0", name, (double)max_dist2);
  GR_REQUIRE(!std::isnan(relative_fitness) && !std::isnan(relative_rmse), "%s: a NaN tolerance", name);
  GR_REQUIRE(ref && E::args_ok(args) && (src || nq == 0) && h_transform0 && transform_out && stats_out && h_status,
             "%s: null points, %sh_transform0, transform_out, stats_out or h_status", name, E::ARG_NAMES);
  Transform0 T0;
  for (int k = 0; k < 12; ++k) {
    GR_REQUIRE(std::isfinite(h_transform0[k]), "%s: h_transform0[%d] is not finite", name, k);
    T0.m[k] = h_transform0[k];
  }
  const IcpWorkspace w = carve_icp(ws, nq, ns, E::NSUM);
  if (!ws || ws_bytes < w.bytes) {
    set_error("%s: workspace of %zu bytes, %zu needed", name, ws_bytes, w.bytes);
    return GR_ERR_WORKSPACE;
  }
  const int D = cloud_grid_dim(ns);
  const unsigned blocks = (unsigned)((nq + THREADS - 1) / THREADS);
  if (nq == 0) {
    GR_HIP(hipMemsetAsync(w.g.misc, 0, MISC * sizeof(int32_t), stream));
  } else {
    KernelTimer timer(grid_timer, stream);
    int rc = cloud_build_support_grid(ref, ns, w.g, w.g.count, w.zero_bytes, stream);
    if (rc != GR_OK) return rc;
    E::after_grid(args, ns, w.g.misc, stream);
    hipLaunchKernelGGL(icp_key_kernel, dim3(blocks), dim3(THREADS), 0, stream, src, nq, T0, D, w.g.B, w.keys_in, w.g.misc);
    GR_LAUNCH_CHECK();
    int bits = 1;
    while ((1ll << bits) < (int64_t)D * D * D) ++bits;
    rc = sort_pairs_u64_iota(w.sort_temp, w.sort_bytes, w.keys_in, w.keys_out, nq, w.order, nq, 0, bits, stream);
    if (rc != GR_OK) return rc;
    hipLaunchKernelGGL(icp_gather_kernel, dim3(blocks), dim3(THREADS), 0, stream, src, w.order, nq, w.q_sorted);
    GR_LAUNCH_CHECK();
  }
  {
    KernelTimer timer(iterate_timer, stream);
    hipLaunchKernelGGL(icp_init_kernel, dim3(1), dim3(WAVE), 0, stream, T0, w.T);
    GR_LAUNCH_CHECK();
    const unsigned qblocks = (unsigned)((nq + QUERY_THREADS - 1) / QUERY_THREADS);
    const int64_t waves = (nq + (THREADS / WAVE) - 1) / (THREADS / WAVE);
    const unsigned fblocks = (unsigned)(waves < FALLBACK_BLOCKS ? waves : FALLBACK_BLOCKS);
    for (int round = 0; round <= (nq == 0 ? 0 : max_iterations); ++round) {
      if (nq > 0) {
        hipLaunchKernelGGL(icp_match_kernel, dim3(qblocks), dim3(QUERY_THREADS), 0, stream, w.g.sorted, w.g.count, w.q_sorted,
                           w.g.B, w.g.misc, w.T, (int32_t)nq, D, max_dist2, w.match_j, w.match_d, w.list);
        hipLaunchKernelGGL(icp_fallback_kernel, dim3(fblocks), dim3(THREADS), 0, stream, w.g.sorted, (int32_t)ns, w.q_sorted,
                           w.list, w.g.misc, w.T, max_dist2, w.match_j, w.match_d);
        hipLaunchKernelGGL(icp_sums_kernel<E>, dim3(w.rows), dim3(THREADS), 0, stream, w.q_sorted, ref, w.match_j, w.match_d,
                           (int32_t)nq, w.g.misc, w.T, args, w.partial);
      }
      hipLaunchKernelGGL(icp_fold_kernel<E>, dim3(1), dim3(THREADS), 0, stream, w.partial, w.rows, (int32_t)nq, w.g.misc, w.T,
                         w.prev, args, max_iterations, relative_fitness, relative_rmse, history, transform_out, stats_out);
      GR_LAUNCH_CHECK();
    }
    if (nq > 0 && (index || dist2)) {
      hipLaunchKernelGGL(icp_scatter_kernel, dim3(blocks), dim3(THREADS), 0, stream, w.q_sorted, w.match_j, w.match_d, (int32_t)nq,
                         w.g.misc, index, dist2);
      GR_LAUNCH_CHECK();
    }
  }
  int32_t h_misc[MISC];
  GR_HIP(hipMemcpyAsync(h_misc, w.g.misc, sizeof h_misc, hipMemcpyDeviceToHost, stream));
  GR_HIP(hipStreamSynchronize(stream));
  GR_REQUIRE(h_misc[M_FLAG] == 0, "%s: %s", name, E::flag_text(h_misc[M_FLAG]));
  h_status[0] = h_misc[M_STATUS];
  h_status[1] = h_misc[M_ITER];
  return GR_OK;
}

}  // namespace
}  // namespace gr
