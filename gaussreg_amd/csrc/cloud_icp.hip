// Point-to-point ICP (include/gaussreg_hip_icp.h): the loop  match -> fp64 sums -> Umeyama -> stop test
// without leaving the device.  The support grid of cloud_nn.hip (cloud_grid.hpp) is built ONCE over ref; the source points
// are put ONCE into the order ascending (cell of p_i under T_0, i) by the stable radix sort of sort.hip -- not by the
// atomic-cursor scatter, whose order inside a cell varies between runs: the sums below are taken in this order, so it has
// to be the same in every call.
//
//   icp_init_kernel       T <- T_0
//   icp_key_kernel        one thread per source point: finiteness flag, key = cell of the point under T_0
//   (sort_pairs_u64_iota: stable, so equal cells keep ascending i)
//   icp_gather_kernel     (x, y, z, i) of the source into that order
//   per round t = 0 .. max_iterations, every kernel starting with a uniform "flag raised or done: return":
//   icp_match_kernel      one thread per ordered source point: p = T_t src, its cell by binary search of the boundaries,
//                         the CAP = 1 shell search with the face and box bound -> match_j / match_d at its position; a
//                         query no rule stops within MAX_SHELLS shells is appended to the list
//   icp_fallback_kernel   one WAVE per listed query scans the whole support, writes the same two arrays
//   icp_sums_kernel       workgroup b reads positions [b SUM_CHUNK, (b + 1) SUM_CHUNK): n, sum src, sum ref, sum src_a ref_b,
//                         sum |src|^2 and S = sum d in fp64, thread t takes positions t, t + 256, .. of the chunk in
//                         order, then the DPP wave sum and the four wave totals in wave order -> one partial row
//   icp_fold_kernel       ONE workgroup: thread t adds rows t, t + 256, .. in order, same tree; thread 0 records history[t],
//                         applies the stop rule, runs umeyama_from_sums and stores T_(t+1), t + 1 -- or done, the status,
//                         transform_out and stats_out
//   icp_scatter_kernel    match_j / match_d of the reported evaluation back into the caller's source order
// The host enqueues max_iterations + 1 rounds blindly -- round max_iterations always stops -- and then makes the call's one
// read-back: flag, status, iteration count.
//
// Reproducibility: the order of the source, the chunking, the trees and the fold depend on the shapes alone; a listed
// query's match lands at its own position whatever the order of the list; only integer atomics are used.
#include <cmath>

#include "../../include/gaussreg_hip_icp.h"
#include "cloud_grid.hpp"
#include "umeyama.hpp"

namespace gr {
namespace {

constexpr int SUM_ITEMS = 8;
constexpr int SUM_CHUNK = THREADS * SUM_ITEMS;  // ordered source points per partial row
constexpr int NSUM = 18;  // n, sum src (3), sum ref (3), sum src_a ref_b (9), sum |src|^2, S
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

// v[NSUM] of every thread -> out[NSUM]: the DPP wave sum, then the wave totals in wave order
__device__ __forceinline__ void block_sum(double (&v)[NSUM], double* __restrict__ red, double* __restrict__ out) {
  const int wave = threadIdx.x / WAVE;
#pragma unroll
  for (int k = 0; k < NSUM; ++k) {
    const double w = wave_sum_f64_dpp(v[k]);
    if ((threadIdx.x & (WAVE - 1)) == 0) red[wave * NSUM + k] = w;
  }
  __syncthreads();
  if (threadIdx.x < NSUM) {
    double a = red[threadIdx.x];
    for (int w = 1; w < THREADS / WAVE; ++w) a += red[w * NSUM + threadIdx.x];
    out[threadIdx.x] = a;
  }
}

__global__ __launch_bounds__(THREADS) void icp_sums_kernel(const float4* __restrict__ q_sorted, const float* __restrict__ ref,
                                                           const int32_t* __restrict__ match_j,
                                                           const float* __restrict__ match_d, int32_t nq,
                                                           const int32_t* __restrict__ misc, double* __restrict__ partial) {
  __shared__ double red[(THREADS / WAVE) * NSUM];
  if (misc[M_FLAG] | misc[M_DONE]) return;
  double v[NSUM];
#pragma unroll
  for (int k = 0; k < NSUM; ++k) v[k] = 0.0;
  const int64_t base = (int64_t)blockIdx.x * SUM_CHUNK + threadIdx.x;
  for (int it = 0; it < SUM_ITEMS; ++it) {
    const int64_t s = base + (int64_t)it * THREADS;
    if (s >= nq) break;
    const int32_t j = match_j[s];
    if (j < 0) continue;
    const float4 q = q_sorted[s];
    const double a[3] = {(double)q.x, (double)q.y, (double)q.z};
    const double r[3] = {(double)ref[3 * (int64_t)j], (double)ref[3 * (int64_t)j + 1], (double)ref[3 * (int64_t)j + 2]};
    v[0] += 1.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      v[1 + c] += a[c];
      v[4 + c] += r[c];
#pragma unroll
      for (int e = 0; e < 3; ++e) v[7 + c * 3 + e] += a[c] * r[e];
    }
    v[16] += (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
    v[17] += (double)match_d[s];
  }
  block_sum(v, red, partial + (int64_t)blockIdx.x * NSUM);
}

__global__ __launch_bounds__(THREADS) void icp_fold_kernel(const double* __restrict__ partial, int32_t rows, int32_t nq,
                                                           int32_t* __restrict__ misc, float* __restrict__ T,
                                                           double* __restrict__ prev, int with_scale, int max_iterations,
                                                           double relative_fitness, double relative_rmse,
                                                           double* __restrict__ history, float* __restrict__ transform_out,
                                                           double* __restrict__ stats_out) {
  __shared__ double red[(THREADS / WAVE) * NSUM];
  __shared__ double sum[NSUM];
  if (misc[M_FLAG] | misc[M_DONE]) return;
  double v[NSUM];
#pragma unroll
  for (int k = 0; k < NSUM; ++k) v[k] = 0.0;
  for (int32_t r = threadIdx.x; r < rows; r += THREADS) {
#pragma unroll
    for (int k = 0; k < NSUM; ++k) v[k] += partial[(int64_t)r * NSUM + k];
  }
  block_sum(v, red, sum);
  __syncthreads();
  if (threadIdx.x != 0) return;
  const int t = misc[M_ITER];
  const double n = sum[0], S = sum[17];
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
  } else if (n < 3.0) {
    status = GR_CLOUD_ICP_DEGENERATE;
  } else {
    float Tn[12];
    bool ok = umeyama_from_sums(n, sum + 1, sum + 4, sum + 7, sum[16], with_scale, Tn);
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
  double* partial;        // (rows, NSUM)
  int32_t rows;
  size_t zero_bytes;      // from g.count: counts, cursors and misc
  size_t bytes;
};

IcpWorkspace carve_icp(void* ws, int64_t nq, int64_t ns) {
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
  w.partial = c.take<double>((size_t)w.rows * NSUM);
  w.bytes = c.used();
  return w;
}

bool icp_shape_ok(int64_t nq, int64_t ns, int max_iterations) {
  return nq >= 0 && nq < (1ll << 31) && ns >= 1 && ns < (1ll << 31) && max_iterations >= 0 &&
         max_iterations <= GR_CLOUD_ICP_MAX_ITERATIONS;
}

}  // namespace
}  // namespace gr

using namespace gr;

extern "C" size_t gr_cloud_icp_workspace_bytes(int64_t n_src, int64_t n_ref, int max_iterations) {
  if (!icp_shape_ok(n_src, n_ref, max_iterations)) return 0;
  return carve_icp(nullptr, n_src, n_ref).bytes;
}

extern "C" int gr_cloud_icp(const float* src, int64_t nq, const float* ref, int64_t ns, const float* h_transform0,
                            float max_dist2, int with_scale, int max_iterations, double relative_fitness,
                            double relative_rmse, float* transform_out, double* stats_out, int64_t* index, float* dist2,
                            double* history, int* h_status, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  GR_REQUIRE(nq >= 0 && nq < (1ll << 31), "cloud icp: n_src = %lld outside [0, 2^31)", (long long)nq);
  GR_REQUIRE(ns >= 1 && ns < (1ll << 31), "cloud icp: n_ref = %lld outside [1, 2^31)", (long long)ns);
  GR_REQUIRE(max_iterations >= 0 && max_iterations <= GR_CLOUD_ICP_MAX_ITERATIONS, "cloud icp: max_iterations = %d outside [0, %d]",
             max_iterations, GR_CLOUD_ICP_MAX_ITERATIONS);
  GR_REQUIRE(max_dist2 >= 0.f && std::isfinite(max_dist2), "cloud icp: max_dist2 = %g must be finite and >= 0", (double)max_dist2);
  GR_REQUIRE(!std::isnan(relative_fitness) && !std::isnan(relative_rmse), "cloud icp: a NaN tolerance");
  GR_REQUIRE(ref && (src || nq == 0) && h_transform0 && transform_out && stats_out && h_status,
             "cloud icp: null points, h_transform0, transform_out, stats_out or h_status");
  Transform0 T0;
  for (int k = 0; k < 12; ++k) {
    GR_REQUIRE(std::isfinite(h_transform0[k]), "cloud icp: h_transform0[%d] is not finite", k);
    T0.m[k] = h_transform0[k];
  }
  const IcpWorkspace w = carve_icp(ws, nq, ns);
  if (!ws || ws_bytes < w.bytes) {
    set_error("cloud icp: workspace of %zu bytes, %zu needed", ws_bytes, w.bytes);
    return GR_ERR_WORKSPACE;
  }
  const int D = cloud_grid_dim(ns);
  const unsigned blocks = (unsigned)((nq + THREADS - 1) / THREADS);
  if (nq == 0) {
    GR_HIP(hipMemsetAsync(w.g.misc, 0, MISC * sizeof(int32_t), stream));
  } else {
    KernelTimer timer("cloud_icp_grid", stream);
    int rc = cloud_build_support_grid(ref, ns, w.g, w.g.count, w.zero_bytes, stream);
    if (rc != GR_OK) return rc;
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
    KernelTimer timer("cloud_icp_iterate", stream);
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
        hipLaunchKernelGGL(icp_sums_kernel, dim3(w.rows), dim3(THREADS), 0, stream, w.q_sorted, ref, w.match_j, w.match_d,
                           (int32_t)nq, w.g.misc, w.partial);
      }
      hipLaunchKernelGGL(icp_fold_kernel, dim3(1), dim3(THREADS), 0, stream, w.partial, w.rows, (int32_t)nq, w.g.misc, w.T, w.prev,
                         with_scale, max_iterations, relative_fitness, relative_rmse, history, transform_out, stats_out);
      GR_LAUNCH_CHECK();
    }
    if (nq > 0 && (index || dist2)) {
      hipLaunchKernelGGL(icp_scatter_kernel, dim3(blocks), dim3(THREADS), 0, stream, w.q_sorted, w.match_j, w.match_d, (int32_t)nq,
                         w.g.misc, index, dist2);
      GR_LAUNCH_CHECK();
    }
  }
  // the one host read-back of a call: flag, status, iteration count
  int32_t h_misc[MISC];
  GR_HIP(hipMemcpyAsync(h_misc, w.g.misc, sizeof h_misc, hipMemcpyDeviceToHost, stream));
  GR_HIP(hipStreamSynchronize(stream));
  GR_REQUIRE(h_misc[M_FLAG] == 0, "cloud icp: points must be finite");
  h_status[0] = h_misc[M_STATUS];
  h_status[1] = h_misc[M_ITER];
  return GR_OK;
}
