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
// Everything but the sums and the fold -- `apply`, the init, key, gather, match, fallback and scatter kernels, the workspace --
// lives in cloud_icp_shared.hpp, which cloud_icp_plane.hip (point-to-plane) includes as well.
//
// Reproducibility: the order of the source, the chunking, the trees and the fold depend on the shapes alone; a listed
// query's match lands at its own position whatever the order of the list; only integer atomics are used.
#include "cloud_icp_shared.hpp"
#include "umeyama.hpp"

namespace gr {
namespace {

constexpr int NSUM = 18;  // n, sum src (3), sum ref (3), sum src_a ref_b (9), sum |src|^2, S

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


}  // namespace
}  // namespace gr

using namespace gr;

extern "C" size_t gr_cloud_icp_workspace_bytes(int64_t n_src, int64_t n_ref, int max_iterations) {
  if (!icp_shape_ok(n_src, n_ref, max_iterations)) return 0;
  return carve_icp(nullptr, n_src, n_ref, NSUM).bytes;
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
  const IcpWorkspace w = carve_icp(ws, nq, ns, NSUM);
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
