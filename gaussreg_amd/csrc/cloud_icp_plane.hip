// Point-to-plane ICP (include/gaussreg_hip_icp_plane.h): the loop of cloud_icp.hip with another update.  The
// grid over ref, the order of the source, the match, its fallback and the scatter are the kernels of cloud_icp_shared.hpp,
// launched exactly as there; this file adds
//
//   icpp_normals_kernel   one thread per reference normal: raises bit 1 of the finiteness flag for a non-finite component
//   icpp_sums_kernel      workgroup b reads positions [b SUM_CHUNK, (b + 1) SUM_CHUNK) of the ordered source: p = T_t src by
//                         the `apply` of the match (the same bits), q = ref[j], v = ref_normals[j]; in fp64 r = (p - q) . v,
//                         a = [p x v, v]; n, S = sum d, the 21 distinct entries of sum a a^T and the 6 of sum a r -> one row
//                         of 29 partial sums, in the order and through the tree of icp_sums_kernel
//   icpp_fold_kernel      ONE workgroup folds the rows as icp_fold_kernel does; thread 0 records history[t], applies the stop
//                         rule, refuses n < 6, solves the 6x6 system by a cyclic Jacobi eigen-decomposition whose matrices
//                         live in LDS (run-time row and column indices, so not in registers), refuses l_min <= 1e-12 l_max,
//                         forms dR = Rz Ry Rx, composes with double(T_t) and stores T_(t+1) rounded once
// The host side enqueues max_iterations + 1 rounds blindly and makes the call's one read-back, as cloud_icp.hip does.
#include <cmath>

#include "../../include/gaussreg_hip_icp_plane.h"
#include "cloud_icp_shared.hpp"

namespace gr {
namespace {

constexpr int NSUMP = 29;  // n, S, H (21: the upper triangle row by row), g (6)
constexpr int P_H = 2, P_G = 23;
constexpr int PLANE_SWEEPS = 32;
constexpr int FLAG_NORMALS = 2;

__global__ __launch_bounds__(THREADS) void icpp_normals_kernel(const float* __restrict__ normals, int64_t count,
                                                               int32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (i >= count) return;
  if (!isfinite(normals[i])) atomicOr(flag, FLAG_NORMALS);
}

// v[NSUMP] of every thread -> out[NSUMP]: the DPP wave sum, then the wave totals in wave order
__device__ __forceinline__ void block_sum_plane(double (&v)[NSUMP], double* __restrict__ red, double* __restrict__ out) {
  const int wave = threadIdx.x / WAVE;
#pragma unroll
  for (int k = 0; k < NSUMP; ++k) {
    const double w = wave_sum_f64_dpp(v[k]);
    if ((threadIdx.x & (WAVE - 1)) == 0) red[wave * NSUMP + k] = w;
  }
  __syncthreads();
  if (threadIdx.x < NSUMP) {
    double a = red[threadIdx.x];
    for (int w = 1; w < THREADS / WAVE; ++w) a += red[w * NSUMP + threadIdx.x];
    out[threadIdx.x] = a;
  }
}

__global__ __launch_bounds__(THREADS) void icpp_sums_kernel(const float4* __restrict__ q_sorted, const float* __restrict__ ref,
                                                            const float* __restrict__ ref_normals,
                                                            const int32_t* __restrict__ match_j,
                                                            const float* __restrict__ match_d, int32_t nq,
                                                            const int32_t* __restrict__ misc, const float* __restrict__ T,
                                                            double* __restrict__ partial) {
  __shared__ double red[(THREADS / WAVE) * NSUMP];
  if (misc[M_FLAG] | misc[M_DONE]) return;
  double v[NSUMP];
#pragma unroll
  for (int k = 0; k < NSUMP; ++k) v[k] = 0.0;
  const int64_t base = (int64_t)blockIdx.x * SUM_CHUNK + threadIdx.x;
  for (int it = 0; it < SUM_ITEMS; ++it) {
    const int64_t s = base + (int64_t)it * THREADS;
    if (s >= nq) break;
    const int32_t j = match_j[s];
    if (j < 0) continue;
    const float4 src = q_sorted[s];
    float fx, fy, fz;
    apply(T, src.x, src.y, src.z, fx, fy, fz);
    const double px = (double)fx, py = (double)fy, pz = (double)fz;
    const double qx = (double)ref[3 * (int64_t)j], qy = (double)ref[3 * (int64_t)j + 1], qz = (double)ref[3 * (int64_t)j + 2];
    const double nx = (double)ref_normals[3 * (int64_t)j], ny = (double)ref_normals[3 * (int64_t)j + 1],
                 nz = (double)ref_normals[3 * (int64_t)j + 2];
    const double r = ((px - qx) * nx + (py - qy) * ny) + (pz - qz) * nz;
    const double a[6] = {py * nz - pz * ny, pz * nx - px * nz, px * ny - py * nx, nx, ny, nz};
    v[0] += 1.0;
    v[1] += (double)match_d[s];
    int e = P_H;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
#pragma unroll
      for (int d = c; d < 6; ++d) v[e++] += a[c] * a[d];
      v[P_G + c] += a[c] * r;
    }
  }
  block_sum_plane(v, red, partial + (int64_t)blockIdx.x * NSUMP);
}

__global__ __launch_bounds__(THREADS) void icpp_fold_kernel(const double* __restrict__ partial, int32_t rows, int32_t nq,
                                                            int32_t* __restrict__ misc, float* __restrict__ T,
                                                            double* __restrict__ prev, int max_iterations,
                                                            double relative_fitness, double relative_rmse,
                                                            double* __restrict__ history, float* __restrict__ transform_out,
                                                            double* __restrict__ stats_out) {
  __shared__ double red[(THREADS / WAVE) * NSUMP];
  __shared__ double sum[NSUMP];
  __shared__ double Hm[36], Vm[36], ys[6], xs[6];  // thread 0's 6x6 solve: indexed at run time, so in LDS
  if (misc[M_FLAG] | misc[M_DONE]) return;
  double v[NSUMP];
#pragma unroll
  for (int k = 0; k < NSUMP; ++k) v[k] = 0.0;
  for (int32_t r = threadIdx.x; r < rows; r += THREADS) {
#pragma unroll
    for (int k = 0; k < NSUMP; ++k) v[k] += partial[(int64_t)r * NSUMP + k];
  }
  block_sum_plane(v, red, sum);
  __syncthreads();
  if (threadIdx.x != 0) return;
  const int t = misc[M_ITER];
  const double n = sum[0], S = sum[1];
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
  } else if (n < 6.0) {
    status = GR_CLOUD_ICP_DEGENERATE;
  } else {
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
    bool ok = lmin > 1e-12 * lmax;  // false for a NaN as well
    if (ok) {
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
      float Tn[12];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          double a = (dR[r * 3] * A[c] + dR[r * 3 + 1] * A[4 + c]) + dR[r * 3 + 2] * A[8 + c];
          if (c == 3) a += dt[r];
          Tn[r * 4 + c] = (float)a;
        }
      }
#pragma unroll
      for (int k = 0; k < 12; ++k) ok = ok && isfinite(Tn[k]);
      if (ok) {
#pragma unroll
        for (int k = 0; k < 12; ++k) T[k] = Tn[k];
      }
    }
    if (!ok) status = GR_CLOUD_ICP_DEGENERATE;
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

extern "C" size_t gr_cloud_icp_plane_workspace_bytes(int64_t n_src, int64_t n_ref, int max_iterations) {
  if (!icp_shape_ok(n_src, n_ref, max_iterations)) return 0;
  return carve_icp(nullptr, n_src, n_ref, NSUMP).bytes;
}

extern "C" int gr_cloud_icp_plane(const float* src, int64_t nq, const float* ref, const float* ref_normals, int64_t ns,
                                  const float* h_transform0, float max_dist2, int max_iterations, double relative_fitness,
                                  double relative_rmse, float* transform_out, double* stats_out, int64_t* index, float* dist2,
                                  double* history, int* h_status, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  GR_REQUIRE(nq >= 0 && nq < (1ll << 31), "cloud icp plane: n_src = %lld outside [0, 2^31)", (long long)nq);
  GR_REQUIRE(ns >= 1 && ns < (1ll << 31), "cloud icp plane: n_ref = %lld outside [1, 2^31)", (long long)ns);
  GR_REQUIRE(max_iterations >= 0 && max_iterations <= GR_CLOUD_ICP_MAX_ITERATIONS,
             "cloud icp plane: max_iterations = %d outside [0, %d]", max_iterations, GR_CLOUD_ICP_MAX_ITERATIONS);
  GR_REQUIRE(max_dist2 >= 0.f && std::isfinite(max_dist2), "cloud icp plane: max_dist2 = %g must be finite and >= 0",
             (double)max_dist2);
  GR_REQUIRE(!std::isnan(relative_fitness) && !std::isnan(relative_rmse), "cloud icp plane: a NaN tolerance");
  GR_REQUIRE(ref && ref_normals && (src || nq == 0) && h_transform0 && transform_out && stats_out && h_status,
             "cloud icp plane: null points, ref_normals, h_transform0, transform_out, stats_out or h_status");
  Transform0 T0;
  for (int k = 0; k < 12; ++k) {
    GR_REQUIRE(std::isfinite(h_transform0[k]), "cloud icp plane: h_transform0[%d] is not finite", k);
    T0.m[k] = h_transform0[k];
  }
  const IcpWorkspace w = carve_icp(ws, nq, ns, NSUMP);
  if (!ws || ws_bytes < w.bytes) {
    set_error("cloud icp plane: workspace of %zu bytes, %zu needed", ws_bytes, w.bytes);
    return GR_ERR_WORKSPACE;
  }
  const int D = cloud_grid_dim(ns);
  const unsigned blocks = (unsigned)((nq + THREADS - 1) / THREADS);
  if (nq == 0) {
    GR_HIP(hipMemsetAsync(w.g.misc, 0, MISC * sizeof(int32_t), stream));
  } else {
    KernelTimer timer("cloud_icp_plane_grid", stream);
    int rc = cloud_build_support_grid(ref, ns, w.g, w.g.count, w.zero_bytes, stream);
    if (rc != GR_OK) return rc;
    hipLaunchKernelGGL(icpp_normals_kernel, dim3((unsigned)((3 * ns + THREADS - 1) / THREADS)), dim3(THREADS), 0, stream,
                       ref_normals, 3 * ns, w.g.misc);
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
    KernelTimer timer("cloud_icp_plane_iterate", stream);
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
        hipLaunchKernelGGL(icpp_sums_kernel, dim3(w.rows), dim3(THREADS), 0, stream, w.q_sorted, ref, ref_normals, w.match_j,
                           w.match_d, (int32_t)nq, w.g.misc, w.T, w.partial);
      }
      hipLaunchKernelGGL(icpp_fold_kernel, dim3(1), dim3(THREADS), 0, stream, w.partial, w.rows, (int32_t)nq, w.g.misc, w.T,
                         w.prev, max_iterations, relative_fitness, relative_rmse, history, transform_out, stats_out);
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
  GR_REQUIRE((h_misc[M_FLAG] & FLAG_NORMALS) == 0, "cloud icp plane: normals must be finite");
  GR_REQUIRE(h_misc[M_FLAG] == 0, "cloud icp plane: points must be finite");
  h_status[0] = h_misc[M_STATUS];
  h_status[1] = h_misc[M_ITER];
  return GR_OK;
}
