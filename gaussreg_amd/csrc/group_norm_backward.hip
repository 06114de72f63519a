// Backward of the GroupNorm (+ residual, LeakyReLU) of kpconv.hip over a (N, C) point-feature matrix: the gradients torch's
// GroupNorm / add / leaky_relu backward give after two transposes, with the matrix left (N, C) and read with float4 loads in
// the forward's thread-to-column mapping (include/gaussreg_hip_train_backbone.h has the math).
//   pass 1  (bwd_sums)   streams x, out, grad_out once: per workgroup and column the fp64 sums of dy and dy * xhat, one slot
//                        per (segment, workgroup) -- no atomics; dy goes to grad_residual on the way when that is wanted
//   fold 1  (bwd_fold)   adds the workgroups of a segment up per column: 16 interleaved chains (workgroup b in chain
//                        b % 16, ascending inside a chain), the chains joined in ascending order
//   fold 2  (bwd_finish) grad_gamma / grad_beta: the segments' column totals in ascending segment order; A / cnt, B / cnt per
//                        (segment, group): the group's channels in four interleaved ascending chains
//   pass 2  (bwd_apply)  streams again and writes grad_x
// Every sum is fp64, as the forward's statistics are: the partials of one column differ by many orders of magnitude between
// workgroups when a segment is short, and fp64 adds cost nothing next to the 28 - 32 bytes per element the passes move.
#include <algorithm>

#include "../../include/gaussreg_hip_train_backbone.h"
#include "common.hpp"

namespace gr {
namespace {

constexpr int GNB_T = 256;     // = the forward's GN_T: the column mapping below is the forward's
constexpr int GNB_MAXG = 64;
constexpr int GNB_FOLD_CH = 16;  // fold 1: channels per workgroup, x 16 chains

__host__ __device__ inline int gnb_block_cap(int64_t c, int64_t nseg) {
  int64_t cap = 131072 / c;  // 16 * cap * c bytes of partials per segment: 2 MB at most, whatever c
  cap = cap < 32 ? 32 : (cap > 1024 ? 1024 : cap);
  const int64_t per_seg = nseg > 2048 ? 1 : 2048 / (nseg > 0 ? nseg : 1);
  return (int)(cap < per_seg ? cap : per_seg);
}

__device__ __forceinline__ float4 gnb_dy(const float4 g, const float4 o, float slope) {
  return make_float4(o.x > 0.f ? g.x : g.x * slope, o.y > 0.f ? g.y : g.y * slope, o.z > 0.f ? g.z : g.z * slope,
                     o.w > 0.f ? g.w : g.w * slope);
}

// partial: [segment][workgroup][2][C] doubles.  STORE_DY: dy is written to dy_out (the grad_residual buffer).
template <bool STORE_DY>
__global__ __launch_bounds__(GNB_T) void group_norm_bwd_sums_kernel(const float* __restrict__ x, const float* __restrict__ out,
                                                                    const float* __restrict__ grad_out,
                                                                    const float* __restrict__ stats, int64_t n, int c, int groups,
                                                                    float slope, int act, double* __restrict__ partial,
                                                                    const int64_t* __restrict__ seg_off,
                                                                    float* __restrict__ dy_out) {
  __shared__ double s_red[8][GNB_T];  // [moment * 4 + j][thread]
  __shared__ float s_mean[GNB_MAXG], s_rstd[GNB_MAXG];
  if (seg_off != nullptr) {
    const int64_t r0 = seg_off[blockIdx.y];
    n = seg_off[blockIdx.y + 1] - r0;
    x += r0 * c;
    grad_out += r0 * c;
    if (act) out += r0 * c;
    if (STORE_DY) dy_out += r0 * c;
  }
  stats += (int64_t)blockIdx.y * 2 * groups;
  partial += ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 2 * c;
  const int cols4 = c / 4, cg = c / groups;
  const int tid = threadIdx.x;
  const int npos = cols4 > GNB_T ? cols4 / GNB_T : 1;
  const int rows_per_pass = cols4 >= GNB_T ? 1 : GNB_T / cols4;
  const int col_base = cols4 >= GNB_T ? tid : tid % cols4;
  const int rsub = cols4 >= GNB_T ? 0 : tid / cols4;
  if (tid < groups) {
    s_mean[tid] = stats[tid];
    s_rstd[tid] = stats[groups + tid];
  }
  __syncthreads();
  for (int p = 0; p < npos; ++p) {
    const int ch = 4 * (col_base + p * GNB_T);
    float mean[4], rstd[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      mean[j] = s_mean[(ch + j) / cg];
      rstd[j] = s_rstd[(ch + j) / cg];
    }
    double sd[4] = {0, 0, 0, 0}, sx[4] = {0, 0, 0, 0};
    for (int64_t r = (int64_t)blockIdx.x * rows_per_pass + rsub; r < n; r += (int64_t)gridDim.x * rows_per_pass) {
      const int64_t at = r * c + ch;
      const float4 v = *reinterpret_cast<const float4*>(x + at);
      float4 dy = *reinterpret_cast<const float4*>(grad_out + at);
      if (act) dy = gnb_dy(dy, *reinterpret_cast<const float4*>(out + at), slope);
      if (STORE_DY) *reinterpret_cast<float4*>(dy_out + at) = dy;
      sd[0] += dy.x, sd[1] += dy.y, sd[2] += dy.z, sd[3] += dy.w;
      sx[0] += (double)dy.x * (double)((v.x - mean[0]) * rstd[0]);
      sx[1] += (double)dy.y * (double)((v.y - mean[1]) * rstd[1]);
      sx[2] += (double)dy.z * (double)((v.z - mean[2]) * rstd[2]);
      sx[3] += (double)dy.w * (double)((v.w - mean[3]) * rstd[3]);
    }
    if (rows_per_pass > 1) {  // (npos == 1 here) the row slots of a column, added in ascending order by its first thread
#pragma unroll
      for (int j = 0; j < 4; ++j) s_red[j][tid] = sd[j], s_red[4 + j][tid] = sx[j];
      __syncthreads();
      if (rsub == 0) {
        for (int rs = 1; rs < rows_per_pass; ++rs) {
#pragma unroll
          for (int j = 0; j < 4; ++j) sd[j] += s_red[j][tid + rs * cols4], sx[j] += s_red[4 + j][tid + rs * cols4];
        }
      }
    }
    if (rsub == 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j) partial[ch + j] = sd[j], partial[c + ch + j] = sx[j];
    }
  }
}

// grid (ceil(C / 16), nseg): tot[segment][2][C] = the segment's partials added over its workgroups
__global__ __launch_bounds__(GNB_T) void group_norm_bwd_fold_kernel(const double* __restrict__ partial, int nblk, int c,
                                                                    double* __restrict__ tot) {
  __shared__ double s_red[2][GNB_T];
  const int tid = threadIdx.x, chl = tid % GNB_FOLD_CH, sub = tid / GNB_FOLD_CH;
  const int ch = blockIdx.x * GNB_FOLD_CH + chl;
  partial += (int64_t)blockIdx.y * nblk * 2 * c;
  double a0 = 0.0, a1 = 0.0;
  if (ch < c)
    for (int b = sub; b < nblk; b += GNB_T / GNB_FOLD_CH) {
      a0 += partial[(int64_t)b * 2 * c + ch];
      a1 += partial[(int64_t)b * 2 * c + c + ch];
    }
  s_red[0][tid] = a0, s_red[1][tid] = a1;
  __syncthreads();
  if (sub == 0 && ch < c) {
    for (int s = 1; s < GNB_T / GNB_FOLD_CH; ++s) a0 += s_red[0][s * GNB_FOLD_CH + chl], a1 += s_red[1][s * GNB_FOLD_CH + chl];
    tot[(int64_t)blockIdx.y * 2 * c + ch] = a0;
    tot[(int64_t)blockIdx.y * 2 * c + c + ch] = a1;
  }
}

// workgroups [0, nb_param): grad_beta / grad_gamma, a thread per channel; the others: ab[segment][0][g] = A / cnt,
// ab[segment][1][g] = B / cnt, four lanes per (segment, group)
__global__ __launch_bounds__(GNB_T) void group_norm_bwd_finish_kernel(const double* __restrict__ tot, const float* __restrict__ gamma,
                                                                      int64_t n, int c, int groups, int nseg, int nb_param,
                                                                      const int64_t* __restrict__ seg_off,
                                                                      float* __restrict__ grad_gamma, float* __restrict__ grad_beta,
                                                                      float* __restrict__ ab) {
  const int tid = threadIdx.x;
  if ((int)blockIdx.x < nb_param) {
    const int ch = blockIdx.x * GNB_T + tid;
    if (ch >= c) return;
    double gb = 0.0, gg = 0.0;
    for (int s = 0; s < nseg; ++s) {
      gb += tot[(int64_t)s * 2 * c + ch];
      gg += tot[(int64_t)s * 2 * c + c + ch];
    }
    if (grad_beta) grad_beta[ch] = (float)gb;
    if (grad_gamma) grad_gamma[ch] = (float)gg;
    return;
  }
  const int item = ((int)blockIdx.x - nb_param) * (GNB_T / 4) + tid / 4, sub = tid % 4;
  const bool live = item < nseg * groups;  // every lane stays for the shuffles
  const int s = live ? item / groups : 0, g = live ? item % groups : 0, cg = c / groups;
  double A = 0.0, B = 0.0;
  if (live)
    for (int k = sub; k < cg; k += 4) {
      const int ch = g * cg + k;
      const double ga = gamma ? (double)gamma[ch] : 1.0;
      B += ga * tot[(int64_t)s * 2 * c + ch];
      A += ga * tot[(int64_t)s * 2 * c + c + ch];
    }
  A += __shfl_xor(A, 1, WAVE), B += __shfl_xor(B, 1, WAVE);
  A += __shfl_xor(A, 2, WAVE), B += __shfl_xor(B, 2, WAVE);
  if (live && sub == 0) {
    const int64_t rows = seg_off ? seg_off[s + 1] - seg_off[s] : n;
    const double cnt = fmax((double)rows * (double)cg, 1.0);
    ab[(int64_t)s * 2 * groups + g] = (float)(A / cnt);
    ab[(int64_t)s * 2 * groups + groups + g] = (float)(B / cnt);
  }
}

// FROM_DY: dy is read back from the grad_residual buffer pass 1 filled (8 bytes per element instead of 12)
template <bool FROM_DY>
__global__ __launch_bounds__(GNB_T) void group_norm_bwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ out,
                                                                     const float* __restrict__ grad_out,
                                                                     const float* __restrict__ gamma, const float* __restrict__ stats,
                                                                     const float* __restrict__ ab, int64_t n, int c, int groups,
                                                                     float slope, int act, const int64_t* __restrict__ seg_off,
                                                                     float* __restrict__ grad_x) {
  __shared__ float s_mean[GNB_MAXG], s_rstd[GNB_MAXG], s_a[GNB_MAXG], s_b[GNB_MAXG];
  if (seg_off != nullptr) {
    const int64_t r0 = seg_off[blockIdx.y];
    n = seg_off[blockIdx.y + 1] - r0;
    x += r0 * c;
    grad_out += r0 * c;  // FROM_DY: the dy buffer
    if (!FROM_DY && act) out += r0 * c;
    grad_x += r0 * c;
  }
  stats += (int64_t)blockIdx.y * 2 * groups;
  ab += (int64_t)blockIdx.y * 2 * groups;
  const int cols4 = c / 4, cg = c / groups;
  const int tid = threadIdx.x;
  const int npos = cols4 > GNB_T ? cols4 / GNB_T : 1;
  const int rows_per_pass = cols4 >= GNB_T ? 1 : GNB_T / cols4;
  const int col_base = cols4 >= GNB_T ? tid : tid % cols4;
  const int rsub = cols4 >= GNB_T ? 0 : tid / cols4;
  if (tid < groups) {
    s_mean[tid] = stats[tid];
    s_rstd[tid] = stats[groups + tid];
    s_a[tid] = ab[tid];
    s_b[tid] = ab[groups + tid];
  }
  __syncthreads();
  for (int p = 0; p < npos; ++p) {
    const int ch = 4 * (col_base + p * GNB_T);
    float mean[4], rstd[4], ca[4], cb[4];
    float4 ga = make_float4(1.f, 1.f, 1.f, 1.f);
    if (gamma) ga = *reinterpret_cast<const float4*>(gamma + ch);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int g = (ch + j) / cg;
      mean[j] = s_mean[g], rstd[j] = s_rstd[g], ca[j] = s_a[g], cb[j] = s_b[g];
    }
    for (int64_t r = (int64_t)blockIdx.x * rows_per_pass + rsub; r < n; r += (int64_t)gridDim.x * rows_per_pass) {
      const int64_t at = r * c + ch;
      const float4 v = *reinterpret_cast<const float4*>(x + at);
      float4 dy = *reinterpret_cast<const float4*>(grad_out + at);
      if (!FROM_DY && act) dy = gnb_dy(dy, *reinterpret_cast<const float4*>(out + at), slope);
      float4 gx;
      gx.x = rstd[0] * (dy.x * ga.x - (cb[0] + (v.x - mean[0]) * rstd[0] * ca[0]));
      gx.y = rstd[1] * (dy.y * ga.y - (cb[1] + (v.y - mean[1]) * rstd[1] * ca[1]));
      gx.z = rstd[2] * (dy.z * ga.z - (cb[2] + (v.z - mean[2]) * rstd[2] * ca[2]));
      gx.w = rstd[3] * (dy.w * ga.w - (cb[3] + (v.w - mean[3]) * rstd[3] * ca[3]));
      *reinterpret_cast<float4*>(grad_x + at) = gx;
    }
  }
}

bool gnb_shape_ok(int64_t c, int64_t groups, int64_t nseg) {
  if (c < 4 || c % 4 != 0 || c > (1 << 20) || groups < 1 || groups > GNB_MAXG || c % groups != 0) return false;
  const int64_t cols4 = c / 4;
  if (!((cols4 <= GNB_T && GNB_T % cols4 == 0) || (cols4 > GNB_T && cols4 % GNB_T == 0))) return false;
  return nseg >= 0 && nseg < 65536;
}

struct GnbLayout {
  double* partial;
  double* tot;
  float* ab;
  size_t bytes;
};

GnbLayout gnb_layout(void* ws, int64_t c, int64_t groups, int64_t nseg, int blocks) {
  Carver cv(ws);
  GnbLayout l;
  l.partial = cv.take<double>((size_t)nseg * blocks * 2 * c);
  l.tot = cv.take<double>((size_t)nseg * 2 * c);
  l.ab = cv.take<float>((size_t)nseg * 2 * groups);
  l.bytes = cv.used();
  return l;
}

}  // namespace
}  // namespace gr

extern "C" size_t gr_group_norm_backward_workspace_bytes(int64_t c, int64_t groups, int64_t nseg) {
  if (!gr::gnb_shape_ok(c, groups, nseg) || nseg == 0) return 0;
  return gr::gnb_layout(nullptr, c, groups, nseg, gr::gnb_block_cap(c, nseg)).bytes;
}

extern "C" int gr_group_norm_backward(const float* x, const float* out, const float* grad_out, const float* gamma,
                                      const float* stats, int64_t n, int64_t c, int64_t groups, float negative_slope,
                                      const int64_t* seg_off, int64_t nseg, int64_t max_seg_rows, float* grad_x,
                                      float* grad_residual, float* grad_gamma, float* grad_beta, void* ws, size_t ws_bytes,
                                      void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const bool seg = seg_off != nullptr;
  if (!seg) nseg = 1, max_seg_rows = n;
  GR_REQUIRE(n >= 0 && c >= 4 && groups >= 1 && groups <= gr::GNB_MAXG && c % groups == 0,
             "group_norm_backward: bad sizes (at most 64 groups, which divide the channels)");
  GR_REQUIRE(gr::gnb_shape_ok(c, groups, 1),
             "group_norm_backward: %lld channels are not supported (C / 4 must divide 256 or be a multiple of it)", (long long)c);
  GR_REQUIRE(nseg >= 0 && nseg < 65536 && max_seg_rows >= 0 && max_seg_rows <= n, "group_norm_backward: bad segments");
  GR_REQUIRE(negative_slope > 0.f, "group_norm_backward: negative_slope must be positive (the sign of out stands for the "
                                   "sign of the pre-activation)");
  auto aligned = [](const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; };
  if (n == 0 || nseg == 0) {
    if (grad_gamma) GR_HIP(hipMemsetAsync(grad_gamma, 0, sizeof(float) * c, stream));
    if (grad_beta) GR_HIP(hipMemsetAsync(grad_beta, 0, sizeof(float) * c, stream));
    return GR_OK;
  }
  const int act = negative_slope != 1.f;
  GR_REQUIRE(x && grad_out && stats && (out || !act), "group_norm_backward: null argument");
  GR_REQUIRE(aligned(x) && aligned(out) && aligned(grad_out) && aligned(gamma) && aligned(grad_x) && aligned(grad_residual),
             "group_norm_backward: unaligned tensors");
  if (!grad_x && !grad_residual && !grad_gamma && !grad_beta) return GR_OK;
  const int64_t cols4 = c / 4;
  const int rows_per_pass = cols4 >= gr::GNB_T ? 1 : (int)(gr::GNB_T / cols4);
  const int tiles = (int)std::min<int64_t>(std::max<int64_t>((max_seg_rows + rows_per_pass - 1) / rows_per_pass, 1), 1 << 20);
  const int nblk_a = std::min(gr::gnb_block_cap(c, nseg), tiles);
  const int nblk_b = std::min(tiles, seg ? std::max(8, 4096 / (int)std::min<int64_t>(nseg, 512)) : 4096);
  const gr::GnbLayout l = gr::gnb_layout(ws, c, groups, nseg, nblk_a);
  GR_REQUIRE(ws != nullptr && ws_bytes >= l.bytes, "group_norm_backward: workspace too small (%zu bytes, %zu needed)", ws_bytes,
             l.bytes);
  const unsigned gy = (unsigned)nseg;
  gr::KernelTimer timer("group_norm_backward", stream);
  if (grad_residual)
    hipLaunchKernelGGL(gr::group_norm_bwd_sums_kernel<true>, dim3(nblk_a, gy), dim3(gr::GNB_T), 0, stream, x, out, grad_out,
                       stats, n, (int)c, (int)groups, negative_slope, act, l.partial, seg_off, grad_residual);
  else
    hipLaunchKernelGGL(gr::group_norm_bwd_sums_kernel<false>, dim3(nblk_a, gy), dim3(gr::GNB_T), 0, stream, x, out, grad_out,
                       stats, n, (int)c, (int)groups, negative_slope, act, l.partial, seg_off, (float*)nullptr);
  if (grad_x || grad_gamma || grad_beta) {
    hipLaunchKernelGGL(gr::group_norm_bwd_fold_kernel, dim3((unsigned)((c + gr::GNB_FOLD_CH - 1) / gr::GNB_FOLD_CH), gy),
                       dim3(gr::GNB_T), 0, stream, l.partial, nblk_a, (int)c, l.tot);
    const int nb_param = (grad_gamma || grad_beta) ? (int)((c + gr::GNB_T - 1) / gr::GNB_T) : 0;
    const int nb_ab = grad_x ? (int)((nseg * groups + gr::GNB_T / 4 - 1) / (gr::GNB_T / 4)) : 0;
    hipLaunchKernelGGL(gr::group_norm_bwd_finish_kernel, dim3(nb_param + nb_ab), dim3(gr::GNB_T), 0, stream, l.tot, gamma, n,
                       (int)c, (int)groups, (int)nseg, nb_param, seg_off, grad_gamma, grad_beta, l.ab);
  }
  if (grad_x) {
    if (grad_residual)
      hipLaunchKernelGGL(gr::group_norm_bwd_apply_kernel<true>, dim3(nblk_b, gy), dim3(gr::GNB_T), 0, stream, x, out,
                         (const float*)grad_residual, gamma, stats, l.ab, n, (int)c, (int)groups, negative_slope, act, seg_off,
                         grad_x);
    else
      hipLaunchKernelGGL(gr::group_norm_bwd_apply_kernel<false>, dim3(nblk_b, gy), dim3(gr::GNB_T), 0, stream, x, out, grad_out,
                         gamma, stats, l.ab, n, (int)c, (int)groups, negative_slope, act, seg_off, grad_x);
  }
  GR_LAUNCH_CHECK();
  return GR_OK;
}
