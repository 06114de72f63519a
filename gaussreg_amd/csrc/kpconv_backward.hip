// KPConv backward (geotransformer/modules/kpconv/kpconv.py:90-120 differentiated) and the backward of the two pooling
// helpers (functional.py:6-22, 54-67), without float atomics: every sum has a fixed order, so two calls on the same inputs
// return the same bits.
//
// With g[m,:] = grad_out[m,:] / num[m]  (num = max(neighbor_num, 1) comes from a comparison and carries no gradient):
//   grad_bias         = sum_m grad_out[m,:]                       column sums per slab of rows, slabs folded in order
//   grad_W (Kd x Co)  = WF^T . g                                  WF recomputed by the forward's own gather kernels;
//                                                                 one partial product per slab of queries on fp32 MFMA,
//                                                                 slabs folded in ascending order
//   gWF (M x Kd)      = g . W^T                                   fp32 MFMA
//   grad_f[n,:]       = sum over edges (m,h) with nb[m,h] = n of sum_k w[m,h,k] gWF[m,k,:]
//                                                                 one lane group per SUPPORT row walks the row's list of
//                                                                 the inverted neighbour index (ascending (m,h)), recomputes
//                                                                 the K influences of the edge from the two points and reads
//                                                                 the gWF rows whose influence is not 0 -- no (M,H,Cin)
//                                                                 per-edge temporary exists at all
// The queries are processed in chunks of at most 64 MB of WF / gWF each; chunk c adds into grad_f and grad_W after chunk c-1.
#include <algorithm>

#include "common.hpp"
#include "mfma_tile.hpp"

namespace gr {
namespace {

constexpr int KPB_KMAX = 16;                     // kernel points, as the forward
constexpr int64_t KPB_CHUNK_BYTES = 64ll << 20;  // WF and gWF of one chunk of queries, each
constexpr int64_t KPB_PART_BYTES = 32ll << 20;   // grad_W partial products of one chunk
constexpr int KPB_MAX_SLABS = 32;

// max(#{h : neighbour valid and flagged}, 1) per query: what the gather kernels leave in `num`, for the calls that skip them
__global__ __launch_bounds__(256) void kpb_num_kernel(const int64_t* __restrict__ nbr, int N, int M, int H,
                                                      const uint8_t* __restrict__ flag, float* __restrict__ num) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  int cnt = 0;
  for (int h = 0; h < H; ++h) {
    const int64_t idx = nbr[(int64_t)m * H + h];
    if (idx >= 0 && idx < N) cnt += flag[idx];
  }
  num[m] = (float)max(cnt, 1);
}

// C (Mi x Nj) = A (Mi x Kd) . B (Kd x Nj) over the k range of slab blockIdx.z: the 64 x 64 tile of mfma_tile.hpp with the
// operands divided while they are staged (A(i,k) / denA[i], B(k,j) / denB[k], each when given).
template <bool A_KFAST, bool B_KFAST>
__global__ __launch_bounds__(256) void kpb_gemm_kernel(const float* __restrict__ A, int64_t lda, const float* __restrict__ B,
                                                       int64_t ldb, int Mi, int Nj, int Kd, int kslab,
                                                       const float* __restrict__ denA, const float* __restrict__ denB,
                                                       float* __restrict__ out, int64_t ldo, int64_t slab_stride) {
  const int kb = blockIdx.z * kslab, ke = min(Kd, kb + kslab);
  out += (int64_t)blockIdx.z * slab_stride;
  gemm64_tile<A_KFAST, B_KFAST, true>(A, lda, B, ldb, Mi, Nj, kb, ke, denA, denB,
                                      [=](int gi, int gj, float v) { out[(int64_t)gi * ldo + gj] = v; });
}

// out[i] = (accumulate ? out[i] : 0) + ((p[0][i] + p[1][i]) + p[2][i]) + ...   -- the slabs in ascending order
__global__ __launch_bounds__(256) void kpb_fold_kernel(const float* __restrict__ partial, int nslab, int64_t stride,
                                                       int64_t count, float* __restrict__ out, int accumulate) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  float s = partial[i];
  for (int k = 1; k < nslab; ++k) s += partial[(int64_t)k * stride + i];
  out[i] = accumulate ? out[i] + s : s;
}

// column sums of x (M x C) over the rows of slab blockIdx.y: 64 columns x 4 row lanes per workgroup
__global__ __launch_bounds__(256) void kpb_colsum_kernel(const float* __restrict__ x, int M, int C, int slab_rows,
                                                         float* __restrict__ partial) {
  __shared__ float s_part[4][64];
  const int col = blockIdx.x * 64 + (threadIdx.x & 63), rsub = threadIdx.x >> 6;
  const int r0 = blockIdx.y * slab_rows, r1 = min(M, r0 + slab_rows);
  float s = 0.f;
  if (col < C)
    for (int r = r0 + rsub; r < r1; r += 4) s += x[(int64_t)r * C + col];
  s_part[rsub][threadIdx.x & 63] = s;
  __syncthreads();
  if (rsub == 0 && col < C)
    partial[(int64_t)blockIdx.y * C + col] = ((s_part[0][threadIdx.x] + s_part[1][threadIdx.x]) + s_part[2][threadIdx.x]) +
                                             s_part[3][threadIdx.x];
}

// first position in the ascending list [b, e) whose edge id is >= key
__device__ __forceinline__ int64_t kpb_lower_bound(const int64_t* __restrict__ edges, int64_t b, int64_t e, int64_t key) {
  while (b < e) {
    const int64_t mid = (b + e) >> 1;
    if (edges[mid] < key) b = mid + 1; else e = mid;
  }
  return b;
}

// grad_f of one chunk of queries [m0, m1): G lanes per support row, a lane owns the channels c = sub, sub + G, ...
// edges: the valid (m, h) pairs as m * H + h, grouped by support row (offsets: N + 1 entries), ascending inside a row.
// The sum over the edges of a row is compensated (Kahan): the hub row of a dense neighbourhood adds thousands of terms.
template <int G>
__global__ __launch_bounds__(256) void kpb_rowsum_kernel(const float* __restrict__ gWF, const float* __restrict__ q_points,
                                                         const float* __restrict__ s_points,
                                                         const int64_t* __restrict__ edges,
                                                         const int64_t* __restrict__ offsets, int N, int H, int Cin, int K,
                                                         const float* __restrict__ kpts, float sigma, int64_t m0, int64_t m1,
                                                         float* __restrict__ grad_f, int accumulate) {
  const int sub = threadIdx.x % G;
  const int64_t row = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;
  if (row >= N) return;
  const int64_t lo = kpb_lower_bound(edges, offsets[row], offsets[row + 1], m0 * H);
  const int64_t hi = kpb_lower_bound(edges, lo, offsets[row + 1], m1 * H);
  const float sx = s_points[3 * row], sy = s_points[3 * row + 1], sz = s_points[3 * row + 2];
  const int64_t kd = (int64_t)K * Cin;
  for (int c = sub; c < Cin; c += G) {
    float acc = 0.f, comp = 0.f;
    for (int64_t j = lo; j < hi; ++j) {
      const uint32_t m = (uint32_t)edges[j] / (uint32_t)H;  // m * H + h < 2^31 (the host checks)
      // the forward's influence, operation for operation (kpconv.py:90-98)
      const float nx = sx - q_points[3 * (int64_t)m], ny = sy - q_points[3 * (int64_t)m + 1], nz = sz - q_points[3 * (int64_t)m + 2];
      const float* g = gWF + ((int64_t)m - m0) * kd + c;
      float t = 0.f;
      for (int k = 0; k < K; ++k) {
        const float dx = nx - kpts[3 * k], dy = ny - kpts[3 * k + 1], dz = nz - kpts[3 * k + 2];
        const float sq = (dx * dx + dy * dy) + dz * dz;
        const float wk = fmaxf(1.0f - sqrtf(sq) / sigma, 0.0f);
        if (wk > 0.0f) t = fmaf(wk, g[(int64_t)k * Cin], t);
      }
      const float y = t - comp, s2 = acc + y;
      comp = (s2 - acc) - y;
      acc = s2;
    }
    float* dst = grad_f + row * Cin + c;
    *dst = accumulate ? *dst + acc : acc;
  }
}

// maxpool: the neighbour column that attains the maximum of (m, c): lowest h on a tie, -1 when the zero shadow row wins
__global__ __launch_bounds__(256) void pool_argmax_kernel(const float* __restrict__ x, int N, int C,
                                                          const int64_t* __restrict__ nbr, int M, int H,
                                                          int32_t* __restrict__ arg) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)M * C) return;
  const int m = (int)(e / C), c = (int)(e % C);
  float best = -INFINITY;
  int a = -1;
  for (int h = 0; h < H; ++h) {
    const int64_t idx = nbr[(int64_t)m * H + h];
    const bool pad = idx >= N || idx < 0;
    const float v = pad ? 0.f : x[idx * C + c];
    if (v > best) {
      best = v;
      a = pad ? -1 : h;
    }
  }
  arg[e] = a;
}

// grad_x[n, c] = sum over the edges (m, h) of row n (ascending) that won (arg == h; arg null: every listed edge) of grad[m, c]
__global__ __launch_bounds__(256) void pool_rowsum_kernel(const float* __restrict__ grad, int N, int C, int H,
                                                          const int64_t* __restrict__ edges,
                                                          const int64_t* __restrict__ offsets,
                                                          const int32_t* __restrict__ arg, float* __restrict__ grad_x) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)N * C) return;
  const int64_t row = e / C;
  const int c = (int)(e % C);
  float acc = 0.f, comp = 0.f;
  for (int64_t j = offsets[row]; j < offsets[row + 1]; ++j) {
    const uint32_t ed = (uint32_t)edges[j];
    const uint32_t m = ed / (uint32_t)H, h = ed % (uint32_t)H;
    const int64_t o = (int64_t)m * C + c;
    if (arg != nullptr && arg[o] != (int)h) continue;
    const float y = grad[o] - comp, s2 = acc + y;
    comp = (s2 - acc) - y;
    acc = s2;
  }
  grad_x[e] = acc;
}

struct KpbLayout {
  int64_t chunk_rows, nchunk, slab_rows, nslab, bias_slab_rows, bias_nslab;
};

KpbLayout kpb_layout(int64_t m, int64_t k, int64_t cin, int64_t cout, int64_t chunk_override) {
  KpbLayout L;
  const int64_t kd = k * cin;
  int64_t rows = chunk_override > 0 ? chunk_override : std::max<int64_t>(256, KPB_CHUNK_BYTES / (kd * 4) / 256 * 256);
  L.chunk_rows = std::max<int64_t>(1, std::min(rows, std::max<int64_t>(m, 1)));
  L.nchunk = m > 0 ? (m + L.chunk_rows - 1) / L.chunk_rows : 0;
  const int64_t max_slabs = std::max<int64_t>(1, std::min<int64_t>(KPB_MAX_SLABS, KPB_PART_BYTES / (kd * cout * 4)));
  L.slab_rows = std::max<int64_t>(64, (L.chunk_rows + max_slabs - 1) / max_slabs);
  L.slab_rows = (L.slab_rows + GK - 1) / GK * GK;
  L.nslab = (L.chunk_rows + L.slab_rows - 1) / L.slab_rows;
  L.bias_slab_rows = std::max<int64_t>(64, (m + 63) / 64);
  L.bias_nslab = m > 0 ? (m + L.bias_slab_rows - 1) / L.bias_slab_rows : 0;
  return L;
}

}  // namespace
}  // namespace gr

using namespace gr;

extern "C" int gr_kpconv_backward_plan(int64_t n, int64_t m, int64_t h, int64_t cin, int64_t cout, int64_t k, int needs,
                                       int64_t chunk_override) {
  if (n < 0 || m < 0 || h < 0 || cin < 1 || cout < 1 || k < 1 || k > KPB_KMAX || chunk_override < 0) return -1;
  int plan = 0;
  if (needs & GR_KPB_NEED_BIAS) plan |= GR_KPB_BIAS;
  if (m == 0 || n == 0 || h == 0) return plan | GR_KPB_EMPTY;
  const KpbLayout L = kpb_layout(m, k, cin, cout, chunk_override);
  if (needs & GR_KPB_NEED_WEIGHTS) plan |= GR_KPB_WEIGHTS | (L.nslab > 1 ? GR_KPB_WEIGHTS_SLABS : 0);
  if (needs & GR_KPB_NEED_FEATS) {
    plan |= GR_KPB_FEATS | (cin <= 16 ? GR_KPB_SUM_G16 : cin <= 32 ? GR_KPB_SUM_G32 : GR_KPB_SUM_G64);
    if (cin > 64) plan |= GR_KPB_SUM_MULTIPASS;
  }
  if ((needs & (GR_KPB_NEED_WEIGHTS | GR_KPB_NEED_FEATS)) && L.nchunk > 1) plan |= GR_KPB_CHUNKED;
  return plan;
}

extern "C" size_t gr_kpconv_backward_workspace_bytes(int64_t n, int64_t m, int64_t h, int64_t cin, int64_t cout, int64_t k,
                                                     int needs, int64_t chunk_override) {
  if (n < 0 || m < 0 || h < 0 || cin < 1 || cout < 1 || k < 1 || chunk_override < 0) return 0;
  const KpbLayout L = kpb_layout(m, k, cin, cout, chunk_override);
  const bool live = m > 0 && n > 0 && h > 0;
  const size_t kd = (size_t)k * cin;
  size_t bytes = align_up((size_t)n + 1, 256) + align_up((size_t)m * sizeof(float), 256) + 1024;
  if (live && (needs & GR_KPB_NEED_WEIGHTS)) bytes += align_up((size_t)L.chunk_rows * kd * sizeof(float), 256);
  if (live && (needs & GR_KPB_NEED_FEATS)) bytes += align_up((size_t)L.chunk_rows * kd * sizeof(float), 256);
  size_t part = (needs & GR_KPB_NEED_BIAS) ? (size_t)L.bias_nslab * cout : 0;
  if (live && (needs & GR_KPB_NEED_WEIGHTS)) part = std::max(part, (size_t)L.nslab * kd * cout);
  return bytes + align_up(part * sizeof(float), 256);
}

extern "C" int gr_kpconv_backward(const float* s_feats, const float* q_points, const float* s_points,
                                  const int64_t* neighbor_indices, int64_t n, int64_t m, int64_t h, int64_t cin,
                                  int64_t cout, const float* kernel_points, int64_t k, const float* weights, float sigma,
                                  float inf, const float* grad_out, const int64_t* inv_edges, const int64_t* inv_offsets,
                                  float* grad_feats, float* grad_weights, float* grad_bias, int64_t chunk_override, void* ws,
                                  size_t ws_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  GR_REQUIRE(n >= 0 && m >= 0 && h >= 0 && cin >= 1 && cout >= 1 && k >= 1 && chunk_override >= 0, "bad sizes");
  GR_REQUIRE(k <= KPB_KMAX, "kernel_size must be <= %d", KPB_KMAX);
  GR_REQUIRE(n < (1ll << 31) && m < (1ll << 31) && m * std::max<int64_t>(h, 1) < (1ll << 31) && k * cin * cout < (1ll << 31),
             "sizes too large");
  const int needs = (grad_feats ? GR_KPB_NEED_FEATS : 0) | (grad_weights ? GR_KPB_NEED_WEIGHTS : 0) |
                    (grad_bias ? GR_KPB_NEED_BIAS : 0);
  if (needs == 0) return GR_OK;
  const int plan = gr_kpconv_backward_plan(n, m, h, cin, cout, k, needs, chunk_override);
  GR_REQUIRE(plan >= 0, "bad sizes");
  const int64_t kd = k * cin;
  KernelTimer timer("kpconv_backward", stream);
  if (plan & GR_KPB_EMPTY) {  // no query, no support point or no neighbour column: WF = 0, so nothing reaches f or W
    if (grad_feats && n > 0) GR_HIP(hipMemsetAsync(grad_feats, 0, (size_t)n * cin * sizeof(float), stream));
    if (grad_weights) GR_HIP(hipMemsetAsync(grad_weights, 0, (size_t)kd * cout * sizeof(float), stream));
    if (grad_bias && m == 0) GR_HIP(hipMemsetAsync(grad_bias, 0, (size_t)cout * sizeof(float), stream));
    if (m == 0 || !grad_bias) return GR_OK;
  }
  GR_REQUIRE(grad_out, "null argument");
  if (!ws || ws_bytes < gr_kpconv_backward_workspace_bytes(n, m, h, cin, cout, k, needs, chunk_override)) {
    set_error("kpconv backward workspace too small");
    return GR_ERR_WORKSPACE;
  }
  const KpbLayout L = kpb_layout(m, k, cin, cout, chunk_override);
  const bool live = !(plan & GR_KPB_EMPTY);
  const bool do_w = live && grad_weights, do_f = live && grad_feats;
  char* p = static_cast<char*>(ws);
  uint8_t* flag = reinterpret_cast<uint8_t*>(p);
  p += align_up((size_t)n + 1, 256);
  float* num = reinterpret_cast<float*>(p);
  p += align_up((size_t)m * sizeof(float), 256);
  float* WF = nullptr;
  float* gWF = nullptr;
  if (do_w) {
    WF = reinterpret_cast<float*>(p);
    p += align_up((size_t)L.chunk_rows * kd * sizeof(float), 256);
  }
  if (do_f) {
    gWF = reinterpret_cast<float*>(p);
    p += align_up((size_t)L.chunk_rows * kd * sizeof(float), 256);
  }
  float* partial = reinterpret_cast<float*>(p);

  if (grad_bias) {
    hipLaunchKernelGGL(kpb_colsum_kernel, dim3((unsigned)((cout + 63) / 64), (unsigned)L.bias_nslab), dim3(256), 0, stream,
                       grad_out, (int)m, (int)cout, (int)L.bias_slab_rows, partial);
    hipLaunchKernelGGL(kpb_fold_kernel, dim3((unsigned)((cout + 255) / 256)), dim3(256), 0, stream, partial, (int)L.bias_nslab,
                       cout, cout, grad_bias, 0);
  }
  if (!live || (!do_w && !do_f)) {
    GR_LAUNCH_CHECK();
    return GR_OK;
  }
  GR_REQUIRE(s_feats && s_points && q_points && neighbor_indices && kernel_points && weights, "null argument");
  GR_REQUIRE(!do_f || inv_offsets, "grad_feats needs the inverted neighbour index");  // no valid entry at all: inv_edges is empty
  kpconv_rowflag_launch(s_feats, n, cin, flag, stream);
  hipLaunchKernelGGL(kpb_num_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, stream, neighbor_indices, (int)n, (int)m,
                     (int)h, flag, num);
  for (int64_t ci = 0; ci < L.nchunk; ++ci) {
    const int64_t m0 = ci * L.chunk_rows, m1 = std::min(m, m0 + L.chunk_rows), mc = m1 - m0;
    const float* go = grad_out + m0 * cout;
    if (do_w) {
      // WF of the chunk, by the launches the forward uses for a call of mc queries
      const int fplan = gr_kpconv_plan(n, mc, h, cin, cout, k, 0);
      GR_REQUIRE(fplan >= 0, "bad sizes");
      kpconv_gather_launch(fplan, s_feats, q_points + 3 * m0, s_points, neighbor_indices + m0 * h, n, mc, h, cin, k,
                           kernel_points, sigma, inf, flag, WF, num + m0, stream);
      const int64_t nslab = (mc + L.slab_rows - 1) / L.slab_rows;
      // partial[s] (Kd x Cout) = WF[slab s]^T . g[slab s]
      hipLaunchKernelGGL((kpb_gemm_kernel<false, false>), dim3((unsigned)((cout + GT - 1) / GT), (unsigned)((kd + GT - 1) / GT),
                                                               (unsigned)nslab),
                         dim3(256), 0, stream, WF, kd, go, cout, (int)kd, (int)cout, (int)mc, (int)L.slab_rows,
                         (const float*)nullptr, num + m0, partial, cout, kd * cout);
      hipLaunchKernelGGL(kpb_fold_kernel, dim3((unsigned)((kd * cout + 255) / 256)), dim3(256), 0, stream, partial, (int)nslab,
                         kd * cout, kd * cout, grad_weights, ci > 0 ? 1 : 0);
    }
    if (do_f) {
      // gWF (mc x Kd) = g . W^T
      hipLaunchKernelGGL((kpb_gemm_kernel<true, true>), dim3((unsigned)((kd + GT - 1) / GT), (unsigned)((mc + GT - 1) / GT), 1u),
                         dim3(256), 0, stream, go, cout, weights, cout, (int)mc, (int)kd, (int)cout, (int)cout, num + m0,
                         (const float*)nullptr, gWF, kd, (int64_t)0);
#define GR_KPB_SUM(G)                                                                                                        \
  hipLaunchKernelGGL((kpb_rowsum_kernel<G>), dim3((unsigned)((n + 256 / G - 1) / (256 / G))), dim3(256), 0, stream, gWF,     \
                     q_points, s_points, inv_edges, inv_offsets, (int)n, (int)h, (int)cin, (int)k, kernel_points, sigma, m0, \
                     m1, grad_feats, ci > 0 ? 1 : 0)
      switch (plan & GR_KPB_SUM_MASK) {
        case GR_KPB_SUM_G16: GR_KPB_SUM(16); break;
        case GR_KPB_SUM_G32: GR_KPB_SUM(32); break;
        default: GR_KPB_SUM(64); break;
      }
#undef GR_KPB_SUM
    }
  }
  GR_LAUNCH_CHECK();
  return GR_OK;
}

extern "C" int gr_neighbor_pool_backward(const float* x, int64_t n, int64_t c, const int64_t* neighbor_indices, int64_t m,
                                         int64_t h, int mode, const float* grad_out, const int64_t* inv_edges,
                                         const int64_t* inv_offsets, float* grad_x, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  GR_REQUIRE(n >= 0 && c >= 1 && m >= 0 && h >= 1 && (mode == 0 || mode == 1), "bad arguments");
  GR_REQUIRE(n < (1ll << 31) && m * h < (1ll << 31) && m * c < (1ll << 40), "sizes too large");
  if (n == 0) return GR_OK;
  GR_REQUIRE(grad_x, "null argument");
  if (m == 0) {
    GR_HIP(hipMemsetAsync(grad_x, 0, (size_t)n * c * sizeof(float), stream));
    return GR_OK;
  }
  GR_REQUIRE(x && neighbor_indices && grad_out && inv_offsets, "null argument");  // inv_edges is empty when no entry is valid
  int32_t* arg = nullptr;
  if (mode == 0) {
    if (!ws || ws_bytes < (size_t)m * c * sizeof(int32_t)) {
      set_error("neighbor_pool_backward workspace too small");
      return GR_ERR_WORKSPACE;
    }
    arg = static_cast<int32_t*>(ws);
    hipLaunchKernelGGL(pool_argmax_kernel, dim3((unsigned)((m * c + 255) / 256)), dim3(256), 0, stream, x, (int)n, (int)c,
                       neighbor_indices, (int)m, (int)h, arg);
  }
  hipLaunchKernelGGL(pool_rowsum_kernel, dim3((unsigned)((n * c + 255) / 256)), dim3(256), 0, stream, grad_out, (int)n, (int)c,
                     (int)h, inv_edges, inv_offsets, arg, grad_x);
  GR_LAUNCH_CHECK();
  return GR_OK;
}
