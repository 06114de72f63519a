// Backward of the fused RPE attention (geo_embedding.hip: gr_rpe_attention), two launches and no float atomics.
//
// With P the saved softmax, hb the channel block of head h and f[n,m] = factors[n,m] * key_weights[m] / sqrt(ch):
//   dP[h,m] = grad_hidden[n,hb] . v[m,hb] (+ grad_scores[h,n,m])     D[h] = sum_m P[h,m] dP[h,m]
//   dz[h,m] = P[h,m] (dP[h,m] - D[h]) f[n,m]                          (the gradient of the raw score q.k + emb.u + add)
//   grad_q[n,hb] = sum_m dz[h,m] k[m,hb]      grad_u[n,h,:] = sum_m dz[h,m] emb[n,m,:]      grad_add[n,h] = sum_m dz[h,m]
//   grad_embed[n,m,:] = sum_h dz[h,m] u[n,h,:]
//   grad_k[m,hb] = sum_n dz[h,n,m] q[n,hb]    grad_v[m,hb] = sum_n P[h,n,m] grad_hidden[n,hb]
//
// Row pass (rpe_bwd_row_kernel): one workgroup per query row, as in the forward.  dP, then dz, live in LDS for all heads
// ((H, M) floats: P itself is read once from the saved scores and not kept).  The embedding row block -- the only N*M*C
// stream of the backward -- is read exactly once: the same float4 loads feed grad_u and, when wanted, grad_embed; the key
// rows ride along for grad_q.  dz leaves as (H, N, M) for the column pass.
// Column pass (rpe_bwd_col_kernel): the two sums over the queries are per-head products (M x N) . (N x ch) on the shared
// fp32 MFMA tile (mfma_tile.hpp), A = dz[h] or P[h] read transposed, B = a column block of q or grad_hidden.
// Every sum runs in an order fixed by the shapes: two runs give the same bits.
#include "common.hpp"
#include "mfma_tile.hpp"

namespace gr {
namespace {

constexpr size_t RPB_LDS_MAX = 150 * 1024;  // the forward's guard: the kernel's few static bytes count against the CU's 160 KB too

// dynamic LDS of the row pass: (H, M) floats padded to a float4, then the four waves' partial rows of grad_u and grad_q
size_t rpb_lds_bytes(int64_t m, int64_t c, int64_t heads) {
  return (((size_t)heads * m + 3) / 4 * 4 + 4 * (size_t)(heads + 1) * c) * sizeof(float);
}

template <int H, int CV>
__global__ __launch_bounds__(256) void rpe_bwd_row_kernel(
    const float* __restrict__ emb, const float* __restrict__ u, const float* __restrict__ k, const float* __restrict__ v,
    const float* __restrict__ factors, const float* __restrict__ key_weights, const float* __restrict__ scores,
    const float* __restrict__ grad_hidden, const float* __restrict__ grad_scores, int n_rows, int m_cols, float inv_sqrt_ch,
    float* __restrict__ dz_out, float* __restrict__ grad_q, float* __restrict__ grad_u, float* __restrict__ grad_add,
    float* __restrict__ grad_embed) {
  constexpr int C = CV * 64, CH = C / H;
  extern __shared__ float4 s_dyn[];
  float* s_dz = reinterpret_cast<float*>(s_dyn);                 // [H][m_cols]
  float* s_part = s_dz + ((H * m_cols + 3) / 4) * 4;             // [4][(H + 1) * C]
  const int n = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, sub = lane & 15, grp = lane >> 4;
  // ---- 1. dP[h][m] = grad_hidden[n, hb] . v[m, hb] (+ grad_scores): 16 lanes share one key row
  {
    float4 gr4[CV];
#pragma unroll
    for (int i = 0; i < CV; ++i) gr4[i] = *reinterpret_cast<const float4*>(grad_hidden + (int64_t)n * C + i * 64 + sub * 4);
    for (int m = w * 4 + grp; m < m_cols; m += 16) {
      const float* vrow = v + (int64_t)m * C + sub * 4;
      float acc[H];
#pragma unroll
      for (int h = 0; h < H; ++h) acc[h] = 0.f;
#pragma unroll
      for (int i = 0; i < CV; ++i) {
        const float4 vv = *reinterpret_cast<const float4*>(vrow + i * 64);
        const float part = fmaf(gr4[i].x, vv.x, fmaf(gr4[i].y, vv.y, fmaf(gr4[i].z, vv.z, gr4[i].w * vv.w)));
        const int hd = (i * 64 + sub * 4) / CH;
#pragma unroll
        for (int h = 0; h < H; ++h) acc[h] += hd == h ? part : 0.f;
      }
#pragma unroll
      for (int h = 0; h < H; ++h) {
#pragma unroll
        for (int d = 8; d > 0; d >>= 1) acc[h] += __shfl_xor(acc[h], d, 64);
      }
      if (sub < H) {
        float val = acc[0];
#pragma unroll
        for (int h = 1; h < H; ++h) val = sub == h ? acc[h] : val;
        if (grad_scores) val += grad_scores[((int64_t)sub * n_rows + n) * m_cols + m];
        s_dz[sub * m_cols + m] = val;
      }
    }
  }
  __syncthreads();
  // ---- 2. D[h], dz[h][m] and grad_add[n][h]: one wave per head (two heads per wave when H = 8)
  for (int h = w; h < H; h += 4) {
    float* row = s_dz + h * m_cols;
    const float* prow = scores + ((int64_t)h * n_rows + n) * m_cols;
    float dsum = 0.f;
    for (int m = lane; m < m_cols; m += 64) dsum = fmaf(prow[m], row[m], dsum);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) dsum += __shfl_xor(dsum, d, 64);
    float* dst = dz_out + ((int64_t)h * n_rows + n) * m_cols;
    float asum = 0.f;
    for (int m = lane; m < m_cols; m += 64) {
      float f = inv_sqrt_ch;
      if (factors) f = factors[(int64_t)n * m_cols + m] * f;
      if (key_weights) f = f * key_weights[m];
      const float dz = prow[m] * (row[m] - dsum) * f;
      row[m] = dz;
      dst[m] = dz;
      asum += dz;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) asum += __shfl_xor(asum, d, 64);
    if (lane == 0) grad_add[n * H + h] = asum;
  }
  __syncthreads();
  // ---- 3. the embedding stream: grad_u and grad_q accumulate per 16-lane group, grad_embed leaves row by row
  float4 au[H][CV], aq[CV], ur[H][CV];
#pragma unroll
  for (int i = 0; i < CV; ++i) {
    aq[i] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int h = 0; h < H; ++h) {
      au[h][i] = make_float4(0.f, 0.f, 0.f, 0.f);
      ur[h][i] = grad_embed ? *reinterpret_cast<const float4*>(u + ((int64_t)n * H + h) * C + i * 64 + sub * 4)
                            : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  for (int m = w * 4 + grp; m < m_cols; m += 16) {
    const int64_t eoff = ((int64_t)n * m_cols + m) * C + sub * 4;
    const float* krow = k + (int64_t)m * C + sub * 4;
    float4 e[CV], kk[CV];
#pragma unroll
    for (int i = 0; i < CV; ++i) {
      e[i] = *reinterpret_cast<const float4*>(emb + eoff + i * 64);
      kk[i] = *reinterpret_cast<const float4*>(krow + i * 64);
    }
    float dz[H];
#pragma unroll
    for (int h = 0; h < H; ++h) dz[h] = s_dz[h * m_cols + m];
#pragma unroll
    for (int i = 0; i < CV; ++i) {
#pragma unroll
      for (int h = 0; h < H; ++h) {
        au[h][i].x = fmaf(dz[h], e[i].x, au[h][i].x);
        au[h][i].y = fmaf(dz[h], e[i].y, au[h][i].y);
        au[h][i].z = fmaf(dz[h], e[i].z, au[h][i].z);
        au[h][i].w = fmaf(dz[h], e[i].w, au[h][i].w);
      }
      const int hd = (i * 64 + sub * 4) / CH;
      float dq = dz[0];
#pragma unroll
      for (int h = 1; h < H; ++h) dq = hd == h ? dz[h] : dq;
      aq[i].x = fmaf(dq, kk[i].x, aq[i].x);
      aq[i].y = fmaf(dq, kk[i].y, aq[i].y);
      aq[i].z = fmaf(dq, kk[i].z, aq[i].z);
      aq[i].w = fmaf(dq, kk[i].w, aq[i].w);
    }
    if (grad_embed) {
#pragma unroll
      for (int i = 0; i < CV; ++i) {
        float4 g = make_float4(dz[0] * ur[0][i].x, dz[0] * ur[0][i].y, dz[0] * ur[0][i].z, dz[0] * ur[0][i].w);
#pragma unroll
        for (int h = 1; h < H; ++h) {
          g.x = fmaf(dz[h], ur[h][i].x, g.x);
          g.y = fmaf(dz[h], ur[h][i].y, g.y);
          g.z = fmaf(dz[h], ur[h][i].z, g.z);
          g.w = fmaf(dz[h], ur[h][i].w, g.w);
        }
        *reinterpret_cast<float4*>(grad_embed + eoff + i * 64) = g;
      }
    }
  }
  // the four groups of a wave (xor butterfly: the same bits in every lane), then the four waves through LDS
  float4* part = reinterpret_cast<float4*>(s_part) + w * ((H + 1) * C / 4);
#pragma unroll
  for (int i = 0; i < CV; ++i) {
#pragma unroll
    for (int h = 0; h <= H; ++h) {
      float4 a = h < H ? au[h < H ? h : 0][i] : aq[i];
#pragma unroll
      for (int d = 16; d <= 32; d <<= 1) {
        a.x += __shfl_xor(a.x, d, 64);
        a.y += __shfl_xor(a.y, d, 64);
        a.z += __shfl_xor(a.z, d, 64);
        a.w += __shfl_xor(a.w, d, 64);
      }
      if (grp == 0) part[(h * C + i * 64) / 4 + sub] = a;
    }
  }
  __syncthreads();
  {
    constexpr int PER = (H + 1) * C / 4;  // float4 per wave: grad_u[n] (H * C floats) followed by grad_q[n] (C floats)
    const float4* p = reinterpret_cast<const float4*>(s_part);
    for (int j = tid; j < PER; j += 256) {
      const float4 a = p[j], b = p[PER + j], c2 = p[2 * PER + j], d2 = p[3 * PER + j];
      float4 r;
      r.x = (a.x + b.x) + (c2.x + d2.x);
      r.y = (a.y + b.y) + (c2.y + d2.y);
      r.z = (a.z + b.z) + (c2.z + d2.z);
      r.w = (a.w + b.w) + (c2.w + d2.w);
      if (j < H * C / 4)
        reinterpret_cast<float4*>(grad_u + (int64_t)n * H * C)[j] = r;
      else
        reinterpret_cast<float4*>(grad_q + (int64_t)n * C)[j - H * C / 4] = r;
    }
  }
}

// blockIdx.z = 2 h + (0: grad_k = dz[h]^T q[:, hb],  1: grad_v = P[h]^T grad_hidden[:, hb]); a 64 x 64 tile of (M, ch)
__global__ __launch_bounds__(256) void rpe_bwd_col_kernel(const float* __restrict__ dz, const float* __restrict__ scores,
                                                          const float* __restrict__ q, const float* __restrict__ grad_hidden,
                                                          int n_rows, int m_cols, int c, int ch, float* __restrict__ grad_k,
                                                          float* __restrict__ grad_v) {
  const int h = blockIdx.z >> 1;
  const bool is_v = blockIdx.z & 1;
  const float* A = (is_v ? scores : dz) + (int64_t)h * n_rows * m_cols;
  const float* B = (is_v ? grad_hidden : q) + h * ch;
  float* out = (is_v ? grad_v : grad_k) + h * ch;
  gemm64_tile<false, false, false>(A, m_cols, B, c, m_cols, ch, 0, n_rows, nullptr, nullptr,
                                   [=](int gi, int gj, float val) { out[(int64_t)gi * c + gj] = val; });
}

}  // namespace
}  // namespace gr

extern "C" size_t gr_rpe_attention_backward_workspace_bytes(int64_t n, int64_t m, int64_t heads) {
  if (n < 0 || m < 0 || heads < 0) return 0;
  return gr::align_up((size_t)heads * n * m * sizeof(float), 256) + 256;
}

extern "C" int64_t gr_rpe_attention_backward_max_keys(int64_t c, int64_t heads) {
  if (c <= 0 || heads <= 0) return 0;
  const size_t fixed = 4 * (size_t)(heads + 1) * c * sizeof(float);
  if (fixed >= gr::RPB_LDS_MAX) return 0;
  int64_t m = (int64_t)((gr::RPB_LDS_MAX - fixed) / (sizeof(float) * heads));
  while (m > 0 && gr::rpb_lds_bytes(m, c, heads) > gr::RPB_LDS_MAX) --m;  // the float4 padding of the (H, M) block
  return m;
}

extern "C" int gr_rpe_attention_backward(const float* embed, const float* u, const float* q, const float* k, const float* v,
                                         const float* scores, const float* attention_factors, const float* key_weights,
                                         const float* grad_hidden, const float* grad_scores, int64_t n, int64_t m, int64_t c,
                                         int64_t heads, float* grad_q, float* grad_k, float* grad_v, float* grad_u,
                                         float* grad_add, float* grad_embed, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  GR_REQUIRE(n >= 0 && m >= 0 && n < (1 << 24) && m < (1 << 24), "rpe_attention_backward: bad sizes");
  GR_REQUIRE((c == 64 || c == 128 || c == 256) && (heads == 1 || heads == 2 || heads == 4 || heads == 8),
             "rpe_attention_backward: d_model must be 64/128/256 and num_heads 1/2/4/8 (got %lld, %lld)", (long long)c,
             (long long)heads);
  if (n == 0) {  // no query: nothing reaches the keys
    if (m > 0) {
      GR_REQUIRE(grad_k && grad_v, "null argument");
      GR_HIP(hipMemsetAsync(grad_k, 0, (size_t)m * c * sizeof(float), stream));
      GR_HIP(hipMemsetAsync(grad_v, 0, (size_t)m * c * sizeof(float), stream));
    }
    return GR_OK;
  }
  GR_REQUIRE(m > 0, "rpe_attention_backward: no keys (softmax over an empty row)");
  GR_REQUIRE(embed && u && q && k && v && scores && grad_hidden && grad_q && grad_k && grad_v && grad_u && grad_add,
             "null argument");
  const size_t lds = gr::rpb_lds_bytes(m, c, heads);
  GR_REQUIRE(lds <= gr::RPB_LDS_MAX, "rpe_attention_backward: %lld keys x %lld heads do not fit in LDS", (long long)m,
             (long long)heads);
  GR_REQUIRE(ws && ws_bytes >= gr_rpe_attention_backward_workspace_bytes(n, m, heads),
             "rpe_attention_backward: workspace too small");
  gr::Carver carve(ws);
  float* dz = carve.take<float>((size_t)heads * n * m);
  const float inv_sqrt_ch = 1.0f / sqrtf((float)(c / heads));
  {
    gr::KernelTimer timer("rpe_attention_backward_rows", stream);
#define GR_RPB(H, CV)                                                                                                 \
  do {                                                                                                                \
    auto kern = gr::rpe_bwd_row_kernel<H, CV>;                                                                        \
    if (lds > 64 * 1024)                                                                                              \
      GR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,    \
                                 (int)lds));                                                                          \
    hipLaunchKernelGGL(kern, dim3((unsigned)n), dim3(256), lds, stream, embed, u, k, v, attention_factors, key_weights, \
                       scores, grad_hidden, grad_scores, (int)n, (int)m, inv_sqrt_ch, dz, grad_q, grad_u, grad_add,   \
                       grad_embed);                                                                                   \
  } while (0)
#define GR_RPB_H(CV)               \
  switch (heads) {                 \
    case 1: GR_RPB(1, CV); break;  \
    case 2: GR_RPB(2, CV); break;  \
    case 4: GR_RPB(4, CV); break;  \
    default: GR_RPB(8, CV); break; \
  }
    if (c == 64) { GR_RPB_H(1); } else if (c == 128) { GR_RPB_H(2); } else { GR_RPB_H(4); }
#undef GR_RPB_H
#undef GR_RPB
    GR_LAUNCH_CHECK();
  }
  {
    gr::KernelTimer timer("rpe_attention_backward_cols", stream);
    const int ch = (int)(c / heads);
    const dim3 grid((unsigned)((ch + gr::GT - 1) / gr::GT), (unsigned)((m + gr::GT - 1) / gr::GT), (unsigned)(2 * heads));
    hipLaunchKernelGGL(gr::rpe_bwd_col_kernel, grid, dim3(256), 0, stream, dz, scores, q, grad_hidden, (int)n, (int)m,
                       (int)c, ch, grad_k, grad_v);
    GR_LAUNCH_CHECK();
  }
  return GR_OK;
}
