// RPE attention (rpe_transformer.py:51-72): the positional score term, the fused forward and its backward.
//
// rpe_transformer.py:55-57 projects the whole (N,M,C) embedding through proj_p in EVERY attention layer
// (2*N*M*C^2 flop = 77 GFLOP at N=M=767, C=256, plus a 602 MB temporary) and then contracts it with q:
//     s_p[h,n,m] = sum_c q[h,n,c] * (W_p emb[n,m] + b_p)[h*ch + c]
// The sum is linear in emb, so it is re-associated as   s_p[h,n,m] = emb[n,m,:] . u[n,h,:] + q[h,n,:].b_p[h]
// with u[n,h,:] = W_p[h-block]^T q[h,n,:] (a tiny GEMM done by the caller): one pass over the embedding, memory-bound.
//
// The three row kernels (rpe_scores_kernel, rpe_attention_kernel, rpe_bwd_row_kernel) share one lane layout:
// workgroup = one query row n, 4 waves; 16 lanes share one (n,m) row (float4 loads, 256 B per 16 lanes: lane `sub` holds
// the channels i*64 + sub*4 .. +3 of chunk i < CV = C / 64); the four 16-lane groups of the four waves take the rows
// m = w*4 + grp, then every 16th.  The pieces on that layout are written once, below.
#include <type_traits>

#include "common.hpp"
#include "mfma_tile.hpp"

namespace gr {
namespace {

template <int H>
struct HeadVals {  // one float per head
  float v[H];
};

struct RowLanes {
  int lane, w, sub, grp;
  __device__ __forceinline__ int first_row() const { return w * 4 + grp; }
};
constexpr int ROW_STRIDE = 16;  // rows a workgroup takes per step: for (m = m_lo + L.first_row(); m < m_hi; m += ROW_STRIDE)

__device__ __forceinline__ RowLanes row_lanes() {
  const int lane = threadIdx.x & 63;
  return {lane, (int)(threadIdx.x >> 6), lane & 15, lane >> 4};
}

// this lane's CV float4 of a C-float row; `p` already points at the lane's first chunk (row + sub * 4)
template <int CV>
__device__ __forceinline__ void load_row(const float* __restrict__ p, float4 (&r)[CV]) {
#pragma unroll
  for (int i = 0; i < CV; ++i) r[i] = *reinterpret_cast<const float4*>(p + i * 64);
}

// the same for two rows, chunk by chunk: the order in which the loads are issued where two rows are needed at once
template <int CV>
__device__ __forceinline__ void load_row2(const float* __restrict__ pa, float4 (&a)[CV], const float* __restrict__ pb,
                                          float4 (&b)[CV]) {
#pragma unroll
  for (int i = 0; i < CV; ++i) {
    a[i] = *reinterpret_cast<const float4*>(pa + i * 64);
    b[i] = *reinterpret_cast<const float4*>(pb + i * 64);
  }
}

// this lane's share of a . b over all C channels
template <int CV>
__device__ __forceinline__ float row_dot(const float4 (&a)[CV], const float4 (&b)[CV]) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < CV; ++i) {
    s = fmaf(a[i].x, b[i].x, s);
    s = fmaf(a[i].y, b[i].y, s);
    s = fmaf(a[i].z, b[i].z, s);
    s = fmaf(a[i].w, b[i].w, s);
  }
  return s;
}

// acc[h] += this lane's share of a[hb] . b[hb]: the four channels of chunk i belong to head (i*64 + sub*4) / CH
template <int H, int CV>
__device__ __forceinline__ void head_dot_add(const float4 (&a)[CV], const float4 (&b)[CV], int sub, float (&acc)[H]) {
  constexpr int CH = CV * 64 / H;
#pragma unroll
  for (int i = 0; i < CV; ++i) {
    const float part = fmaf(a[i].x, b[i].x, fmaf(a[i].y, b[i].y, fmaf(a[i].z, b[i].z, a[i].w * b[i].w)));
    const int hd = (i * 64 + sub * 4) / CH;
#pragma unroll
    for (int h = 0; h < H; ++h) acc[h] += hd == h ? part : 0.f;
  }
}

// sum over the 16 lanes of a row, per head; every lane of the row ends with the same bits
template <int H>
__device__ __forceinline__ void reduce16(float (&acc)[H]) {
#pragma unroll
  for (int h = 0; h < H; ++h) {
#pragma unroll
    for (int d = 8; d > 0; d >>= 1) acc[h] += __shfl_xor(acc[h], d, 64);
  }
}

// x.v[idx] without a dynamic register index (lane `sub` keeps head `sub`).  By value: the select chain has to see values.
// Over loads through a reference the optimiser, which simplifies this function before it inlines it, merges the chain into one
// load at a selected address, and the caller's array then leaves the registers for scratch memory or LDS.
template <int H>
__device__ __forceinline__ float pick(const HeadVals<H> x, int idx) {
  float v = x.v[0];
#pragma unroll
  for (int h = 1; h < H; ++h) v = idx == h ? x.v[h] : v;
  return v;
}

__device__ __forceinline__ void axpy(float s, const float4& x, float4& y) {
  y.x = fmaf(s, x.x, y.x);
  y.y = fmaf(s, x.y, y.y);
  y.z = fmaf(s, x.z, y.z);
  y.w = fmaf(s, x.w, y.w);
}

// the four waves' partial rows
__device__ __forceinline__ float4 fold4(const float4& a, const float4& b, const float4& c, const float4& d) {
  return make_float4((a.x + b.x) + (c.x + d.x), (a.y + b.y) + (c.y + d.y), (a.z + b.z) + (c.z + d.z), (a.w + b.w) + (c.w + d.w));
}

__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) x = fmaxf(x, __shfl_xor(x, d, 64));
  return x;
}
__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d, 64);
  return x;
}

// ---------------------------------------------------------------- positional score term alone
// out[h,n,m] = emb[n,m,:] . u[n,h,:] (+ add[n,h]); blockIdx.y takes 256 key columns.
template <int H, int CV>  // CV = C / 64 (float4 chunks per lane)
__global__ __launch_bounds__(256) void rpe_scores_kernel(const float* __restrict__ emb, const float* __restrict__ u,
                                                         const float* __restrict__ add, int n_rows, int m_cols,
                                                         float* __restrict__ out) {
  constexpr int C = CV * 64;
  const int n = blockIdx.x;
  const RowLanes L = row_lanes();
  const int sub = L.sub;
  float4 ur[H][CV];
#pragma unroll
  for (int h = 0; h < H; ++h) load_row<CV>(u + ((int64_t)n * H + h) * C + sub * 4, ur[h]);
  HeadVals<H> bias;
#pragma unroll
  for (int h = 0; h < H; ++h) bias.v[h] = add ? add[n * H + h] : 0.f;
  const int m_lo = blockIdx.y * 256;
  const int m_hi = min(m_lo + 256, m_cols);
  for (int m = m_lo + L.first_row(); m < m_hi; m += ROW_STRIDE) {  // the 16 lanes of a row enter and leave together
    float4 e[CV];
    load_row<CV>(emb + ((int64_t)n * m_cols + m) * C + sub * 4, e);
    HeadVals<H> acc;
#pragma unroll
    for (int h = 0; h < H; ++h) acc.v[h] = row_dot<CV>(e, ur[h]);
    reduce16<H>(acc.v);
    if (sub < H) out[((int64_t)sub * n_rows + n) * m_cols + m] = pick<H>(acc, sub) + pick<H>(bias, sub);
  }
}

// ---------------------------------------------------------------- RPE attention, fused (rpe_transformer.py:51-72)
// One workgroup per query row n does the whole attention row for all heads:
//   1. raw scores  s[h][m] = (q[h,n,:] . k[h,m,:] + emb[n,m,:] . u[n,h,:] + add[n,h]) / sqrt(ch)   (16 lanes share one
//      (n, m) pair: float4 loads of the embedding row -- the only N*M*C stream, read exactly once per layer -- and of the
//      key row, xor-shuffle reduction), then attention_factors, key_weights, key_masks exactly in the reference's order;
//   2. softmax over m per head in LDS (wave reductions), written out as attention_scores (H, N, M);
//   3. hidden[n, h*ch + c] = sum_m p[h][m] * v[m, h*ch + c]  (thread = output channel, the value matrix streams from L2).
// Nothing of size N*M*C or H*N*M is re-read from HBM between the steps; the reference materialises the (N, M, C) projected
// embedding, two (H, N, M) score tensors and the softmax in separate ATen kernels.
template <int H, int CV>
__global__ __launch_bounds__(256) void rpe_attention_kernel(const float* __restrict__ emb, const float* __restrict__ u,
                                                            const float* __restrict__ add, const float* __restrict__ q,
                                                            const float* __restrict__ k, const float* __restrict__ v,
                                                            const float* __restrict__ factors,
                                                            const float* __restrict__ key_weights,
                                                            const uint8_t* __restrict__ key_masks, int n_rows, int m_cols,
                                                            float inv_sqrt_ch, float* __restrict__ out_scores,
                                                            float* __restrict__ out_hidden) {
  constexpr int C = CV * 64, CH = C / H;
  extern __shared__ float s_sc[];  // [H][m_cols]
  const int n = blockIdx.x;
  const RowLanes L = row_lanes();
  const int lane = L.lane, w = L.w, sub = L.sub;
  float4 ur[H][CV], qr[CV];
  // q and u[0] chunk by chunk: with one row after the other <1, 4> takes 78 VGPRs instead of 64 and loses two waves per SIMD
  load_row2<CV>(q + (int64_t)n * C + sub * 4, qr, u + (int64_t)n * H * C + sub * 4, ur[0]);
#pragma unroll
  for (int h = 1; h < H; ++h) load_row<CV>(u + ((int64_t)n * H + h) * C + sub * 4, ur[h]);
  // ---- 1. raw scores
  for (int m = L.first_row(); m < m_cols; m += ROW_STRIDE) {
    float4 e[CV], kk[CV];
    load_row2<CV>(emb + ((int64_t)n * m_cols + m) * C + sub * 4, e, k + (int64_t)m * C + sub * 4, kk);
    HeadVals<H> acc;
#pragma unroll
    for (int h = 0; h < H; ++h) acc.v[h] = row_dot<CV>(e, ur[h]);
    head_dot_add<H, CV>(qr, kk, sub, acc.v);  // q . k
    reduce16<H>(acc.v);
    if (sub < H) {
      float sc = (pick<H>(acc, sub) + add[n * H + sub]) * inv_sqrt_ch;
      if (factors) sc = factors[(int64_t)n * m_cols + m] * sc;
      if (key_weights) sc = sc * key_weights[m];
      if (key_masks && key_masks[m]) sc = -INFINITY;
      s_sc[sub * m_cols + m] = sc;
    }
  }
  __syncthreads();
  // ---- 2. softmax over m, one wave per head (two heads per wave when H = 8)
  for (int h = w; h < H; h += 4) {
    float* row = s_sc + h * m_cols;
    float mx = -INFINITY;
    for (int m = lane; m < m_cols; m += 64) mx = fmaxf(mx, row[m]);
    mx = wave_max(mx);
    float sum = 0.f;
    for (int m = lane; m < m_cols; m += 64) {
      const float ev = expf(row[m] - mx);
      row[m] = ev;
      sum += ev;
    }
    sum = wave_sum(sum);
    const float inv = 1.0f / sum;
    float* dst = out_scores + ((int64_t)h * n_rows + n) * m_cols;
    for (int m = lane; m < m_cols; m += 64) {
      const float p = row[m] * inv;
      row[m] = p;
      dst[m] = p;
    }
  }
  __syncthreads();
  // ---- 3. hidden = P V: wave w takes a quarter of the keys, lane l the four channels 4l .. 4l+3 (float4 loads of the
  //         value rows, eight keys in flight), then the four partial rows are added through LDS
  __shared__ float4 s_part[4][64];
  {
    const int per = (m_cols + 3) / 4;
    const int m0 = w * per, m1 = min(m_cols, m0 + per);
    const bool on = lane * 4 < C;
    const float* prow = s_sc + ((lane * 4) / CH) * m_cols;
    const float* vcol = v + lane * 4;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (on) {
      int m = m0;
      for (; m + 8 <= m1; m += 8) {
        float4 vv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) vv[j] = *reinterpret_cast<const float4*>(vcol + (int64_t)(m + j) * C);
#pragma unroll
        for (int j = 0; j < 8; ++j) axpy(prow[m + j], vv[j], acc);
      }
      for (; m < m1; ++m) axpy(prow[m], *reinterpret_cast<const float4*>(vcol + (int64_t)m * C), acc);
    }
    s_part[w][lane] = acc;
    __syncthreads();
    if (w == 0 && on)
      *reinterpret_cast<float4*>(out_hidden + (int64_t)n * C + lane * 4) =
          fold4(s_part[0][lane], s_part[1][lane], s_part[2][lane], s_part[3][lane]);
  }
}

// ---------------------------------------------------------------- backward: two launches and no float atomics
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
  const RowLanes L = row_lanes();
  const int tid = threadIdx.x, lane = L.lane, w = L.w, sub = L.sub, grp = L.grp;
  // ---- 1. dP[h][m] = grad_hidden[n, hb] . v[m, hb] (+ grad_scores): 16 lanes share one key row
  {
    float4 gr4[CV];
    load_row<CV>(grad_hidden + (int64_t)n * C + sub * 4, gr4);
    for (int m = L.first_row(); m < m_cols; m += ROW_STRIDE) {
      float4 vv[CV];
      load_row<CV>(v + (int64_t)m * C + sub * 4, vv);
      HeadVals<H> acc;
#pragma unroll
      for (int h = 0; h < H; ++h) acc.v[h] = 0.f;
      head_dot_add<H, CV>(gr4, vv, sub, acc.v);
      reduce16<H>(acc.v);
      if (sub < H) {
        float val = pick<H>(acc, sub);
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
    dsum = wave_sum(dsum);
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
    asum = wave_sum(asum);
    if (lane == 0) grad_add[n * H + h] = asum;
  }
  __syncthreads();
  // ---- 3. the embedding stream: grad_u and grad_q accumulate per 16-lane group, grad_embed leaves row by row
  float4 au[H][CV], aq[CV], ur[H][CV];
#pragma unroll
  for (int i = 0; i < CV; ++i) {
    aq[i] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int h = 0; h < H; ++h) au[h][i] = ur[h][i] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if (grad_embed) {
#pragma unroll
    for (int h = 0; h < H; ++h) load_row<CV>(u + ((int64_t)n * H + h) * C + sub * 4, ur[h]);
  }
  for (int m = L.first_row(); m < m_cols; m += ROW_STRIDE) {
    const int64_t eoff = ((int64_t)n * m_cols + m) * C + sub * 4;
    float4 e[CV], kk[CV];
    load_row2<CV>(emb + eoff, e, k + (int64_t)m * C + sub * 4, kk);
    HeadVals<H> dzv;
#pragma unroll
    for (int h = 0; h < H; ++h) dzv.v[h] = s_dz[h * m_cols + m];
    const float(&dz)[H] = dzv.v;
#pragma unroll
    for (int i = 0; i < CV; ++i) {
#pragma unroll
      for (int h = 0; h < H; ++h) axpy(dz[h], e[i], au[h][i]);
      axpy(pick<H>(dzv, (i * 64 + sub * 4) / CH), kk[i], aq[i]);
    }
    if (grad_embed) {
#pragma unroll
      for (int i = 0; i < CV; ++i) {
        float4 g = make_float4(dz[0] * ur[0][i].x, dz[0] * ur[0][i].y, dz[0] * ur[0][i].z, dz[0] * ur[0][i].w);
#pragma unroll
        for (int h = 1; h < H; ++h) axpy(dz[h], ur[h][i], g);
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
      const float4 r = fold4(p[j], p[PER + j], p[2 * PER + j], p[3 * PER + j]);
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

// ---------------------------------------------------------------- host side
// the size and shape checks of the three entry points; `name` keeps every message the entry point's own
int rpe_check_shape(const char* name, int64_t n, int64_t m, int64_t c, int64_t heads) {
  GR_REQUIRE(n >= 0 && m >= 0 && n < (1 << 24) && m < (1 << 24), "%s: bad sizes", name);
  GR_REQUIRE((c == 64 || c == 128 || c == 256) && (heads == 1 || heads == 2 || heads == 4 || heads == 8),
             "%s: d_model must be 64/128/256 and num_heads 1/2/4/8 (got %lld, %lld)", name, (long long)c, (long long)heads);
  return GR_OK;
}

// (c, heads), already checked, -> f(integral_constant<H>, integral_constant<CV>): the 12 instantiations of a row kernel
template <class F>
int rpe_dispatch(int64_t c, int64_t heads, F&& f) {
  auto with_cv = [&](auto cv) {
    switch (heads) {
      case 1: return f(std::integral_constant<int, 1>{}, cv);
      case 2: return f(std::integral_constant<int, 2>{}, cv);
      case 4: return f(std::integral_constant<int, 4>{}, cv);
      default: return f(std::integral_constant<int, 8>{}, cv);
    }
  };
  if (c == 64) return with_cv(std::integral_constant<int, 1>{});
  if (c == 128) return with_cv(std::integral_constant<int, 2>{});
  return with_cv(std::integral_constant<int, 4>{});
}

// one workgroup per query row with `lds` bytes of dynamic LDS (forward, row pass of the backward)
template <class... P, class... A>
int rpe_launch_rows(void (*kern)(P...), int64_t n, size_t lds, hipStream_t stream, A... args) {
  if (lds > 64 * 1024)  // what this launch needs: the kernel's static LDS counts against the CU's 160 KB too
    GR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kern, dim3((unsigned)n), dim3(256), lds, stream, static_cast<P>(args)...);
  GR_LAUNCH_CHECK();
  return GR_OK;
}

}  // namespace
}  // namespace gr

using namespace gr;

extern "C" int gr_rpe_scores(const float* embed, const float* u, const float* add, int64_t n, int64_t m, int64_t c,
                             int64_t heads, float* out, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (int rc = rpe_check_shape("rpe_scores", n, m, c, heads)) return rc;
  if (n == 0 || m == 0) return GR_OK;
  GR_REQUIRE(embed && u && out, "null argument");
  const dim3 grid((unsigned)n, (unsigned)((m + 255) / 256));
  KernelTimer timer("rpe_scores", stream);
  return rpe_dispatch(c, heads, [&](auto h, auto cv) {
    hipLaunchKernelGGL((rpe_scores_kernel<decltype(h)::value, decltype(cv)::value>), grid, dim3(256), 0, stream, embed, u, add,
                       (int)n, (int)m, out);
    GR_LAUNCH_CHECK();
    return GR_OK;
  });
}

extern "C" int gr_rpe_attention(const float* embed, const float* u, const float* add, const float* q, const float* k,
                                const float* v, const float* attention_factors, const float* key_weights,
                                const uint8_t* key_masks, int64_t n, int64_t m, int64_t c, int64_t heads, float* out_scores,
                                float* out_hidden, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (int rc = rpe_check_shape("rpe_attention", n, m, c, heads)) return rc;
  if (n == 0) return GR_OK;
  GR_REQUIRE(m > 0, "rpe_attention: no keys (softmax over an empty row)");
  GR_REQUIRE(embed && u && add && q && k && v && out_scores && out_hidden, "null argument");
  const size_t lds = (size_t)heads * m * sizeof(float);
  GR_REQUIRE(lds <= 150 * 1024, "rpe_attention: %lld keys x %lld heads do not fit in LDS", (long long)m, (long long)heads);
  const float inv_sqrt_ch = 1.0f / sqrtf((float)(c / heads));
  KernelTimer timer("rpe_attention", stream);
  return rpe_dispatch(c, heads, [&](auto h, auto cv) {
    return rpe_launch_rows(rpe_attention_kernel<decltype(h)::value, decltype(cv)::value>, n, lds, stream, embed, u, add, q, k,
                           v, attention_factors, key_weights, key_masks, n, m, inv_sqrt_ch, out_scores, out_hidden);
  });
}

extern "C" size_t gr_rpe_attention_backward_workspace_bytes(int64_t n, int64_t m, int64_t heads) {
  if (n < 0 || m < 0 || heads < 0) return 0;
  return align_up((size_t)heads * n * m * sizeof(float), 256) + 256;
}

extern "C" int64_t gr_rpe_attention_backward_max_keys(int64_t c, int64_t heads) {
  if (c <= 0 || heads <= 0) return 0;
  const size_t fixed = 4 * (size_t)(heads + 1) * c * sizeof(float);
  if (fixed >= RPB_LDS_MAX) return 0;
  int64_t m = (int64_t)((RPB_LDS_MAX - fixed) / (sizeof(float) * heads));
  while (m > 0 && rpb_lds_bytes(m, c, heads) > RPB_LDS_MAX) --m;  // the float4 padding of the (H, M) block
  return m;
}

extern "C" int gr_rpe_attention_backward(const float* embed, const float* u, const float* q, const float* k, const float* v,
                                         const float* scores, const float* attention_factors, const float* key_weights,
                                         const float* grad_hidden, const float* grad_scores, int64_t n, int64_t m, int64_t c,
                                         int64_t heads, float* grad_q, float* grad_k, float* grad_v, float* grad_u,
                                         float* grad_add, float* grad_embed, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (int rc = rpe_check_shape("rpe_attention_backward", n, m, c, heads)) return rc;
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
  const size_t lds = rpb_lds_bytes(m, c, heads);
  GR_REQUIRE(lds <= RPB_LDS_MAX, "rpe_attention_backward: %lld keys x %lld heads do not fit in LDS", (long long)m,
             (long long)heads);
  GR_REQUIRE(ws && ws_bytes >= gr_rpe_attention_backward_workspace_bytes(n, m, heads),
             "rpe_attention_backward: workspace too small");
  Carver carve(ws);
  float* dz = carve.take<float>((size_t)heads * n * m);
  const float inv_sqrt_ch = 1.0f / sqrtf((float)(c / heads));
  {
    KernelTimer timer("rpe_attention_backward_rows", stream);
    const int rc = rpe_dispatch(c, heads, [&](auto h, auto cv) {
      return rpe_launch_rows(rpe_bwd_row_kernel<decltype(h)::value, decltype(cv)::value>, n, lds, stream, embed, u, k, v,
                             attention_factors, key_weights, scores, grad_hidden, grad_scores, n, m, inv_sqrt_ch, dz, grad_q,
                             grad_u, grad_add, grad_embed);
    });
    if (rc != GR_OK) return rc;
  }
  {
    KernelTimer timer("rpe_attention_backward_cols", stream);
    const int ch = (int)(c / heads);
    const dim3 grid((unsigned)((ch + GT - 1) / GT), (unsigned)((m + GT - 1) / GT), (unsigned)(2 * heads));
    hipLaunchKernelGGL(rpe_bwd_col_kernel, grid, dim3(256), 0, stream, dz, scores, q, grad_hidden, (int)n, (int)m, (int)c, ch,
                       grad_k, grad_v);
    GR_LAUNCH_CHECK();
  }
  return GR_OK;
}
