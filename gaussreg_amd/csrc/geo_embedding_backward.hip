// GeometricStructureEmbedding backward: the gradients of proj_d / proj_a for one cloud (include/gaussreg_hip_train.h).
//   out[r, :] = W_d phi(xd_r) + b_d + red_i (W_a phi(xa_{r,i}) + b_a),   r = (a, b) over the N^2 pairs
//   grad_W_d[c, j] = sum_r go[r, c] phi_j(xd_r)                       -- a (C x N^2) . (N^2 x C) product whose B operand is
//   mean: grad_W_a[c, j] = sum_r go[r, c] (1/k) sum_i phi_j(xa_{r,i})    generated on the fly, as the forward generates its A
//   max:  grad_W_a[c, j] = sum_i sum_r [win(r, c) = i] go[r, c] phi_j(xa_{r,i})   -- k products, go masked by the winner
//   grad_b_d[c] = grad_b_a[c] = sum_r go[r, c]
// Launch 1 is the forward's geo_knn_kernel, and the pairs' indices come from the forward's ge_pair_indices
// (geo_embedding_shared.hpp): the backward differentiates the function the forward evaluated, neighbour sets included.
// Launch 2, geo_embedding_backward_kernel: a workgroup owns a slab of consecutive pairs (the reduction index: the MFMA's k),
// GB_CT rows c and GB_JT columns j of the two gradients.  Per 32 pairs it stages go[r, c-tile] (float4 reads of the rows)
// transposed into LDS, generates the sinusoid rows into LDS with the forward fp32 kernel's expression
// (sincosf(x * div_term[f]), (sin, cos) interleaved) and accumulates on v_mfma_f32_32x32x2_f32 through mfma_slab.  The
// 'max' winners are re-derived from the F_a table by ft_eval -- the forward table kernel's expression in the forward's
// order, the lowest i among equal values.  The column sums of go ride on the staging pass.  Every workgroup writes its
// partial tiles to the workspace; launch 3 adds them in ascending slab order (no float atomics; slab boundaries depend on
// the shapes only, so two runs leave the same bits) and writes the four gradients or adds into them.
// phi is regenerated once per c-tile (C / GB_CT times) and go re-read once per j-tile (C / GB_JT times): at C = 256 the
// sincos VALU time and the MFMA time of a workgroup are comparable, and several workgroups per CU overlap the two pipes.
#include <algorithm>

#include "common.hpp"
#include "mfma_tile.hpp"
#include "geo_embedding_shared.hpp"
#include "../../include/gaussreg_hip_train.h"

namespace gr {
namespace {

constexpr int GB_CT = 64;    // rows c of a workgroup's tile of grad_W
constexpr int GB_JT = 128;   // columns j of it
constexpr int GB_K = 32;     // pairs per MFMA slab
constexpr int GB_LD = GB_K + 1;
constexpr int GB_T = 256;    // 2 x 2 waves of 32 x 64
constexpr int64_t GB_SLAB_PAIRS_MAX = 8192;  // the longest fp32 accumulation chain of a workgroup (6 144 at the demo size) ...
constexpr int64_t GB_SLABS_MAX = 1024;       // ... until the partials would outgrow this many slabs (n > 2896)
constexpr int64_t GB_TARGET_WG = 768;        // three workgroups per CU (256 CUs), all resident at 3 waves per SIMD
static_assert(GE_ROWS % GB_K == 0, "a chunk of ge_pair_indices is a whole number of MFMA slabs");

struct GebPlan {
  int64_t slabs, pairs_per_slab, c_tiles, j_tiles;
};

// depends on the shapes only
GebPlan geb_plan(int64_t n, int64_t c) {
  GebPlan p;
  p.c_tiles = (c + GB_CT - 1) / GB_CT;
  p.j_tiles = (c + GB_JT - 1) / GB_JT;
  const int64_t total = n * n;
  const int64_t want = std::max<int64_t>(1, GB_TARGET_WG / (p.c_tiles * p.j_tiles));
  int64_t pps = (total + want - 1) / want;
  pps = std::min(pps, GB_SLAB_PAIRS_MAX);
  pps = std::max(pps, (total + GB_SLABS_MAX - 1) / GB_SLABS_MAX);
  pps = std::max<int64_t>(GB_K, (pps + GB_K - 1) / GB_K * GB_K);  // a multiple of 32; at small n: many slabs of 32
  p.pairs_per_slab = pps;
  p.slabs = std::max<int64_t>(1, (total + pps - 1) / pps);
  return p;
}

// MODE 0: angle_k == 0, 1: mean, 2: max
template <int MODE>
__global__ __launch_bounds__(GB_T, 3) void geo_embedding_backward_kernel(
    const float* __restrict__ pts, int n, const int32_t* __restrict__ knn, int k, const float* __restrict__ go,
    const float4* __restrict__ tab_a, int rows_a, float inv_h, const float* __restrict__ w_a, const float* __restrict__ b_a,
    const float* __restrict__ div_term, int C, float sigma_d, float factor_a, int pairs_per_slab,
    float* __restrict__ part, float* __restrict__ bias_part) {
  __shared__ float sa[GB_CT][GB_LD];  // go[r, c-tile] transposed (masked by the winner for 'max'): [c][r]
  __shared__ float sb[GB_JT][GB_LD];  // phi_j(x_r): [j][r]
  __shared__ float xs[GE_KMAX + 1][GE_ROWS];
  constexpr int mode = MODE;
  const int s0 = blockIdx.x * pairs_per_slab, s1 = min(s0 + pairs_per_slab, n * n);  // fits: the host checks n < 46341
  const int c0 = blockIdx.y * GB_CT, j0 = blockIdx.z * GB_JT;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wi = (w >> 1) * 32, wj = (w & 1) * 64;
  const bool live = c0 + wi < C && j0 + wj < C;  // wave-uniform: a wave whose block lies outside the outputs skips the MFMAs
  const int c4 = C / 4;
  const int cg = tid & 15, gc = c0 + 4 * cg;     // the four channels this thread stages
  const float inv_k = k > 0 ? 1.0f / (float)k : 0.f;

  f32x16 accd[1][2], acca[1][2];
  mfma_zero(accd);
  mfma_zero(acca);
  float4 bsum = make_float4(0.f, 0.f, 0.f, 0.f);

  // phi rows of one index plane into sb: 32 pairs x 64 frequencies, 8 (pair, frequency) per thread
  auto gen = [&](int plane, int xr0, bool sum_k) {
#pragma unroll 1
    for (int u = 0; u < GB_K * (GB_JT / 2) / GB_T; ++u) {
      const int e = tid + u * GB_T;
      const int r = e & (GB_K - 1), f = e / GB_K;
      const int gj = j0 + 2 * f;
      float sn = 0.f, cs = 0.f;
      if (gj < C) {
        const float dv = div_term[gj >> 1];
        if (sum_k) {
#pragma unroll 1
          for (int i = 0; i < k; ++i) {
            float s1_, c1_;
            sincosf(xs[i][xr0 + r] * dv, &s1_, &c1_);
            sn += s1_;
            cs += c1_;
          }
          sn *= inv_k;
          cs *= inv_k;
        } else {
          sincosf(xs[plane][xr0 + r] * dv, &sn, &cs);  // positional_embedding.py:27, as geo_embedding_kernel
        }
      }
      sb[2 * f][r] = sn;  // positional_embedding.py:30-31: (sin, cos) interleaved
      sb[2 * f + 1][r] = cs;
    }
  };

  for (int rc = s0; rc < s1; rc += GE_ROWS) {
    // pairs past the slab get index 0 (their go is staged as 0).  (Every phase below ends in a barrier.)
    ge_pair_indices(pts, n, knn, k, sigma_d, factor_a, rc, s1, tid, xs);
    __syncthreads();
    for (int sub = 0; sub < GE_ROWS / GB_K; ++sub) {
      const int rs = rc + sub * GB_K;
      if (rs >= s1) break;
      const int xr0 = sub * GB_K;
      // ---- go[rs .. rs + 32, c-tile]: two float4 per thread; rows past the slab are zeros
      float4 g[2];
      unsigned win = 0;  // 'max': the winner of each of the 8 staged entries, 4 bits each
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int r = (tid >> 4) + 16 * u;
        const int gr = rs + r;
        const bool ok = gr < s1 && gc < C;
        g[u] = ok ? *reinterpret_cast<const float4*>(go + (int64_t)gr * C + gc) : make_float4(0.f, 0.f, 0.f, 0.f);
        bsum.x += g[u].x, bsum.y += g[u].y, bsum.z += g[u].z, bsum.w += g[u].w;
        if (mode == 2 && ok) {
          float4 best = make_float4(0.f, 0.f, 0.f, 0.f);
          unsigned wx = 0, wy = 0, wz = 0, ww = 0;
#pragma unroll 1
          for (int i = 0; i < k; ++i) {  // geo_embedding_table_kernel's order; strict >: the lowest i among equals wins
            const float4 v = ft_eval(tab_a, rows_a, c4, gc >> 2, inv_h, xs[i][xr0 + r], w_a, b_a, div_term);
            if (i == 0 || v.x > best.x) best.x = v.x, wx = i;
            if (i == 0 || v.y > best.y) best.y = v.y, wy = i;
            if (i == 0 || v.z > best.z) best.z = v.z, wz = i;
            if (i == 0 || v.w > best.w) best.w = v.w, ww = i;
          }
          win |= (wx | (wy << 4) | (wz << 8) | (ww << 12)) << (16 * u);
        }
      }
      auto stage_go = [&](int only) {  // only < 0: go itself; else go where the winner is `only`
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int r = (tid >> 4) + 16 * u;
          const unsigned wn = win >> (16 * u);
          const float4 v = g[u];
          sa[4 * cg + 0][r] = only < 0 || (int)(wn & 15u) == only ? v.x : 0.f;
          sa[4 * cg + 1][r] = only < 0 || (int)((wn >> 4) & 15u) == only ? v.y : 0.f;
          sa[4 * cg + 2][r] = only < 0 || (int)((wn >> 8) & 15u) == only ? v.z : 0.f;
          sa[4 * cg + 3][r] = only < 0 || (int)((wn >> 12) & 15u) == only ? v.w : 0.f;
        }
      };
      // ---- grad_W_d (plane k, go itself).  Every phase ends in a barrier.
      stage_go(-1);
      gen(k, xr0, false);
      __syncthreads();
      if (live) mfma_slab<GB_K>(accd, sa, sb, wi, wj, lane);
      __syncthreads();
      // ---- grad_W_a: one phase with the mean of the k sinusoid rows (sa still holds go), or k phases with go masked by
      //      the winner
      const int phases = mode == 1 ? 1 : mode == 2 ? k : 0;
#pragma unroll 1
      for (int ph = 0; ph < phases; ++ph) {
        if (mode == 2) stage_go(ph);
        gen(ph, xr0, mode == 1);
        __syncthreads();
        if (live) mfma_slab<GB_K>(acca, sa, sb, wi, wj, lane);
        __syncthreads();
      }
    }
  }

  // ---- the partial tiles of this slab
  if (live) {
    float* pd = part + (int64_t)blockIdx.x * 2 * C * C;
    float* pa = pd + (int64_t)C * C;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int gj = mfma_col(j0 + wj + 32 * b, lane);
      if (gj >= C) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int gi = mfma_row(c0 + wi, r, lane);
        if (gi < C) {
          pd[(int64_t)gi * C + gj] = accd[0][b][r];
          if (mode != 0) pa[(int64_t)gi * C + gj] = acca[0][b][r];
        }
      }
    }
  }
  // ---- column sums of go over the slab: the 16 threads that staged a channel, in ascending order (the j-tile 0 workgroups)
  if (blockIdx.z == 0) {
    float* red = &sb[0][0];  // free: the last phase ended in a barrier
    red[(tid >> 4) * GB_CT + 4 * cg + 0] = bsum.x;
    red[(tid >> 4) * GB_CT + 4 * cg + 1] = bsum.y;
    red[(tid >> 4) * GB_CT + 4 * cg + 2] = bsum.z;
    red[(tid >> 4) * GB_CT + 4 * cg + 3] = bsum.w;
    __syncthreads();
    if (tid < GB_CT && c0 + tid < C) {
      float s = 0.f;
      for (int t = 0; t < GB_T / 16; ++t) s += red[t * GB_CT + tid];
      bias_part[(int64_t)blockIdx.x * C + c0 + tid] = s;
    }
  }
}

// out = (accumulate ? out : 0) + the partials in ascending slab order; one thread per element of (grad_W_d, grad_W_a, bias)
__global__ __launch_bounds__(256) void geo_embedding_backward_reduce_kernel(
    const float* __restrict__ part, const float* __restrict__ bias_part, int slabs, int C, int has_a, int accumulate,
    float* __restrict__ gwd, float* __restrict__ gbd, float* __restrict__ gwa, float* __restrict__ gba) {
  const int64_t cc = (int64_t)C * C;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= 2 * cc + C) return;
  if (idx < 2 * cc) {
    float* out = idx < cc ? gwd + idx : (gwa ? gwa + (idx - cc) : nullptr);
    if (!out) return;
    float s = 0.f;
    if (idx < cc || has_a)
      for (int sl = 0; sl < slabs; ++sl) s += part[(int64_t)sl * 2 * cc + idx];
    else if (accumulate)
      return;
    *out = accumulate ? *out + s : s;
  } else {
    const int c = (int)(idx - 2 * cc);
    float s = 0.f;
    for (int sl = 0; sl < slabs; ++sl) s += bias_part[(int64_t)sl * C + c];
    gbd[c] = accumulate ? gbd[c] + s : s;
    if (gba) {
      if (has_a) gba[c] = accumulate ? gba[c] + s : s;  // one winner per entry; the mean's weights sum to 1
      else if (!accumulate) gba[c] = 0.f;
    }
  }
}

int geb_check_shape(int64_t n, int64_t c, int64_t angle_k) {
  GR_REQUIRE(n >= 0 && n < 46341, "geo_embedding: n*n must fit int32 pair ids per row (n=%lld)", (long long)n);
  GR_REQUIRE(c > 0 && c % 32 == 0, "geo_embedding_backward: hidden_dim must be a positive multiple of 32 (got %lld)", (long long)c);
  GR_REQUIRE(angle_k >= 0 && angle_k <= GE_KMAX, "geo_embedding: angle_k must be in [0, %d]", GE_KMAX);
  GR_REQUIRE(angle_k < n || n == 0, "geo_embedding: angle_k (%lld) needs more than %lld points", (long long)angle_k, (long long)n);
  return GR_OK;
}

}  // namespace
}  // namespace gr

using namespace gr;

extern "C" size_t gr_geo_embedding_backward_workspace_bytes(int64_t n, int64_t c, int64_t angle_k) {
  if (geb_check_shape(n, c, angle_k) != GR_OK) return 0;  // 0: a shape the call refuses
  const GebPlan p = geb_plan(n, c);
  return align_up((size_t)n * (size_t)std::max<int64_t>(angle_k, 1) * 4, 256) +
         align_up((size_t)p.slabs * 2 * (size_t)c * (size_t)c * 4, 256) + align_up((size_t)p.slabs * (size_t)c * 4, 256) + 256;
}

extern "C" int gr_geo_embedding_backward_plan(int64_t n, int64_t c, int64_t angle_k, int64_t* slabs, int64_t* pairs_per_slab,
                                              int64_t* c_tiles) {
  if (int rc = geb_check_shape(n, c, angle_k)) return rc;
  const GebPlan p = geb_plan(n, c);
  if (slabs) *slabs = p.slabs;
  if (pairs_per_slab) *pairs_per_slab = p.pairs_per_slab;
  if (c_tiles) *c_tiles = p.c_tiles;
  return GR_OK;
}

extern "C" int gr_geo_embedding_backward(const float* points, int64_t n, const float* grad_out, const float* tab_a,
                                         int64_t rows_a, float inv_h, const float* w_a, const float* b_a,
                                         const float* div_term, int64_t c, float sigma_d, float factor_a, int64_t angle_k,
                                         int reduction_mean, int accumulate, float* grad_w_d, float* grad_b_d, float* grad_w_a,
                                         float* grad_b_a, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (int rc = geb_check_shape(n, c, angle_k)) return rc;
  const int mode = angle_k == 0 ? 0 : ((reduction_mean & 1) ? 1 : 2);
  GR_REQUIRE(grad_w_d && grad_b_d && (angle_k == 0 || (grad_w_a && grad_b_a)), "geo_embedding_backward: null gradient");
  if (n == 0) {
    if (!accumulate) {
      GR_HIP(hipMemsetAsync(grad_w_d, 0, (size_t)c * c * 4, stream));
      GR_HIP(hipMemsetAsync(grad_b_d, 0, (size_t)c * 4, stream));
      if (grad_w_a) GR_HIP(hipMemsetAsync(grad_w_a, 0, (size_t)c * c * 4, stream));
      if (grad_b_a) GR_HIP(hipMemsetAsync(grad_b_a, 0, (size_t)c * 4, stream));
    }
    return GR_OK;
  }
  GR_REQUIRE(points && grad_out && div_term, "null argument");
  GR_REQUIRE(reinterpret_cast<uintptr_t>(grad_out) % 16 == 0, "geo_embedding_backward: grad_out must be 16-byte aligned");
  if (mode == 2) {
    GR_REQUIRE(tab_a && w_a && b_a, "geo_embedding_backward: reduction 'max' needs the F_a table and proj_a");
    GR_REQUIRE(rows_a >= 4 && inv_h > 0.0f, "geo_embedding_backward: bad table");
    GR_REQUIRE(reinterpret_cast<uintptr_t>(tab_a) % 16 == 0, "geo_embedding_backward: the table must be 16-byte aligned");
  }
  if (!ws || ws_bytes < gr_geo_embedding_backward_workspace_bytes(n, c, angle_k)) {
    set_error("geo_embedding_backward workspace too small");
    return GR_ERR_WORKSPACE;
  }
  // every refusal comes before the first launch
  const GebPlan p = geb_plan(n, c);
  Carver cv(ws);
  int32_t* knn = cv.take<int32_t>((size_t)n * std::max<int64_t>(angle_k, 1));
  float* part = cv.take<float>((size_t)p.slabs * 2 * c * c);
  float* bias_part = cv.take<float>((size_t)p.slabs * c);
  if (angle_k > 0)
    hipLaunchKernelGGL(geo_knn_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream, points, (int)n, (int)angle_k, knn);
  {
    KernelTimer timer("geo_embedding_backward", stream);
    const dim3 grid((unsigned)p.slabs, (unsigned)p.c_tiles, (unsigned)p.j_tiles);
#define GR_GEB(MODE)                                                                                                          \
  hipLaunchKernelGGL(geo_embedding_backward_kernel<MODE>, grid, dim3(GB_T), 0, stream, points, (int)n, knn, (int)angle_k,     \
                     grad_out, reinterpret_cast<const float4*>(tab_a), (int)rows_a, inv_h, w_a, b_a, div_term, (int)c, sigma_d, \
                     factor_a, (int)p.pairs_per_slab, part, bias_part)
    if (mode == 0) GR_GEB(0);
    else if (mode == 1) GR_GEB(1);
    else GR_GEB(2);
#undef GR_GEB
    const int64_t elems = 2 * c * c + c;
    hipLaunchKernelGGL(geo_embedding_backward_reduce_kernel, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, stream, part,
                       bias_part, (int)p.slabs, (int)c, mode != 0 ? 1 : 0, accumulate ? 1 : 0, grad_w_d, grad_b_d, grad_w_a,
                       grad_b_a);
  }
  GR_LAUNCH_CHECK();
  return GR_OK;
}
