// Optimiser step of a Gaussian scene: Adam over up to GR_GS_ADAM_MAX_GROUPS parameter tensors that share
// the leading dimension P, in ONE launch, with optional per-Gaussian visibility, and the densification statistics.
//
// gs_adam_kernel.  Work is per element: a thread owns four consecutive floats of one group, so the seven streams
// (p, g, m, v read; p, m, v written) move as 16-byte accesses whatever K is; the Gaussian an element belongs to is
// element / K with a compile-time K for the six row lengths of a 3DGS scene (a multiply-high) and a runtime division
// otherwise.  The group table is a kernel argument; a workgroup finds its group from the table's workgroup offsets.
// Per element, in fp32, in the association of torch.optim.Adam's own device code (lerp_, addcmul_, addcdiv_), whose
// multiply-adds are fused; the build has -ffp-contract=off, so every fused operation is an explicit fmaf:
//   m = fma(1 - beta1, g - m, m)                       (= beta1 m + (1 - beta1) g; the rounding of beta1 itself, 2.6e-8
//                                                       relative for 0.9, never multiplies the running moment)
//   v = fma(1 - beta2, g * g, beta2 * v)
//   p = fma(-(lr / bc1), m / (sqrt(v) / sqrt(bc2) + eps), p)
// with beta2, 1 - beta, lr / bc1 and sqrt(bc2) formed in double on the host and rounded once.
// An invisible Gaussian costs its visibility lookup and nothing else: a quad whose elements are all invisible is skipped
// before any load, a quad that mixes visible and invisible elements (or is the unaligned / partial tail) goes element by
// element.  No atomics, no LDS, no workspace.
//
// gs_densify_stats_kernel.  One thread per Gaussian, views added in index order.
#include "common.hpp"

namespace gr {
namespace {

constexpr int THREADS = 256;
constexpr int QUAD = 4;                       // floats per thread
constexpr uint32_t ELEMS_PER_BLOCK = THREADS * QUAD;

struct AdamGroup {
  float* p;
  const float* g;
  float* m;
  float* v;
  uint32_t n;       // P * K elements
  uint32_t K;
  uint32_t block0;  // first workgroup of this group
  uint32_t wide;    // all four pointers 16-byte aligned
  float step;       // lr / bc1
  uint32_t pad_;
};

struct AdamTable {
  AdamGroup group[GR_GS_ADAM_MAX_GROUPS];
  int count;
};

struct AdamScalars {
  float one_minus_beta1, beta2, one_minus_beta2, sqrt_bc2, eps;
};

struct Visibility {
  const uint8_t* mask;    // (P) or null
  const int32_t* radii;   // (V, P) or null
  uint32_t P;
  int V;
};

__device__ __forceinline__ bool visible(const Visibility& vis, uint32_t gaussian) {
  if (vis.mask) return vis.mask[gaussian] != 0;
  if (vis.radii) {
    bool any = false;
    for (int v = 0; v < vis.V; ++v) any |= vis.radii[(size_t)v * vis.P + gaussian] > 0;
    return any;
  }
  return true;
}

__device__ __forceinline__ void adam_element(float& p, float g, float& m, float& v, float step, const AdamScalars& s) {
  m = fmaf(s.one_minus_beta1, g - m, m);
  v = fmaf(s.one_minus_beta2, g * g, s.beta2 * v);
  const float denom = sqrtf(v) / s.sqrt_bc2 + s.eps;
  p = fmaf(-step, m / denom, p);
}

// KC > 0: row length known at compile time; KC = 0: G.K at run time
template <uint32_t KC>
__device__ __forceinline__ void adam_quad(const AdamGroup& G, uint32_t e0, const Visibility& vis, const AdamScalars& s) {
  const uint32_t K = KC ? KC : G.K;
  const uint32_t count = min((uint32_t)QUAD, G.n - e0);
  bool vis_e[QUAD];
  bool all = true, any = false;
  uint32_t last = 0xffffffffu;
  bool last_vis = false;
#pragma unroll
  for (int j = 0; j < QUAD; ++j) {
    vis_e[j] = false;
    if ((uint32_t)j < count) {
      const uint32_t gaussian = (e0 + j) / K;
      if (gaussian != last) {
        last = gaussian;
        last_vis = visible(vis, gaussian);
      }
      vis_e[j] = last_vis;
    }
    all &= vis_e[j];
    any |= vis_e[j];
  }
  if (!any) return;
  if (all && G.wide) {  // count == QUAD here: an absent element is never visible
    float4 p = *reinterpret_cast<const float4*>(G.p + e0);
    const float4 g = *reinterpret_cast<const float4*>(G.g + e0);
    float4 m = *reinterpret_cast<const float4*>(G.m + e0);
    float4 v = *reinterpret_cast<const float4*>(G.v + e0);
    adam_element(p.x, g.x, m.x, v.x, G.step, s);
    adam_element(p.y, g.y, m.y, v.y, G.step, s);
    adam_element(p.z, g.z, m.z, v.z, G.step, s);
    adam_element(p.w, g.w, m.w, v.w, G.step, s);
    *reinterpret_cast<float4*>(G.p + e0) = p;
    *reinterpret_cast<float4*>(G.m + e0) = m;
    *reinterpret_cast<float4*>(G.v + e0) = v;
    return;
  }
#pragma unroll
  for (int j = 0; j < QUAD; ++j) {
    if (vis_e[j]) {
      const uint32_t e = e0 + j;
      float p = G.p[e], m = G.m[e], v = G.v[e];
      adam_element(p, G.g[e], m, v, G.step, s);
      G.p[e] = p;
      G.m[e] = m;
      G.v[e] = v;
    }
  }
}

__global__ __launch_bounds__(THREADS) void gs_adam_kernel(AdamTable table, AdamScalars s, Visibility vis) {
  int gi = 0;
  for (int i = 1; i < table.count; ++i) gi = blockIdx.x >= table.group[i].block0 ? i : gi;
  const AdamGroup G = table.group[gi];
  const uint32_t e0 = (blockIdx.x - G.block0) * ELEMS_PER_BLOCK + threadIdx.x * QUAD;
  if (e0 >= G.n) return;
  switch (G.K) {
    case 1: adam_quad<1>(G, e0, vis, s); break;
    case 3: adam_quad<3>(G, e0, vis, s); break;
    case 4: adam_quad<4>(G, e0, vis, s); break;
    case 9: adam_quad<9>(G, e0, vis, s); break;
    case 24: adam_quad<24>(G, e0, vis, s); break;
    case 45: adam_quad<45>(G, e0, vis, s); break;
    default: adam_quad<0>(G, e0, vis, s); break;
  }
}

__global__ __launch_bounds__(THREADS) void gs_densify_stats_kernel(const float* __restrict__ grad2d /*(V, P, 3)*/,
                                                                    const int32_t* __restrict__ radii /*(V, P)*/, int64_t P,
                                                                    int V, float* __restrict__ grad_accum,
                                                                    int32_t* __restrict__ denom, int32_t* __restrict__ max_radii) {
  const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (i >= P) return;
  float acc = 0.f;
  int32_t seen = 0, rmax = 0;
  for (int v = 0; v < V; ++v) {
    const int32_t r = radii[(int64_t)v * P + i];
    if (r > 0) {
      const float* gp = grad2d + ((int64_t)v * P + i) * 3;
      const float gx = gp[0], gy = gp[1];
      const float norm = sqrtf(gx * gx + gy * gy);
      // the first visible view starts from the stored sum, so a batch adds in the order single views would
      acc = seen ? acc + norm : grad_accum[i] + norm;
      rmax = max(rmax, r);
      ++seen;
    }
  }
  if (seen) {
    grad_accum[i] = acc;
    denom[i] += seen;
    max_radii[i] = max(max_radii[i], rmax);
  }
}

}  // namespace
}  // namespace gr

using namespace gr;

extern "C" int gr_gs_adam_step(const gr_gs_adam_group* groups, int n_groups, int64_t P, double beta1, double beta2, double eps,
                               double bias_correction1, double bias_correction2, const uint8_t* visible_mask,
                               const int32_t* radii, int V, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  GR_REQUIRE(n_groups >= 0 && n_groups <= GR_GS_ADAM_MAX_GROUPS && (groups || n_groups == 0),
             "gs adam: %d groups (at most %d per call)", n_groups, GR_GS_ADAM_MAX_GROUPS);
  GR_REQUIRE(P >= 0 && P < (1ll << 31), "gs adam: P = %lld outside [0, 2^31)", (long long)P);
  GR_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0, "gs adam: betas (%g, %g) or eps %g invalid",
             beta1, beta2, eps);
  GR_REQUIRE(bias_correction1 > 0.0 && bias_correction2 > 0.0, "gs adam: bias corrections (%g, %g) must be positive",
             bias_correction1, bias_correction2);
  GR_REQUIRE(!(visible_mask && radii), "gs adam: give a byte mask or radii, not both");
  GR_REQUIRE(!radii || V >= 1, "gs adam: radii need V >= 1 (got %d)", V);
  AdamTable table;
  memset(&table, 0, sizeof table);
  uint64_t blocks = 0;
  for (int i = 0; i < n_groups; ++i) {
    const gr_gs_adam_group& in = groups[i];
    GR_REQUIRE(in.K >= 0, "gs adam: group %d has K = %d", i, in.K);
    if (in.K == 0 || !in.grad || P == 0) continue;  // empty f_rest at SH degree 0; a parameter without a gradient
    GR_REQUIRE(in.param && in.exp_avg && in.exp_avg_sq, "gs adam: group %d has a null param or moment pointer", i);
    const int64_t n = P * in.K;
    // 32-bit element indices: the last quad may start at n - 1 and index up to n + 2
    GR_REQUIRE(n <= 0xffffffffll - QUAD, "gs adam: group %d has P * K = %lld elements, more than the 32-bit element index holds",
               i, (long long)n);
    AdamGroup& G = table.group[table.count++];
    G.p = in.param;
    G.g = in.grad;
    G.m = in.exp_avg;
    G.v = in.exp_avg_sq;
    G.n = (uint32_t)n;
    G.K = (uint32_t)in.K;
    G.block0 = (uint32_t)blocks;
    G.wide = (((uintptr_t)in.param | (uintptr_t)in.grad | (uintptr_t)in.exp_avg | (uintptr_t)in.exp_avg_sq) & 15) == 0;
    G.step = (float)(in.lr / bias_correction1);
    blocks += ((uint64_t)n + ELEMS_PER_BLOCK - 1) / ELEMS_PER_BLOCK;
  }
  GR_REQUIRE(blocks < (1ull << 31), "gs adam: %llu workgroups exceed one launch", (unsigned long long)blocks);
  if (blocks == 0) return GR_OK;
  AdamScalars s;
  s.one_minus_beta1 = (float)(1.0 - beta1);
  s.beta2 = (float)beta2;
  s.one_minus_beta2 = (float)(1.0 - beta2);
  s.sqrt_bc2 = (float)sqrt(bias_correction2);
  s.eps = (float)eps;
  Visibility vis;
  vis.mask = visible_mask;
  vis.radii = radii;
  vis.P = (uint32_t)P;
  vis.V = radii ? V : 0;
  KernelTimer timer("gs_adam_step", stream);
  hipLaunchKernelGGL(gs_adam_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, stream, table, s, vis);
  GR_LAUNCH_CHECK();
  return GR_OK;
}

extern "C" int gr_gs_densify_stats(const float* means2D_grad, const int32_t* radii, int64_t P, int V, float* grad_accum,
                                   int32_t* denom, int32_t* max_radii, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  GR_REQUIRE(P >= 0 && V >= 0, "gs densify stats: P = %lld, V = %d", (long long)P, V);
  if (P == 0 || V == 0) return GR_OK;
  GR_REQUIRE(means2D_grad && radii && grad_accum && denom && max_radii, "gs densify stats: null argument");
  const int64_t blocks = (P + THREADS - 1) / THREADS;
  GR_REQUIRE(blocks < (1ll << 31), "gs densify stats: P = %lld exceeds one launch", (long long)P);
  KernelTimer timer("gs_densify_stats", stream);
  hipLaunchKernelGGL(gs_densify_stats_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, stream, means2D_grad, radii, P, V, grad_accum,
                     denom, max_radii);
  GR_LAUNCH_CHECK();
  return GR_OK;
}
