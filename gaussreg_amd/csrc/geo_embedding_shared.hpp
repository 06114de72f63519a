// Device code that the structure embedding's forward (geo_embedding.hip) and backward (geo_embedding_backward.hip) share,
// so that the backward walks the forward's pairs with the forward's own arithmetic: distances and neighbour sets
// (sq_dist_ref, geo_knn_kernel), the per-pair embedding indices (ge_pair_indices), the function-table evaluation
// (ft_eval, ft_direct) and the split-bf16 kernel's sincos_moderate.  Device-only; every translation unit gets its own copy.
#pragma once
#include "common.hpp"

namespace gr {
namespace {

constexpr int GE_ROWS = 128;  // (n,m) pairs per workgroup
constexpr int GE_KMAX = 8;    // angle_k <= 8

__device__ __forceinline__ float sq_dist_ref(const float3 a, float a2, const float3 b, float b2) {
  // pairwise_distance.py:21-31: xy by matmul, then (x2 - 2 xy) + y2, clamped at 0
  const float xy = fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x));
  return fmaxf((a2 - 2.0f * xy) + b2, 0.0f);
}
__device__ __forceinline__ float3 ld3(const float* p, int i) { return make_float3(p[3 * i], p[3 * i + 1], p[3 * i + 2]); }
__device__ __forceinline__ float norm2(const float3 a) { return (a.x * a.x + a.y * a.y) + a.z * a.z; }


// k nearest other points per point: geotransformer.py:42 topk(k+1, largest=False)[1][:, :, 1:]
// (ascending distance, the first -- the point itself -- dropped; ties: lowest index first).  One wave per point.
__global__ __launch_bounds__(256) void geo_knn_kernel(const float* __restrict__ pts, int n, int k,
                                                      int32_t* __restrict__ knn) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= n) return;
  const float3 p = ld3(pts, row);
  const float p2 = norm2(p);
  unsigned long long best[GE_KMAX + 1];
#pragma unroll
  for (int i = 0; i <= GE_KMAX; ++i) best[i] = ~0ull;
  for (int m = lane; m < n; m += 64) {
    const float3 q = ld3(pts, m);
    const float d = sqrtf(sq_dist_ref(p, p2, q, norm2(q)));
    unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)m;
#pragma unroll
    for (int i = 0; i <= GE_KMAX; ++i) {  // sorted insertion (register-resident)
      const unsigned long long lo = key < best[i] ? key : best[i];
      key = key < best[i] ? best[i] : key;
      best[i] = lo;
    }
  }
  for (int s = 0; s <= k; ++s) {
    unsigned long long v = best[0];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      const unsigned long long o = __shfl_xor(v, d, 64);
      v = o < v ? o : v;
    }
    if (best[0] == v) {  // the owner pops (keys are unique: they carry the index)
#pragma unroll
      for (int i = 0; i < GE_KMAX; ++i) best[i] = best[i + 1];
      best[GE_KMAX] = ~0ull;
    }
    if (s > 0 && lane == 0) knn[row * k + (s - 1)] = v == ~0ull ? row : (int)(unsigned)(v & 0xffffffffull);
  }
}

// per-pair embedding indices (geotransformer.py:38-55) for the GE_ROWS consecutive (a, b) pairs of a workgroup:
// xs[0..k-1][row] = angular indices, xs[k][row] = distance index
__device__ __forceinline__ void ge_pair_indices(const float* __restrict__ pts, int n, const int32_t* __restrict__ knn,
                                                int k, float sigma_d, float factor_a, int64_t r0, int64_t total, int tid,
                                                float (*xs)[GE_ROWS]) {
  if (tid < GE_ROWS) {
    const int64_t r = r0 + tid;
    float xd = 0.f, xa[GE_KMAX];
#pragma unroll
    for (int i = 0; i < GE_KMAX; ++i) xa[i] = 0.f;
    if (r < total) {
      const int a = (int)(r / n), b = (int)(r - (int64_t)a * n);
      const float3 pa = ld3(pts, a), pb = ld3(pts, b);
      xd = sqrtf(sq_dist_ref(pa, norm2(pa), pb, norm2(pb))) / sigma_d;
      const float3 anc = make_float3(pb.x - pa.x, pb.y - pa.y, pb.z - pa.z);
#pragma unroll
      for (int i = 0; i < GE_KMAX; ++i)
        if (i < k) {
          const float3 pk = ld3(pts, knn[a * k + i]);
          const float3 ref = make_float3(pk.x - pa.x, pk.y - pa.y, pk.z - pa.z);
          const float3 cr = make_float3(ref.y * anc.z - ref.z * anc.y, ref.z * anc.x - ref.x * anc.z,
                                        ref.x * anc.y - ref.y * anc.x);
          const float sn = sqrtf(norm2(cr));
          // torch.sum accumulates from +0: an all-(-0) product row (a == b, anc = +0) must give +0, not -0 (atan2 -> pi)
          const float cs = ((0.0f + ref.x * anc.x) + ref.y * anc.y) + ref.z * anc.z;
          xa[i] = atan2f(sn, cs) * factor_a;
        }
    }
#pragma unroll
    for (int i = 0; i < GE_KMAX; ++i)
      if (i < k) xs[i][tid] = xa[i];
    xs[k][tid] = xd;
  }
}

// sin and cos for moderate arguments (|x| < 2^11; the embedding's index * div_term is a few tens): three-constant
// Cody-Waite reduction by pi/2 and the Cephes single-precision polynomials on [-pi/4, pi/4] (~1 ulp).  Used by the
// split-bf16 kernel, where the operand generation competes with a 2.7x faster matrix pipe; workgroups that see a larger
// index (or a non-finite one) use the library sincosf().
__device__ __forceinline__ void sincos_moderate(float x, float* sn, float* cs) {
  const float kf = rintf(x * 0.636619772367581343f);  // 2/pi
  float r = fmaf(kf, -1.5703125f, x);                   // pi/2 = 1.5703125 + 4.837512969970703125e-4 + 7.54978995489188e-8
  r = fmaf(kf, -4.837512969970703125e-4f, r);
  r = fmaf(kf, -7.54978995489188e-8f, r);
  const float r2 = r * r;
  float ps = -1.9515295891e-4f;
  ps = fmaf(ps, r2, 8.3321608736e-3f);
  ps = fmaf(ps, r2, -1.6666654611e-1f);
  const float s = fmaf(ps * r2, r, r);
  float pc = 2.443315711809948e-5f;
  pc = fmaf(pc, r2, -1.388731625493765e-3f);
  pc = fmaf(pc, r2, 4.166664568298827e-2f);
  const float c = fmaf(pc * r2, r2, fmaf(-0.5f, r2, 1.0f));
  const int q = (int)kf;
  const float s1 = (q & 1) ? c : s, c1 = (q & 1) ? s : c;
  *sn = (q & 2) ? -s1 : s1;
  *cs = ((q + 1) & 2) ? -c1 : c1;
}

__device__ __forceinline__ float4 ft_direct(const float* __restrict__ w, const float* __restrict__ b,
                                             const float* __restrict__ div_term, int C, int ch, float x) {
  float acc[4] = {b[ch], b[ch + 1], b[ch + 2], b[ch + 3]};
  for (int i = 0; i < C / 2; ++i) {
    const float om = x * div_term[i];
    const float sn = sinf(om), cs = cosf(om);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = fmaf(w[(int64_t)(ch + j) * C + 2 * i + 1], cs, fmaf(w[(int64_t)(ch + j) * C + 2 * i], sn, acc[j]));
  }
  return make_float4(acc[0], acc[1], acc[2], acc[3]);
}

__device__ __forceinline__ float4 ft_eval(const float4* __restrict__ tab, int rows, int c4, int cg, float inv_h, float x,
                                          const float* __restrict__ w, const float* __restrict__ b,
                                          const float* __restrict__ div_term) {
  const float m = floorf(x * inv_h);
  const float t = fmaf(x, inv_h, -m);  // one rounding: the position inside the cell keeps full precision
  if (!(m >= 0.0f) || !(m + 3.0f <= (float)(rows - 1))) return ft_direct(w, b, div_term, 4 * c4, 4 * cg, x);  // wave-uniform
  const float4* r = tab + (int64_t)(int)m * c4 + cg;
  const float4 v0 = r[0], v1 = r[c4], v2 = r[2 * c4], v3 = r[3 * c4];
  const float tm1 = t - 1.0f, tm2 = t - 2.0f, tp1 = t + 1.0f;
  const float w0 = -t * tm1 * tm2 * (1.0f / 6.0f), w1 = tp1 * tm1 * tm2 * 0.5f, w2 = -tp1 * t * tm2 * 0.5f,
              w3 = tp1 * t * tm1 * (1.0f / 6.0f);
  return make_float4(fmaf(w3, v3.x, fmaf(w2, v2.x, fmaf(w1, v1.x, w0 * v0.x))), fmaf(w3, v3.y, fmaf(w2, v2.y, fmaf(w1, v1.y, w0 * v0.y))),
                     fmaf(w3, v3.z, fmaf(w2, v2.z, fmaf(w1, v1.z, w0 * v0.z))), fmaf(w3, v3.w, fmaf(w2, v2.w, fmaf(w1, v1.w, w0 * v0.w))));
}

}  // namespace
}  // namespace gr
