// Densification of a Gaussian scene: upstream 3DGS's densify_and_prune (clone, split into two children,
// prune) as one classification pass and one gather pass.
//
// Plan, three launches, no atomics:
//   gs_densify_classify_kernel  one thread per Gaussian: the three emission flags (original kept, clone, children) from
//                               scaling, opacity and the statistics, in fp32; a byte of flags per Gaussian and the three
//                               sums of every workgroup of 256 Gaussians;
//   gs_densify_scan_kernel      ONE workgroup turns the per-workgroup sums into exclusive prefixes, 256 workgroups a
//                               round with a running carry, and leaves the four block counts {A, B, C, C};
//   gs_densify_scatter_kernel   one thread per Gaussian: its rank inside the workgroup (lane prefix on the DPP network,
//                               wave prefixes through 4 LDS words) plus the workgroup's prefix gives the destination rows
//                               original scanA[i], clone A + scanB[i], child k A + B + k C + scanC[i]; writes source, kind.
// Every prefix is a sum of integers in a fixed tree, so source and kind do not depend on scheduling.
//
// Apply, gs_densify_apply_kernel: output-centric, per element, the group table by value as in gs_adam_kernel.  A thread
// owns four consecutive output floats of one tensor (the parameter or one of the two moments of a group), finds their
// rows by the compile-time row-length divisions of gs_adam_kernel, and copies from row source[row] of the old tensor.
// The destination quad is 16-byte aligned whenever the new tensor is; a gathered source row rarely is, so a quad that
// lies inside one row is fetched with one 16-byte load that assumes 4-byte alignment only (the hardware takes a dwordx4
// at any dword address), a quad that crosses rows element by element.  Moments of new rows (kind != 0) are zeros and read
// nothing.  scaling and xyz of children are computed: scaling' = log(exp(scaling) / 1.6),
// xyz' = xyz + R(q / |q|) (exp(scaling) o noise[source][k]).  No LDS, no atomics.
#include "common.hpp"

namespace gr {
namespace {

constexpr int THREADS = 256;
constexpr int QUAD = 4;
constexpr uint32_t ELEMS_PER_BLOCK = THREADS * QUAD;
constexpr int WAVES = THREADS / WAVE;

constexpr uint32_t FLAG_KEEP = 1, FLAG_CLONE = 2, FLAG_CHILDREN = 4;
constexpr float SPLIT_SHRINK = 1.6f;  // upstream's 0.8 * N with N = 2 children

struct PlanScalars {
  float max_grad, min_opacity, dense_limit /*percent_dense * extent*/, world_limit /*0.1 * extent*/, max_screen_size;
  int screen;  // max_screen_size given
};

// three counts of at most 256 each in one word, so that one scan serves all three
__device__ __forceinline__ int pack3(uint32_t f) {
  return (int)((f & FLAG_KEEP) | ((f & FLAG_CLONE) << 9) | ((f & FLAG_CHILDREN) << 18));
}
__device__ __forceinline__ int unpackA(int v) { return v & 1023; }
__device__ __forceinline__ int unpackB(int v) { return (v >> 10) & 1023; }
__device__ __forceinline__ int unpackC(int v) { return (v >> 20) & 1023; }

__device__ __forceinline__ uint32_t classify(int64_t i, const float* __restrict__ scaling, const float* __restrict__ opacity,
                                             const float* __restrict__ grad_accum, const int32_t* __restrict__ denom,
                                             const int32_t* __restrict__ max_radii, const PlanScalars& s) {
  const int32_t d = denom[i];
  const float g = d != 0 ? grad_accum[i] / (float)d : 0.f;
  const float s0 = scaling[3 * i], s1 = scaling[3 * i + 1], s2 = scaling[3 * i + 2];
  const float world = expf(fmaxf(s0, fmaxf(s1, s2)));  // exp is monotone: max_c exp(s_c), bit for bit
  const float child_world = expf(logf(world / SPLIT_SHRINK));
  const float o = 1.f / (1.f + expf(-opacity[i]));
  const bool selected = g >= s.max_grad;
  const bool large = world > s.dense_limit;
  const bool clone = selected && !large, split = selected && large;
  const bool low = o < s.min_opacity;
  const bool big_radius = s.screen && (float)max_radii[i] > s.max_screen_size;
  const bool big_world = s.screen && world > s.world_limit;
  const bool big_child = s.screen && child_world > s.world_limit;
  uint32_t f = 0;
  if (!(split || low || big_radius || big_world)) f |= FLAG_KEEP;
  if (clone && !low && !big_world) f |= FLAG_CLONE;
  if (split && !low && !big_child) f |= FLAG_CHILDREN;
  return f;
}

__global__ __launch_bounds__(THREADS) void gs_densify_classify_kernel(const float* __restrict__ scaling,
                                                                       const float* __restrict__ opacity,
                                                                       const float* __restrict__ grad_accum,
                                                                       const int32_t* __restrict__ denom,
                                                                       const int32_t* __restrict__ max_radii, int64_t P,
                                                                       PlanScalars s, uint8_t* __restrict__ flags,
                                                                       int32_t* __restrict__ block_sums /*(3, nblocks)*/,
                                                                       int64_t nblocks) {
  __shared__ int wave_sum[WAVES];
  const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  uint32_t f = 0;
  if (i < P) {
    f = classify(i, scaling, opacity, grad_accum, denom, max_radii, s);
    flags[i] = (uint8_t)f;
  }
  const int total = wave_sum_i32_dpp(pack3(f));
  if ((threadIdx.x & (WAVE - 1)) == 0) wave_sum[threadIdx.x / WAVE] = total;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) t += wave_sum[w];
    block_sums[blockIdx.x] = unpackA(t);
    block_sums[nblocks + blockIdx.x] = unpackB(t);
    block_sums[2 * nblocks + blockIdx.x] = unpackC(t);
  }
}

// exclusive prefix of `v` over the workgroup; `total` = the workgroup's sum, in every thread
__device__ __forceinline__ int block_excl_scan(int v, int* wave_sum, int& total) {
  const int incl = wave_incl_scan_add_dpp(v);
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  __syncthreads();  // wave_sum may still be read from the previous use
  if (lane == WAVE - 1) wave_sum[wave] = incl;
  __syncthreads();
  int before = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    const int t = wave_sum[w];
    before += w < wave ? t : 0;
    total += t;
  }
  return before + incl - v;
}

__global__ __launch_bounds__(THREADS) void gs_densify_scan_kernel(int32_t* __restrict__ block_sums /*(3, nblocks), in place*/,
                                                                   int64_t nblocks, int32_t* __restrict__ counts /*4*/) {
  __shared__ int wave_sum[WAVES];
  int carry[3] = {0, 0, 0};
  for (int64_t base = 0; base < nblocks; base += THREADS) {
    const int64_t b = base + threadIdx.x;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int v = b < nblocks ? block_sums[r * nblocks + b] : 0;
      int total;
      const int excl = block_excl_scan(v, wave_sum, total);
      if (b < nblocks) block_sums[r * nblocks + b] = carry[r] + excl;
      carry[r] += total;
    }
  }
  if (threadIdx.x == 0) {
    counts[0] = carry[0];
    counts[1] = carry[1];
    counts[2] = carry[2];
    counts[3] = carry[2];
  }
}

__global__ __launch_bounds__(THREADS) void gs_densify_scatter_kernel(const uint8_t* __restrict__ flags, int64_t P,
                                                                      const int32_t* __restrict__ block_prefix /*(3, nblocks)*/,
                                                                      int64_t nblocks, const int32_t* __restrict__ counts,
                                                                      int32_t* __restrict__ source, uint8_t* __restrict__ kind) {
  __shared__ int wave_sum[WAVES];
  const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  const uint32_t f = i < P ? flags[i] : 0u;
  int total;
  const int rank = block_excl_scan(pack3(f), wave_sum, total);
  if (f == 0) return;
  const int64_t A = counts[0], B = counts[1], C = counts[2];
  if (f & FLAG_KEEP) {
    const int64_t row = block_prefix[blockIdx.x] + unpackA(rank);
    source[row] = (int32_t)i;
    kind[row] = 0;
  }
  if (f & FLAG_CLONE) {
    const int64_t row = A + block_prefix[nblocks + blockIdx.x] + unpackB(rank);
    source[row] = (int32_t)i;
    kind[row] = 1;
  }
  if (f & FLAG_CHILDREN) {
    const int64_t row = A + B + block_prefix[2 * nblocks + blockIdx.x] + unpackC(rank);
    source[row] = (int32_t)i;
    kind[row] = 2;
    source[row + C] = (int32_t)i;
    kind[row + C] = 3;
  }
}

// ---- apply -----------------------------------------------------------------------------------------------------------

struct ApplyGroup {
  const float* src[3];  // param, exp_avg, exp_avg_sq of the old scene
  float* dst[3];        // of the new one
  uint32_t n;           // P_new * K elements
  uint32_t K;
  uint32_t block0;             // first workgroup of this group
  uint32_t blocks_per_tensor;  // workgroups of one of its tensors
  uint32_t role;
  uint32_t wide;  // bit t: dst[t] is 16-byte aligned
};

struct ApplyTable {
  ApplyGroup group[GR_GS_ADAM_MAX_GROUPS];
  int count;
};

struct ApplyRoles {
  const int32_t* source;
  const uint8_t* kind;
  const float* scaling;   // (P, 3) of the old scene
  const float* rotation;  // (P, 4)
  const float* noise;     // (P, 2, 3)
};

// four floats at any 4-byte-aligned address in one access
struct __attribute__((packed, aligned(4))) Quad4 {
  float x, y, z, w;
};

// component c of a child's position
__device__ __forceinline__ float child_xyz(const ApplyRoles& R, const float* __restrict__ xyz, uint32_t s, uint32_t k, uint32_t c) {
  const float* q = R.rotation + (size_t)s * 4;
  const float* sc = R.scaling + (size_t)s * 3;
  const float* nz = R.noise + ((size_t)s * 2 + k) * 3;
  const float qr = q[0], qx = q[1], qy = q[2], qz = q[3];
  const float norm = sqrtf(qr * qr + qx * qx + qy * qy + qz * qz);
  const float r = qr / norm, x = qx / norm, y = qy / norm, z = qz / norm;
  const float v0 = expf(sc[0]) * nz[0], v1 = expf(sc[1]) * nz[1], v2 = expf(sc[2]) * nz[2];
  float r0, r1, r2;
  if (c == 0) {
    r0 = 1.f - 2.f * (y * y + z * z);
    r1 = 2.f * (x * y - r * z);
    r2 = 2.f * (x * z + r * y);
  } else if (c == 1) {
    r0 = 2.f * (x * y + r * z);
    r1 = 1.f - 2.f * (x * x + z * z);
    r2 = 2.f * (y * z - r * x);
  } else {
    r0 = 2.f * (x * z - r * y);
    r1 = 2.f * (y * z + r * x);
    r2 = 1.f - 2.f * (x * x + y * y);
  }
  return fmaf(r2, v2, fmaf(r1, v1, r0 * v0)) + xyz[(size_t)s * 3 + c];
}

// t: 0 parameter, 1 / 2 the moments.  KC > 0: row length known at compile time; KC = 0: G.K at run time
template <uint32_t KC>
__device__ __forceinline__ void apply_quad(const ApplyGroup& G, int t, uint32_t e0, const ApplyRoles& R) {
  const uint32_t K = KC ? KC : G.K;
  // selected, not indexed: a dynamic index into the by-value group would put it into memory
  const float* __restrict__ src = t == 0 ? G.src[0] : t == 1 ? G.src[1] : G.src[2];
  float* __restrict__ dst = t == 0 ? G.dst[0] : t == 1 ? G.dst[1] : G.dst[2];
  const uint32_t count = min((uint32_t)QUAD, G.n - e0);
  const bool computed = t == 0 && G.role != GR_GS_DENSIFY_CARRIED;
  const uint32_t row0 = e0 / K, col0 = e0 - row0 * K;
  float out[QUAD] = {0.f, 0.f, 0.f, 0.f};
  if (count == QUAD && col0 + QUAD <= K && !computed) {  // the quad lies inside one row
    if (t == 0 || R.kind[row0] == 0) {
      const Quad4 q = *reinterpret_cast<const Quad4*>(src + (size_t)R.source[row0] * K + col0);
      out[0] = q.x, out[1] = q.y, out[2] = q.z, out[3] = q.w;
    }
  } else {
    uint32_t row = row0, col = col0;
    uint32_t s = 0, k = 0;
    bool fresh = true;
#pragma unroll
    for (int j = 0; j < QUAD; ++j) {
      if ((uint32_t)j < count) {
        if (fresh) {
          s = (uint32_t)R.source[row];
          k = R.kind[row];
          fresh = false;
        }
        if (t != 0) {
          if (k == 0) out[j] = src[(size_t)s * K + col];
        } else if (computed && k >= 2) {
          out[j] = G.role == GR_GS_DENSIFY_XYZ ? child_xyz(R, src, s, k - 2, col)
                                               : logf(expf(src[(size_t)s * K + col]) / SPLIT_SHRINK);
        } else {
          out[j] = src[(size_t)s * K + col];
        }
        if (++col == K) {
          col = 0;
          ++row;
          fresh = true;
        }
      }
    }
  }
  if (count == QUAD && ((G.wide >> t) & 1u)) {
    *reinterpret_cast<float4*>(dst + e0) = make_float4(out[0], out[1], out[2], out[3]);
  } else {
#pragma unroll
    for (int j = 0; j < QUAD; ++j)
      if ((uint32_t)j < count) dst[e0 + j] = out[j];
  }
}

__global__ __launch_bounds__(THREADS) void gs_densify_apply_kernel(ApplyTable table, ApplyRoles roles) {
  int gi = 0;
  for (int i = 1; i < table.count; ++i) gi = blockIdx.x >= table.group[i].block0 ? i : gi;
  const ApplyGroup G = table.group[gi];
  uint32_t b = blockIdx.x - G.block0;
  const int t = (b >= G.blocks_per_tensor) + (b >= 2 * G.blocks_per_tensor);
  b -= t * G.blocks_per_tensor;
  const uint32_t e0 = b * ELEMS_PER_BLOCK + threadIdx.x * QUAD;
  if (e0 >= G.n) return;
  switch (G.K) {
    case 1: apply_quad<1>(G, t, e0, roles); break;
    case 3: apply_quad<3>(G, t, e0, roles); break;
    case 4: apply_quad<4>(G, t, e0, roles); break;
    case 9: apply_quad<9>(G, t, e0, roles); break;
    case 24: apply_quad<24>(G, t, e0, roles); break;
    case 45: apply_quad<45>(G, t, e0, roles); break;
    default: apply_quad<0>(G, t, e0, roles); break;
  }
}

constexpr int64_t PLAN_MAX_P = 1ll << 30;  // 2 P rows and their int32 indices

int64_t plan_blocks(int64_t P) { return (P + THREADS - 1) / THREADS; }

struct PlanWorkspace {
  uint8_t* flags;
  int32_t* block_sums;
  size_t bytes;
};

PlanWorkspace carve_plan(void* ws, int64_t P) {
  Carver c(ws);
  PlanWorkspace w;
  w.flags = c.take<uint8_t>((size_t)P);
  w.block_sums = c.take<int32_t>(3 * (size_t)plan_blocks(P));
  w.bytes = c.used();
  return w;
}

}  // namespace
}  // namespace gr

using namespace gr;

extern "C" size_t gr_gs_densify_plan_workspace_bytes(int64_t P) {
  if (P <= 0 || P > PLAN_MAX_P) return 0;
  return carve_plan(nullptr, P).bytes;
}

extern "C" int gr_gs_densify_plan(const float* scaling, const float* opacity, const float* grad_accum, const int32_t* denom,
                                  const int32_t* max_radii, int64_t P, double max_grad, double min_opacity, double extent,
                                  double percent_dense, int use_max_screen_size, double max_screen_size, int32_t* source,
                                  uint8_t* kind, int32_t* counts, int64_t* h_counts, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  GR_REQUIRE(P >= 0 && P <= PLAN_MAX_P, "gs densify plan: P = %lld outside [0, 2^30]", (long long)P);
  if (P == 0) {
    if (h_counts) h_counts[0] = h_counts[1] = h_counts[2] = h_counts[3] = 0;
    if (counts) GR_HIP(hipMemsetAsync(counts, 0, 4 * sizeof(int32_t), stream));
    return GR_OK;
  }
  GR_REQUIRE(scaling && opacity && grad_accum && denom && max_radii && source && kind && counts, "gs densify plan: null argument");
  const PlanWorkspace w = carve_plan(ws, P);
  if (!ws || ws_bytes < w.bytes) {
    set_error("gs densify plan: workspace of %zu bytes, %zu needed", ws_bytes, w.bytes);
    return GR_ERR_WORKSPACE;
  }
  PlanScalars s;
  s.max_grad = (float)max_grad;
  s.min_opacity = (float)min_opacity;
  s.dense_limit = (float)(percent_dense * extent);
  s.world_limit = (float)(0.1 * extent);
  s.screen = use_max_screen_size != 0;
  s.max_screen_size = s.screen ? (float)max_screen_size : 0.f;
  const int64_t nblocks = plan_blocks(P);
  {
    KernelTimer timer("gs_densify_plan", stream);
    hipLaunchKernelGGL(gs_densify_classify_kernel, dim3((unsigned)nblocks), dim3(THREADS), 0, stream, scaling, opacity, grad_accum,
                       denom, max_radii, P, s, w.flags, w.block_sums, nblocks);
    GR_LAUNCH_CHECK();
    hipLaunchKernelGGL(gs_densify_scan_kernel, dim3(1), dim3(THREADS), 0, stream, w.block_sums, nblocks, counts);
    GR_LAUNCH_CHECK();
    hipLaunchKernelGGL(gs_densify_scatter_kernel, dim3((unsigned)nblocks), dim3(THREADS), 0, stream, w.flags, P, w.block_sums,
                       nblocks, counts, source, kind);
    GR_LAUNCH_CHECK();
  }
  if (h_counts) {  // the one host synchronisation of a densification
    int32_t h[4];
    GR_HIP(hipMemcpyAsync(h, counts, sizeof h, hipMemcpyDeviceToHost, stream));
    GR_HIP(hipStreamSynchronize(stream));
    for (int i = 0; i < 4; ++i) h_counts[i] = h[i];
  }
  return GR_OK;
}

extern "C" int gr_gs_densify_apply(const gr_gs_densify_group* groups, int n_groups, int64_t P, int64_t P_new,
                                   const int32_t* source, const uint8_t* kind, const float* scaling, const float* rotation,
                                   const float* noise, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  GR_REQUIRE(n_groups >= 0 && n_groups <= GR_GS_ADAM_MAX_GROUPS && (groups || n_groups == 0),
             "gs densify apply: %d groups (at most %d per call)", n_groups, GR_GS_ADAM_MAX_GROUPS);
  GR_REQUIRE(P >= 0 && P <= PLAN_MAX_P, "gs densify apply: P = %lld outside [0, 2^30]", (long long)P);
  GR_REQUIRE(P_new >= 0 && P_new <= 2 * P, "gs densify apply: P_new = %lld outside [0, 2 P = %lld]", (long long)P_new,
             (long long)(2 * P));
  ApplyTable table;
  memset(&table, 0, sizeof table);
  uint64_t blocks = 0;
  for (int i = 0; i < n_groups; ++i) {
    const gr_gs_densify_group& in = groups[i];
    GR_REQUIRE(in.K >= 0, "gs densify apply: group %d has K = %d", i, in.K);
    GR_REQUIRE(in.role == GR_GS_DENSIFY_CARRIED || in.role == GR_GS_DENSIFY_XYZ || in.role == GR_GS_DENSIFY_SCALING,
               "gs densify apply: group %d has role %d", i, in.role);
    GR_REQUIRE(in.role != GR_GS_DENSIFY_XYZ || in.K == 3, "gs densify apply: the xyz group has K = %d, not 3", in.K);
    GR_REQUIRE(in.role != GR_GS_DENSIFY_SCALING || in.K == 3, "gs densify apply: the scaling group has K = %d, not 3", in.K);
    GR_REQUIRE(in.role != GR_GS_DENSIFY_XYZ || (scaling && rotation && noise),
               "gs densify apply: the xyz group needs the old scaling, rotation and the noise");
    const bool has_state = in.src_exp_avg || in.dst_exp_avg || in.src_exp_avg_sq || in.dst_exp_avg_sq;
    const int64_t n = P_new * in.K;
    GR_REQUIRE(n <= 0xffffffffll - QUAD && P * in.K <= 0xffffffffll - QUAD,
               "gs densify apply: group %d has more elements than the 32-bit element index holds (P_new * K = %lld)", i, (long long)n);
    if (n == 0) continue;  // empty f_rest at SH degree 0; an empty new scene
    GR_REQUIRE(source && kind, "gs densify apply: null source or kind");
    GR_REQUIRE(in.src_param && in.dst_param, "gs densify apply: group %d has a null parameter pointer", i);
    GR_REQUIRE(!has_state || (in.src_exp_avg && in.dst_exp_avg && in.src_exp_avg_sq && in.dst_exp_avg_sq),
               "gs densify apply: group %d has some moment pointers but not all four", i);
    ApplyGroup& G = table.group[table.count++];
    G.src[0] = in.src_param, G.dst[0] = in.dst_param;
    G.src[1] = in.src_exp_avg, G.dst[1] = in.dst_exp_avg;
    G.src[2] = in.src_exp_avg_sq, G.dst[2] = in.dst_exp_avg_sq;
    G.n = (uint32_t)n;
    G.K = (uint32_t)in.K;
    G.role = (uint32_t)in.role;
    G.block0 = (uint32_t)blocks;
    G.blocks_per_tensor = (uint32_t)(((uint64_t)n + ELEMS_PER_BLOCK - 1) / ELEMS_PER_BLOCK);
    const int tensors = has_state ? 3 : 1;
    for (int t = 0; t < tensors; ++t) G.wide |= (uint32_t)(((uintptr_t)G.dst[t] & 15) == 0) << t;
    blocks += (uint64_t)G.blocks_per_tensor * tensors;
  }
  GR_REQUIRE(blocks < (1ull << 31), "gs densify apply: %llu workgroups exceed one launch", (unsigned long long)blocks);
  if (blocks == 0) return GR_OK;
  ApplyRoles roles;
  roles.source = source;
  roles.kind = kind;
  roles.scaling = scaling;
  roles.rotation = rotation;
  roles.noise = noise;
  KernelTimer timer("gs_densify_apply", stream);
  hipLaunchKernelGGL(gs_densify_apply_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, stream, table, roles);
  GR_LAUNCH_CHECK();
  return GR_OK;
}
