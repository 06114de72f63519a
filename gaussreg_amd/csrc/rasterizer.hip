// 3D-Gaussian-splatting rasterizer forward for MI355X (gfx950), batched over views.
//
// Interface replaced: diff_gaussian_rasterization.GaussianRasterizer.forward (public upstream
// graphdeco-inria/diff-gaussian-rasterization; NOT in the GaussReg tree).
// Numerics contract: oracle/rasterizer_oracle.c -- every fp32 operation below is written in the
// same order (fmaf where the oracle says fmaf, separate mul/add elsewhere; this TU is compiled
// with -ffp-contract=off), so images and radii are compared bit-exact with the oracle.
//
// Pipeline per batch of V views over one set of P Gaussians:
//   preprocess  1 thread / Gaussian, loops over the V cameras (inputs read once per batch;
//               cov3D built once): cull, project, cov2D, conic, radius, tile rect, SH -> RGB
//   depth sort  stable radix sort of (view, depth bits) -> per-view front-to-back Gaussian order
//   tile bin    NO second sort and no (tile, id) key stream: chunks of 2048 depth-ordered Gaussians are binned by tile inside
//               LDS and written out as one contiguous block per chunk (see "tile binning" below); a tile's list is the
//               concatenation of its per-chunk segments -- in depth order, i.e. exactly upstream's single sort of
//               (tile << 32 | depth) keys
//   blend       1 workgroup / tile (16x16 px, 4 waves): walks the tile's segments chunk by chunk, Gaussian parameters
//               staged through LDS in batches of 256, front-to-back alpha blending, deterministic exp
#include <algorithm>
#include <type_traits>
#include <vector>

#include <atomic>
#include <optional>

#include "raster_shared.hpp"

namespace gr {
namespace {

static_assert(TILE == RASTER_TILE, "get_rect / rect_decode (common.hpp) are written for this tile size");
static_assert(TILE == PLAN_TILE && WAVE == PLAN_WAVE && SCAN_SINGLE_ROW == PLAN_SCAN_SINGLE_ROW && MAX_VIEWS == PLAN_MAX_VIEWS,
              "raster_plan.hpp states these values for itself");


// ------------------------------------------------------------------------------------ preprocess
// Per (view, Gaussian) the preprocess emits a 32-bit depth-sort field and the packed tile rectangle (26 bits:
// x:7 | y:7 | w:6 | h:6; rectangles that do not fit store RECT_MARKER26 and are rebuilt from the record).  The sort moves
// (field << 32 | Gaussian id) words and looks the rectangle up by id in its last pass.
// Field: float bits of depth minus those of 0.125 (visible depths are > 0.2, so this is > 0 and order-preserving; < 2^27
// while depth < 8192): 27 bits sort in three 9-bit passes.  A depth >= 8192 raises a flag and the call re-sorts on the
// full 32 depth bits (slow path, never taken by sane scenes).
constexpr int KEY_DEPTH_BITS = 27;
static_assert(KEY_DEPTH_BITS == PLAN_KEY_DEPTH_BITS, "raster_plan.hpp states this value for itself");
constexpr uint32_t KEY_DEPTH_BASE = 0x3E000000u;  // bits of 0.125f

__device__ __forceinline__ uint32_t pack_rect(const int* rmin, const int* rmax) {
  const int w = rmax[0] - rmin[0], h = rmax[1] - rmin[1];
  if (w > 63 || h > 63 || rmin[0] > 126 || rmin[1] > 126) return RECT_MARKER26;
  return (uint32_t)rmin[0] | ((uint32_t)rmin[1] << 7) | ((uint32_t)w << 14) | ((uint32_t)h << 20);
}

constexpr int REC_PLANE = 66;  // float4 per record-piece plane (64 + 2): the transposed ds_read_b128 are conflict-free
constexpr int SH_ROW = 13;  // float4 per staged Gaussian: 12 used + 1 pad -> conflict-free ds_read_b128

// SH16: 16 coefficients per Gaussian, 16-byte aligned.  LATE (one view per call): the 192 bytes are fetched only by the
// Gaussians that survive the culling of THE view (12 float4 loads per visible lane, straight into registers) -- with a
// single camera 40 % of the benchmark scene never reads its SH; with several views every Gaussian is visible somewhere,
// and the coalesced stream through LDS below is the better way.
// The body (preprocess_body.hpp) is included in preprocess_kernel (WAVE_MM = false: the kernel as it was) and in
// preprocess_many_kernel (more than four views per call with the bucket depth sort behind it: per-wave key ranges).
template <bool HAS_SH, bool HAS_COV, bool SH16, bool LATE>
__global__ __launch_bounds__(256) void preprocess_kernel(
    int P, int D, int M, int V, const DevView* __restrict__ views, const float* __restrict__ means3D,
    const float* __restrict__ shs, const float* __restrict__ colors_precomp,
    const float* __restrict__ opacities, const float* __restrict__ scales,
    const float* __restrict__ rotations, const float* __restrict__ cov3D_precomp, int W, int H,
    int32_t* __restrict__ radii, float4* __restrict__ rec, uint32_t* __restrict__ dfield,
    uint32_t* __restrict__ rect_raw, int32_t* __restrict__ far_flag, DevView cam1, int far_seq,
    int2* __restrict__ key_mm) {
  constexpr bool WAVE_MM = false;
#define GR_PREPROCESS_BODY_OK
#include "preprocess_body.hpp"
#undef GR_PREPROCESS_BODY_OK
}

template <bool HAS_SH, bool HAS_COV, bool SH16>
__global__ __launch_bounds__(256) void preprocess_many_kernel(
    int P, int D, int M, int V, const DevView* __restrict__ views, const float* __restrict__ means3D,
    const float* __restrict__ shs, const float* __restrict__ colors_precomp,
    const float* __restrict__ opacities, const float* __restrict__ scales,
    const float* __restrict__ rotations, const float* __restrict__ cov3D_precomp, int W, int H,
    int32_t* __restrict__ radii, float4* __restrict__ rec, uint32_t* __restrict__ dfield,
    uint32_t* __restrict__ rect_raw, int32_t* __restrict__ far_flag, DevView cam1, int far_seq,
    int2* __restrict__ key_mm) {
  constexpr bool WAVE_MM = true;
  constexpr bool LATE = false;
#define GR_PREPROCESS_BODY_OK
#include "preprocess_body.hpp"
#undef GR_PREPROCESS_BODY_OK
}

// slow path of the depth sort: the field becomes the full 32 depth bits (visible depths are > 0.2: non-zero)
__global__ __launch_bounds__(256) void full_keys_kernel(int64_t n, const float4* __restrict__ rec,
                                                        const int32_t* __restrict__ radii, uint32_t* __restrict__ dfield) {
  const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= n) return;
  dfield[o] = radii[o] > 0 ? __float_as_uint(rec[4 * o + 3].y) : 0u;
}

// ------------------------------------------------------------------------------------ tile binning
// Input: per view the Gaussians in depth order (ids) with their tile rectangles (26-bit packing, RECT_MARKER26 = "did not
// fit, rebuild from the record").  Output: point_list, CHUNK-major: the instances of one chunk of BIN_CHUNK consecutive
// depth-ordered Gaussians form one contiguous block, sorted by tile inside LDS (depth order kept inside every (chunk,
// tile) segment), and seg_off[view][chunk][tile] says where each segment starts.  The blend walks a tile's segments in
// chunk order = depth order, so it sees exactly what a stable sort of (tile, depth-rank) keys would give, but no key is
// ever materialised and every global write is a full coalesced line (scattering 4-byte ids straight into per-tile lists
// was measured first: 62 M partial-line writes per 32 views cost 1.1 ms in the L2 alone).
//   count    a few views: a workgroup owns a chunk, histograms its tiles in LDS -> chunk_cnt, chunk_total; many views:
//            only the chunk totals -- out of the bucket launch of the depth sort, or by chunk_total_kernel behind the
//            three-pass sort
//   scan     chunk totals -> chunk bases (per view); a few views: per chunk an exclusive scan over the tiles -> seg_off
//            (many views: the scatter scans the tile counts it builds anyway and writes its own row of seg_off)
//   scatter  a workgroup owns a chunk; wave w owns a quarter of its Gaussians and a private cursor per tile in LDS
//            (segment start + the earlier waves' counts).  64 Gaussians (lanes) per step:
//              small rectangles (<= 8 x 8 tiles, wave-uniform test): with Mx = the largest width and My = the largest height
//                in the wave, a rectangle holds at most ONE tile of every residue class (x mod Mx, y mod My), so the wave
//                walks the Mx*My classes and in each every lane issues the (at most one) tile it has there (the exact
//                moduli, not a power of two: most steps of a 640 x 480 frame are 3 x 3 or 3 x 2, nine or six rounds instead
//                of sixteen).  A given tile is therefore requested by
//                all its Gaussians in the SAME instruction, and LANE_ORDERED (one ds_add_rtn_u32; equal-address lanes
//                served in lane order -- probed on the device, see below) hands them consecutive slots in lane = depth
//                order.  Without that property the lanes of a tile find each other with one ballot per tile-id bit and
//                rank themselves explicitly.
//              a step containing a larger rectangle is walked one Gaussian at a time, lanes over its tiles.
//            A wave's LDS instructions execute in issue order, so every segment stays in depth order.  Ids land in an LDS
//            staging block at their final chunk-local position; the block is then copied out with coalesced stores
//            (chunks whose instances do not fit the staging block write straight to their final global position).
// With >= 8 views the workgroups of one view all run on the same XCD (block b sits on XCD b % 8).

// block -> (view, chunk); XCD-affine when there are at least 8 views
__device__ __forceinline__ bool bin_block(int V, int nchunk, int& v, int& c) {
  const int b = blockIdx.x;
  if (V >= 8) {
    const int k = b >> 3;
    v = (b & 7) + 8 * (k / nchunk);
    c = k % nchunk;
    return v < V;
  }
  v = b / nchunk;
  c = b % nchunk;
  return true;
}
inline int bin_grid(int V, int nchunk) { return V >= 8 ? 8 * ((V + 7) / 8) * nchunk : V * nchunk; }
// (which launches count for which frame, the scatter's workgroup size and its LDS: raster_plan.hpp)

// n mod d for n < 256, 1 <= d <= 8, exact: with m = floor(2^15 / d) + 1 the error m d - 2^15 is at most d, and
// 255 * 8 < 2^15, so (n m) >> 15 = floor(n / d).  The eight 16-bit multipliers sit in two literals (d wave-uniform:
// scalar selects, no division; d a constant: folded).
__device__ __forceinline__ constexpr int mod_small(int n, int d) {
  const unsigned long long tab = d <= 4 ? 0x2001'2aab'4001'8001ull : 0x1001'124a'1556'199aull;
  const unsigned int m = (unsigned int)(tab >> (((d - 1) & 3) * 16)) & 0xffffu;
  return n - (int)(((unsigned int)n * m) >> 15) * d;
}
static_assert(mod_small(255, 7) == 255 % 7 && mod_small(254, 3) == 254 % 3 && mod_small(250, 5) == 0 &&
              mod_small(251, 6) == 251 % 6 && mod_small(255, 8) == 7 && mod_small(200, 1) == 0, "mod_small multipliers");
// calls f(integral_constant<int, mx>) for the wave-uniform mx in 1 .. 8
template <typename F>
__device__ __forceinline__ void by_modulus(int mx, F&& f) {
  switch (mx) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 5: f(std::integral_constant<int, 5>{}); break;
    case 6: f(std::integral_constant<int, 6>{}); break;
    case 7: f(std::integral_constant<int, 7>{}); break;
    default: f(std::integral_constant<int, 8>{}); break;
  }
}

__global__ __launch_bounds__(BIN_T) void tile_count_kernel(int P, int V, int gx, int gy, int nchunk,
                                                           const int32_t* __restrict__ nvis,
                                                           const uint32_t* __restrict__ rects,
                                                           const int32_t* __restrict__ ids,
                                                           const float4* __restrict__ rec,
                                                           uint16_t* __restrict__ chunk_cnt,
                                                           int32_t* __restrict__ chunk_total) {
  extern __shared__ unsigned int s_hist[];
  __shared__ int s_wsum[BIN_T / WAVE];
  int v, c;
  if (!bin_block(V, nchunk, v, c)) return;
  const int tiles = gx * gy;
  for (int T = threadIdx.x; T < tiles; T += BIN_T) s_hist[T] = 0u;
  __syncthreads();
  const int64_t vbase = (int64_t)v * P;
  const int nv = nvis[v];
  int mine = 0;
  // all of a thread's rectangles are requested before the first one is used: one memory round trip instead of eight
  uint32_t rr[BIN_CHUNK / BIN_T];
#pragma unroll
  for (int it = 0; it < BIN_CHUNK / BIN_T; ++it) {
    const int t = c * BIN_CHUNK + it * BIN_T + threadIdx.x;
    rr[it] = t < nv ? rects[vbase + t] : 0u;
  }
#pragma unroll
  for (int it = 0; it < BIN_CHUNK / BIN_T; ++it) {
    const int t = c * BIN_CHUNK + it * BIN_T + threadIdx.x;
    const uint32_t r = rr[it];
    if (r == 0u) continue;
    int x0, y0, w, h;
    if (!rect_decode(r, r == RECT_MARKER26 ? ids[vbase + t] : 0, vbase, rec, gx, gy, x0, y0, w, h)) continue;
    mine += w * h;
    for (int y = y0; y < y0 + h; ++y)
      for (int x = x0; x < x0 + w; ++x) atomicAdd(&s_hist[y * gx + x], 1u);
  }
  const int wsum = wave_sum_i32_dpp(mine);
  if ((threadIdx.x & (WAVE - 1)) == 0) s_wsum[threadIdx.x / WAVE] = wsum;
  __syncthreads();
  uint16_t* dst = chunk_cnt + ((int64_t)v * nchunk + c) * tiles;
  // a tile can appear at most once per Gaussian: counts <= BIN_CHUNK < 65536
  for (int T = threadIdx.x; T < tiles; T += BIN_T) dst[T] = (uint16_t)s_hist[T];
  if (threadIdx.x == 0) {
    int tot = 0;
    for (int i = 0; i < BIN_T / WAVE; ++i) tot += s_wsum[i];
    chunk_total[v * nchunk + c] = tot;
  }
}

// many views per call: only the instance total of every (view, chunk) -- no tile histogram.  The scatter counts the tiles
// of its chunk anyway and scans them itself (tile_scatter_kernel SEG_SELF_SCAN); it needs nothing but the chunk bases.
__global__ __launch_bounds__(BIN_T) void chunk_total_kernel(int P, int V, int gx, int gy, int nchunk,
                                                            const int32_t* __restrict__ nvis,
                                                            const uint32_t* __restrict__ rects,
                                                            const int32_t* __restrict__ ids,
                                                            const float4* __restrict__ rec,
                                                            int32_t* __restrict__ chunk_total) {
  __shared__ int s_wsum[BIN_T / WAVE];
  int v, c;
  if (!bin_block(V, nchunk, v, c)) return;
  const int64_t vbase = (int64_t)v * P;
  const int nv = nvis[v];
  int mine = 0;
  uint32_t rr[BIN_CHUNK / BIN_T];
#pragma unroll
  for (int it = 0; it < BIN_CHUNK / BIN_T; ++it) {
    const int t = c * BIN_CHUNK + it * BIN_T + threadIdx.x;
    rr[it] = t < nv ? rects[vbase + t] : 0u;
  }
#pragma unroll
  for (int it = 0; it < BIN_CHUNK / BIN_T; ++it) {
    const int t = c * BIN_CHUNK + it * BIN_T + threadIdx.x;
    const uint32_t r = rr[it];
    int x0, y0, w, h;
    if (r != 0u && rect_decode(r, r == RECT_MARKER26 ? ids[vbase + t] : 0, vbase, rec, gx, gy, x0, y0, w, h)) mine += w * h;
  }
  const int wsum = wave_sum_i32_dpp(mine);
  if ((threadIdx.x & (WAVE - 1)) == 0) s_wsum[threadIdx.x / WAVE] = wsum;
  __syncthreads();
  if (threadIdx.x == 0) {
    int tot = 0;
    for (int i = 0; i < BIN_T / WAVE; ++i) tot += s_wsum[i];
    chunk_total[v * nchunk + c] = tot;
  }
}

// largest chunk total (sizes the scatter's LDS staging block); one workgroup, no same-address atomics
__global__ __launch_bounds__(1024) void chunk_max_kernel(int n, const int32_t* __restrict__ chunk_total,
                                                         int32_t* __restrict__ chunk_max) {
  __shared__ int s_m[1024 / WAVE];
  int m = 0;
  for (int i = threadIdx.x; i < n; i += 1024) m = max(m, chunk_total[i]);
  m = wave_max_i32_dpp(m);
  if ((threadIdx.x & (WAVE - 1)) == 0) s_m[threadIdx.x / WAVE] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 0; i < 1024 / WAVE; ++i) m = max(m, s_m[i]);
    *chunk_max = m;
  }
}

// per chunk: seg_off[tile] = view base + chunk base + exclusive scan of the chunk's tile counts; [tiles] = end
// SELF (a few views per call): no scan launch ran before this kernel -- every workgroup sums the raw chunk totals in front
// of its own (at most a few thousand values), and the first chunk of every view leaves the view's total and its largest
// chunk total for the host.  One launch less in a frame that is a chain of launches.
template <bool SELF>
__global__ __launch_bounds__(256) void seg_scan_kernel(int V, int tiles, int nchunk, const uint16_t* __restrict__ chunk_cnt,
                                                       const int32_t* __restrict__ chunk_base /* per view; SELF: raw totals */,
                                                       int32_t* __restrict__ totals, uint32_t* __restrict__ seg_off,
                                                       int32_t* __restrict__ mail, int mail_seq) {
  // mail (SELF only; host-mapped pinned memory or null): [V] totals, [V] chunk maxima, [1] far flag word, [V] stamps -- the host
  // polls the stamps instead of waiting for a device-to-host copy behind an event (both sat in the stream in front of the
  // scatter: 4 us of copy + a 6 - 8 us hand-over gap per frame)
  __shared__ int s_w[256 / WAVE];
  __shared__ int s_carry;
  const int v = blockIdx.x / nchunk, c = blockIdx.x % nchunk;
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
  int vb = 0;
  if (SELF) {
    const int me = (int)blockIdx.x;  // = v * nchunk + c: everything in front belongs to earlier views / chunks
    int part = 0;
    for (int i = threadIdx.x; i < me; i += 256) part += chunk_base[i];
    part = wave_sum_i32_dpp(part);
    if (lane == 0) s_w[wv] = part;
    __syncthreads();
    vb = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    __syncthreads();
    if (c == 0) {  // block-uniform
      int sum = 0, mx = 0;
      for (int i = threadIdx.x; i < nchunk; i += 256) {
        const int t = chunk_base[v * nchunk + i];
        sum += t;
        mx = max(mx, t);
      }
      sum = wave_sum_i32_dpp(sum);
      mx = wave_max_i32_dpp(mx);
      if (lane == 0) {
        s_w[wv] = sum;
      }
      __shared__ int s_m[256 / WAVE];
      if (lane == 0) s_m[wv] = mx;
      __syncthreads();
      if (threadIdx.x == 0) {
        const int tv = s_w[0] + s_w[1] + s_w[2] + s_w[3], mv = max(max(s_m[0], s_m[1]), max(s_m[2], s_m[3]));
        totals[v] = tv;
        totals[V + v] = mv;
        if (mail != nullptr) {
          __hip_atomic_store(&mail[v], tv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          __hip_atomic_store(&mail[V + v], mv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          if (v == 0) __hip_atomic_store(&mail[2 * V], totals[2 * V], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          __hip_atomic_store(&mail[2 * V + 1 + v], mail_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
      }
      __syncthreads();
    }
  } else {
    for (int u = 0; u < v; ++u) vb += totals[u];
  }
  const uint16_t* src = chunk_cnt + ((int64_t)v * nchunk + c) * tiles;
  uint32_t* dst = seg_off + ((int64_t)v * nchunk + c) * (tiles + 1);
  if (threadIdx.x == 0) s_carry = SELF ? vb : vb + chunk_base[v * nchunk + c];
  __syncthreads();
  for (int T0 = 0; T0 < tiles; T0 += 256) {
    const int T = T0 + threadIdx.x;
    const int n = T < tiles ? (int)src[T] : 0;
    const int incl = wave_incl_scan_add_dpp(n);
    if (lane == WAVE - 1) s_w[wv] = incl;
    __syncthreads();
    int base = s_carry;
    for (int i = 0; i < wv; ++i) base += s_w[i];
    if (T < tiles) dst[T] = (uint32_t)(base + incl - n);
    __syncthreads();
    if (threadIdx.x == 255) s_carry = base + incl;
    __syncthreads();
  }
  if (threadIdx.x == 0) dst[tiles] = (uint32_t)s_carry;
}

// TT = threads per workgroup: 256 (four waves, each a quarter of the chunk) for many views per call; 1024 for a few views,
// where the launch has fewer workgroups than the chip has CUs and a workgroup's walk through its chunk IS the kernel's
// duration (16 waves, an eighth of the steps each: 33 -> 12 us per one-camera frame)
// SEG says where the chunk's place in the list and its segment starts come from:
//   SEG_READ       (a few views per call, plain path) tile_count_kernel + seg_scan_kernel wrote every row of seg_off
//   SEG_SELF_RAW   (a few views per call, behind the bucket depth sort): no count / scan launch ran before this one.  The
//                  chunk totals came out of the sort (chunk_total: raw, per (view, chunk)); every workgroup sums the ones in
//                  front of its own, and the first chunk of a view reports the view's total and largest chunk to the host
//                  (see seg_scan_kernel<true>, whose job this is otherwise)
//   SEG_SELF_SCAN  (many views per call): chunk_total_kernel + exclusive_scan_i32 left the raw totals, the chunk bases
//                  inside every view (chunk_total + V * nchunk) and the view totals
// In both SELF modes the workgroup scans the tile counts it has to build anyway and WRITES its row of seg_off for the blend.
// (the constants: raster_plan.hpp)
struct SelfSeg {
  const int32_t* chunk_total;
  int32_t* totals;
  int32_t* mail;
  int mail_seq;
};
// The per-wave cursors are 16-bit, two tiles to an LDS word (rows of an even number of tiles): positions inside the chunk,
// which holds at most 65 535 instances -- a larger one (block-uniform `big`) keeps positions inside the tile's segment and
// writes at seg_off[tile] + position.  A cursor never carries into its neighbour: it stays below the chunk (segment) end.
template <bool LANE_ORDERED, int TT, int SEG = SEG_READ>
__global__ __launch_bounds__(TT) void tile_scatter_kernel(int P, int V, int gx, int gy, int nchunk, int tile_bits,
                                                             int stage_cap, const int32_t* __restrict__ nvis,
                                                             const uint32_t* __restrict__ rects,
                                                             const int32_t* __restrict__ ids,
                                                             const float4* __restrict__ rec,
                                                             uint32_t* __restrict__ seg_off,
                                                             int32_t* __restrict__ point_list, unsigned int list_cap, int elist_cap,
                                                             SelfSeg self) {
  // list_cap: entries the point list holds.  A speculative launch (gr_raster_forward) sizes the list before the instance
  // count is known: a chunk that would end past it writes nothing (the host then repeats the render with a larger list)
  extern __shared__ unsigned int s_cur[];  // [waves][row] 16-bit counts -> cursors, then [stage_cap] staged chunk-local indices
  constexpr int NW = TT / WAVE, CW = BIN_CHUNK / NW;
  constexpr bool SELF = SEG != SEG_READ;
  int v, c;
  if (!bin_block(V, nchunk, v, c)) return;
  const int tiles = gx * gy;
  const int row = (tiles + 1) & ~1;  // halfwords per wave row
  uint32_t* seg = seg_off + ((int64_t)v * nchunk + c) * (tiles + 1);
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
  // the wave's rectangles and ids, requested up front and before anything else is waited for (on clamped positions; what
  // lies past the view's visible count is dropped once that count has arrived): both walks below run out of registers, and
  // the trip to memory overlaps the ones of the prologue instead of following them
  const int64_t vbase = (int64_t)v * P;
  const int w_begin = c * BIN_CHUNK + wv * (BIN_CHUNK / (TT / WAVE));
  uint32_t rr[BIN_CHUNK / TT];
  int32_t ii[BIN_CHUNK / TT];
#pragma unroll
  for (int j = 0; j < BIN_CHUNK / TT; ++j) {
    const int64_t o = vbase + min(w_begin + j * WAVE + lane, P - 1);
    rr[j] = rects[o];
    ii[j] = ids[o];
  }
  const int nv = nvis[v];
  __shared__ int s_red[2][TT / WAVE];
  __shared__ unsigned int s_carry;
  unsigned int chunk_begin;
  int total;
  if (SEG == SEG_SELF_RAW) {
    const int me = v * nchunk + c;  // everything in front belongs to earlier views / chunks
    int part = 0;
    for (int i = threadIdx.x; i < me; i += TT) part += self.chunk_total[i];
    part = wave_sum_i32_dpp(part);
    if (lane == 0) s_red[0][wv] = part;
    __syncthreads();
    int front = 0;
#pragma unroll
    for (int w2 = 0; w2 < TT / WAVE; ++w2) front += s_red[0][w2];
    chunk_begin = (unsigned int)front;
    total = self.chunk_total[me];
    if (c == 0) {  // block-uniform: the view's figures for the host
      __syncthreads();
      int sum = 0, mx = 0;
      for (int i = threadIdx.x; i < nchunk; i += TT) {
        const int t = self.chunk_total[v * nchunk + i];
        sum += t;
        mx = max(mx, t);
      }
      sum = wave_sum_i32_dpp(sum);
      mx = wave_max_i32_dpp(mx);
      if (lane == 0) s_red[0][wv] = sum, s_red[1][wv] = mx;
      __syncthreads();
      if (threadIdx.x == 0) {
        int tv = 0, mv = 0;
        for (int w2 = 0; w2 < TT / WAVE; ++w2) tv += s_red[0][w2], mv = max(mv, s_red[1][w2]);
        self.totals[v] = tv;
        self.totals[V + v] = mv;
        if (self.mail != nullptr) {
          __hip_atomic_store(&self.mail[v], tv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          __hip_atomic_store(&self.mail[V + v], mv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          if (v == 0) __hip_atomic_store(&self.mail[2 * V], self.totals[2 * V], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          __hip_atomic_store(&self.mail[2 * V + 1 + v], self.mail_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
      }
    }
  } else if (SEG == SEG_SELF_SCAN) {
    // (V <= MAX_VIEWS: the views in front are a few scalar loads)
    unsigned int front = (unsigned int)self.chunk_total[(int64_t)V * nchunk + v * nchunk + c];
    for (int u = 0; u < v; ++u) front += (unsigned int)self.totals[u];
    chunk_begin = front;
    total = self.chunk_total[v * nchunk + c];
  } else {
    chunk_begin = seg[0];
    total = (int)(seg[tiles] - chunk_begin);
    if (total == 0 || seg[tiles] > list_cap) return;  // block-uniform
  }
  if (SELF && total == 0) {  // an empty row for the blend
    for (int T = threadIdx.x; T <= tiles; T += TT) seg[T] = chunk_begin;
    return;
  }
  // (SELF: a chunk that would end past the list still counts and scans: the render that repeats this frame with a larger
  // list finds every row of seg_off in place; it stops before it writes any entry)
  const bool big = total > 0xffff;
  const bool staged = !big && total <= stage_cap;
  unsigned int* myw = s_cur + wv * (row / 2);  // this wave's cursor row, two tiles per word
  unsigned short* const cur16 = reinterpret_cast<unsigned short*>(s_cur);
  unsigned short* my16 = cur16 + wv * row;
  // staged entries are 16-bit positions inside the chunk (BIN_CHUNK <= 65536); the ids are looked up on the way out
  unsigned short* stage = reinterpret_cast<unsigned short*>(s_cur + NW * (row / 2));
  // (elist_cap > 0) per wave: the (owner lane, tile) words of one 64-Gaussian step, behind the staging block
  unsigned int* elist = s_cur + NW * (row / 2) + (stage_cap + 1) / 2 + wv * elist_cap;
  for (int T = threadIdx.x; T < NW * (row / 2); T += TT) s_cur[T] = 0u;
  __syncthreads();
  const int w_end = min(nv, w_begin + CW);
#pragma unroll
  for (int j = 0; j < CW / WAVE; ++j) {
    const int t = w_begin + j * WAVE + lane;
    rr[j] = t < w_end ? rr[j] : 0u;  // (past the view's visible count the arrays hold leftovers)
    ii[j] = t < w_end ? ii[j] : 0;
  }
  // ---- phase A: this wave's tile counts
  if constexpr (TT == WIDE_T) {
    // a few views per call: every lane loops over its own rectangle (one camera: 5 390 views/s against 5 260 with the
    // residue-class walk of phase C)
    auto count = [&](int tile) { atomicAdd(&myw[tile >> 1], 1u << ((tile & 1) * 16)); };
#pragma unroll
    for (int j = 0; j < CW / WAVE; ++j) {
      const uint32_t r = rr[j];
      int x0 = 0, y0 = 0, w = 0, h = 0;
      if (r != 0u && !rect_decode(r, ii[j], vbase, rec, gx, gy, x0, y0, w, h)) w = h = 0;
      const int Mx = wave_max_i32_dpp(w);
      if (Mx == 0) continue;  // (a live rectangle has w > 0 and h > 0)
      for (int y = y0; y < y0 + h; ++y)
        for (int x = x0; x < x0 + w; ++x) count(y * gx + x);
    }
  } else {
    // No walk: the wave's cursor row is a difference grid, cell = tile.  A rectangle adds +1 at (x0, y0), -1 at (x0 + w, y0)
    // and (x0, y0 + h), +1 at (x0 + w, y0 + h) -- corners on the right or bottom edge of the image are left out: they would
    // only feed cells outside it -- and the 2-D inclusive prefix of the grid is the number of the wave's rectangles on each
    // tile: at most four LDS adds per Gaussian whatever its size, no moduli, no class loop, no separate path for wide ones.
    // Exactness: a cell is half (tile & 1) of a word and is changed by a plain 32-bit add of +-(1 << 16 (tile & 1)), so a
    // word holds the INTEGER lo + 65536 hi of its two signed cells (a negative lo borrows from the upper half; it is not
    // two independent halfwords).  A wave holds CW = 512 rectangles, each of which changes a cell, a column sum or the final
    // count by at most one: every cell stays within +-512 at every stage, |lo + 65536 hi| < 2^31, and the final counts are
    // 0 .. 512, where the integer and the two halfwords phase B reads are the same thing.
    static_assert(CW <= 0x7fff, "signed 16-bit difference cells");
    auto corner = [&](int tile, unsigned int one) { atomicAdd(&myw[tile >> 1], one << ((tile & 1) * 16)); };
    auto wave_sync = [] {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
#pragma unroll
    for (int j = 0; j < CW / WAVE; ++j) {
      const uint32_t r = rr[j];
      int x0 = 0, y0 = 0, w = 0, h = 0;
      if (r != 0u && rect_decode(r, ii[j], vbase, rec, gx, gy, x0, y0, w, h)) {
        const int t00 = y0 * gx + x0, t10 = t00 + h * gx;
        const bool in_x = x0 + w < gx, in_y = y0 + h < gy;
        corner(t00, 1u);
        if (in_x) corner(t00 + w, ~0u);
        if (in_y) corner(t10, ~0u);
        if (in_x && in_y) corner(t10 + w, 1u);
      }
    }
    wave_sync();
    if ((gx & 1) == 0) {
      // rows start on a word: both passes stay on the integers.  Down the columns (lanes = word columns) the running sum
      // of the words is the word of the running sums.
      const int nw = gx >> 1;
      for (int k = lane; k < nw; k += WAVE) {
        unsigned int run = 0u;
        int y = 0;
        for (; y + 4 <= gy; y += 4) {  // four rows requested at a time, not one LDS round trip per row
          unsigned int* p = myw + y * nw + k;
          const unsigned int a0 = p[0], a1 = p[nw], a2 = p[2 * nw], a3 = p[3 * nw];
          p[0] = run += a0;
          p[nw] = run += a1;
          p[2 * nw] = run += a2;
          p[3 * nw] = run += a3;
        }
        for (; y < gy; ++y) myw[y * nw + k] = run += myw[y * nw + k];
      }
      wave_sync();
      // Along the rows (lanes = rows): n + (n << 16) is the word of {lo, lo + hi}, and the sum in front of the word goes
      // into both halves.  This is the last pass: what leaves is a count, so the upper half IS the row's sum so far.
      for (int y = lane; y < gy; y += WAVE) {
        unsigned int* p = myw + y * nw;
        unsigned int front = 0u;  // (the sum in front) * 0x10001
        auto step = [&](unsigned int n) {
          n += (n << 16) + front;
          front = (n >> 16) * 0x10001u;
          return n;
        };
        int k = 0;
        for (; k + 4 <= nw; k += 4) {
          const unsigned int a0 = p[k], a1 = p[k + 1], a2 = p[k + 2], a3 = p[k + 3];
          p[k] = step(a0);
          p[k + 1] = step(a1);
          p[k + 2] = step(a2);
          p[k + 3] = step(a3);
        }
        for (; k < nw; ++k) p[k] = step(p[k]);
      }
    } else {
      // an odd number of tile columns: a column changes halves from row to row.  Turn the integers into independent signed
      // halfwords first (+ 65536 where lo < 0 took one from the upper half), then both passes run on halfwords.
      for (int i = lane; i < row / 2; i += WAVE) {
        const unsigned int n = myw[i];
        myw[i] = n + ((n & 0x8000u) << 1);
      }
      wave_sync();
      short* g16 = reinterpret_cast<short*>(my16);
      for (int x = lane; x < gx; x += WAVE) {
        int run = 0;
        for (int y = 0; y < gy; ++y) g16[y * gx + x] = (short)(run += g16[y * gx + x]);
      }
      wave_sync();
      for (int y = lane; y < gy; y += WAVE) {
        int run = 0;
        for (int x = 0; x < gx; ++x) g16[y * gx + x] = (short)(run += g16[y * gx + x]);
      }
    }
  }
  __syncthreads();
  // ---- phase B: counts -> cursors (chunk-local; segment-local for a big chunk)
  if (SELF) {
    // the segment starts are this workgroup's own exclusive scan over the tiles of the counts it just made
    if (threadIdx.x == 0) s_carry = 0u;
    __syncthreads();
    for (int T0 = 0; T0 < tiles; T0 += TT) {
      const int T = T0 + (int)threadIdx.x;
      unsigned int cw[NW];
      int n_all = 0;
#pragma unroll
      for (int w2 = 0; w2 < NW; ++w2) {
        cw[w2] = T < tiles ? cur16[w2 * row + T] : 0u;
        n_all += (int)cw[w2];
      }
      const int incl = wave_incl_scan_add_dpp(n_all);
      if (lane == WAVE - 1) s_red[0][wv] = incl;
      __syncthreads();
      unsigned int before = s_carry + (unsigned int)(incl - n_all);
      for (int w2 = 0; w2 < wv; ++w2) before += (unsigned int)s_red[0][w2];
      if (T < tiles) {
        seg[T] = chunk_begin + before;
        unsigned int run = big ? 0u : before;
#pragma unroll
        for (int w2 = 0; w2 < NW; ++w2) {
          cur16[w2 * row + T] = (unsigned short)run;
          run += cw[w2];
        }
      }
      __syncthreads();
      if (threadIdx.x == TT - 1) s_carry = before + (unsigned int)n_all;
      __syncthreads();
    }
    if (threadIdx.x == 0) seg[tiles] = chunk_begin + (unsigned int)total;
    if (chunk_begin + (unsigned int)total > list_cap) return;  // block-uniform
  } else {
    for (int T = threadIdx.x; T < tiles; T += TT) {
      unsigned int run = big ? 0u : seg[T] - chunk_begin;
#pragma unroll
      for (int w2 = 0; w2 < NW; ++w2) {
        const unsigned int n = cur16[w2 * row + T];
        cur16[w2 * row + T] = (unsigned short)run;
        run += n;
      }
    }
  }
  __syncthreads();  // (also orders this workgroup's seg_off stores before a big chunk's reads of them)
  // ---- phase C
  // typed stores under a block-uniform branch (a generic pointer would turn the LDS case into flat_store)
  auto put = [&](unsigned int tile, unsigned int pos, int local, int val) {
    if (staged) stage[pos] = (unsigned short)local;
    else if (!big) point_list[chunk_begin + pos] = val;
    else point_list[seg[tile] + pos] = val;
  };
  // LANE_ORDERED: one ds_add_rtn_u32 on the word of the tile's cursor; the other half of the word is another tile's
  auto bump_raw = [&](unsigned int tile) -> unsigned int {  // the whole word: the tile's cursor is half (tile & 1) of it
    return atomicAdd(&myw[tile >> 1], 1u << ((tile & 1u) * 16u));
  };
  auto bump = [&](unsigned int tile) -> unsigned int { return (bump_raw(tile) >> ((tile & 1u) * 16u)) & 0xffffu; };
  const unsigned long long lt = (1ull << lane) - 1ull;
  // (rolled: the body is large; the preloaded values move down one register per step instead of being indexed)
#pragma unroll 1
  for (int t0 = w_begin; t0 < w_end; t0 += WAVE) {
    const int t = t0 + lane;
    int x0 = 0, y0 = 0, w = 0, h = 0;
    const int id = ii[0];
    const uint32_t r_now = rr[0];
#pragma unroll
    for (int k = 0; k + 1 < CW / WAVE; ++k) {
      rr[k] = rr[k + 1];
      ii[k] = ii[k + 1];
    }
    if (r_now != 0u && !rect_decode(r_now, id, vbase, rec, gx, gy, x0, y0, w, h)) w = h = 0;
    unsigned long long live = __ballot(w * h != 0);
    if (live == 0ull) continue;
    const int Mx = wave_max_i32_dpp(w), My = wave_max_i32_dpp(h);
    const int maxd = max(Mx, My);
    if (maxd <= 8) {
      // The classes are (x mod Mx, y mod My) with the step's exact moduli: the row of Mx classes is a template instance
      // (pos / act stay in registers), the My rows are a rolled loop.
      // all requests of a row of residue classes are issued before the first returned slot is used: Mx LDS atomics in
      // flight instead of one round trip per class (a wave's LDS instructions still execute in issue order)
      auto walk = [&](auto mtag) {
        constexpr int MX = decltype(mtag)::value;
        const int x0m = mod_small(x0, MX), y0m = mod_small(y0, My);
        auto dx_of = [&](int rx) {
          const int d = rx - x0m;
          return d + (d < 0 ? MX : 0);
        };
#pragma unroll 1
        for (int ry = 0; ry < My; ++ry) {
          int dy = ry - y0m;
          dy += dy < 0 ? My : 0;
          const int rowbase = (y0 + dy) * gx + x0;
          const bool vy = dy < h;
          if (LANE_ORDERED) {
            // the first loop only issues: the slot is cut out of the returned word in the second one -- with the shift and
            // mask next to the atomic the compiler waits for every atomic where it is issued (s_waitcnt lgkmcnt(0) + v_bfe
            // under the same exec mask), one LDS round trip per class
            unsigned int raw[MX];
            bool act[MX];
            const int wrow = vy ? w : 0;
#pragma unroll
            for (int rx = 0; rx < MX; ++rx) {
              const int dx = dx_of(rx);
              act[rx] = dx < wrow;
              raw[rx] = 0u;
              if (act[rx]) raw[rx] = bump_raw((unsigned int)(rowbase + dx));
            }
#pragma unroll
            for (int rx = 0; rx < MX; ++rx)
              if (act[rx]) {
                const unsigned int tile = (unsigned int)(rowbase + dx_of(rx));
                put(tile, (raw[rx] >> ((tile & 1u) * 16u)) & 0xffffu, t - c * BIN_CHUNK, id);
              }
          } else {
            for (int rx = 0; rx < MX; ++rx) {
              const int dx = dx_of(rx);
              const bool act = vy && dx < w;
              const unsigned int tile = (unsigned int)(rowbase + dx);
              unsigned long long peers = __ballot(act);
              if (peers == 0ull) continue;
              for (int bit = 0; bit < tile_bits; ++bit) {
                const bool one = (tile >> bit) & 1u;
                const unsigned long long bal = __ballot(one);
                peers &= one ? bal : ~bal;
              }
              if (act) {
                const unsigned int base = my16[tile];
                put(tile, base + (unsigned int)__popcll(peers & lt), t - c * BIN_CHUNK, id);
                if ((peers >> lane) == 1ull) my16[tile] = (unsigned short)(base + (unsigned int)__popcll(peers));  // last lane
              }
              __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
              __builtin_amdgcn_wave_barrier();
              __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
          }
        }
      };
      // Rectangles of 5 .. 8 tiles a side (large images): the residue walk issues 25 .. 64 rounds with a seventh of the lanes
      // active.  Instead every lane lists its own tiles (owner lane << 16 | tile) at its offset in a per-wave LDS list, and the
      // wave then works through the list with all lanes busy: lane i of a round holds instance i -- instances are in (owner,
      // tile) order, so the lanes of one atomic still arrive at a tile's cursor in depth order.
      int n_inst = 0, inc_inst = 0, t_inst = 0x7fffffff;
      if (maxd > 4 && elist_cap > 0) {
        n_inst = w * h;
        inc_inst = wave_incl_scan_add_dpp(n_inst);
        t_inst = __builtin_amdgcn_readlane(inc_inst, WAVE - 1);
      }
      if (t_inst > elist_cap) by_modulus(Mx, walk);  // (sides <= 4, or no list / a step that does not fit it)
      else {
        {
          unsigned int* dst = elist + (inc_inst - n_inst);
          const unsigned int tag = (unsigned int)lane << 16;
          for (int dy = 0; dy < h; ++dy)
            for (int dx = 0; dx < w; ++dx) *dst++ = tag | (unsigned int)((y0 + dy) * gx + x0 + dx);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int i0 = 0; i0 < t_inst; i0 += WAVE) {
          const int i = i0 + lane;
          const bool act = i < t_inst;
          const unsigned int e = act ? elist[i] : 0u;
          const int owner = (int)(e >> 16);
          const unsigned int tile = e & 0xffffu;
          const int oid = __shfl(id, owner, WAVE);
          const int olocal = t0 + owner - c * BIN_CHUNK;
          if (LANE_ORDERED) {
            if (act) put(tile, bump(tile), olocal, oid);
          } else {
            unsigned long long peers = __ballot(act);
            for (int bit = 0; bit < tile_bits; ++bit) {
              const bool one = (tile >> bit) & 1u;
              const unsigned long long bal = __ballot(one);
              peers &= one ? bal : ~bal;
            }
            if (act) {
              const unsigned int base = my16[tile];
              put(tile, base + (unsigned int)__popcll(peers & lt), olocal, oid);
              if ((peers >> lane) == 1ull) my16[tile] = (unsigned short)(base + (unsigned int)__popcll(peers));  // last lane
            }
          }
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
      }
    } else {
      const uint32_t pr = (uint32_t)x0 | ((uint32_t)y0 << 8) | ((uint32_t)w << 16) | ((uint32_t)h << 24);  // gx, gy <= 255
      while (live) {
        const int j = __ffsll((long long)live) - 1;
        live &= live - 1ull;
        const uint32_t sr = (uint32_t)__builtin_amdgcn_readlane((int)pr, j);
        const int sid = __builtin_amdgcn_readlane(id, j);
        const int sx = (int)(sr & 255u), sy = (int)((sr >> 8) & 255u), sw = (int)((sr >> 16) & 255u), sh = (int)(sr >> 24);
        for (int y = 0; y < sh; ++y)
          for (int xb = 0; xb < sw; xb += WAVE)
            if (xb + lane < sw) {
              const unsigned int tile = (unsigned int)((sy + y) * gx + sx + xb + lane);
              if (LANE_ORDERED) {
                put(tile, bump(tile), t0 + j - c * BIN_CHUNK, sid);
              } else {
                // distinct tiles: no two lanes share a slot here (but two may share a word: a 16-bit store each)
                const unsigned int pos = my16[tile];
                my16[tile] = (unsigned short)(pos + 1u);
                put(tile, pos, t0 + j - c * BIN_CHUNK, sid);
              }
            }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      }
    }
  }
  if (!staged) return;
  __syncthreads();
  // ---- phase D: the chunk's block leaves as full coalesced lines
  const int32_t* cid = ids + vbase + (int64_t)c * BIN_CHUNK;
  // (four independent LDS -> gather -> store chains in flight per thread: a rolled loop runs them one after the other)
  int i = threadIdx.x;
  for (; i + 3 * TT < total; i += 4 * TT) {
    const int a0 = cid[stage[i]], a1 = cid[stage[i + TT]], a2 = cid[stage[i + 2 * TT]], a3 = cid[stage[i + 3 * TT]];
    point_list[chunk_begin + i] = a0;
    point_list[chunk_begin + i + TT] = a1;
    point_list[chunk_begin + i + 2 * TT] = a2;
    point_list[chunk_begin + i + 3 * TT] = a3;
  }
  for (; i < total; i += TT) point_list[chunk_begin + i] = cid[stage[i]];
}

// ------------------------------------------------------------------------------------ blend
// Per-tile front-to-back blend.  A 16x16 tile is 16 cells of 4x4 pixels; 16 consecutive lanes own
// one cell, a wave owns a row of four cells.  Per batch of 256 depth-ordered Gaussians:
//   load   thread k gathers Gaussian k's 48-byte record into LDS, computes its exact cutoffs
//          (pc: power below which alpha < 1/255; rc2: squared radius beyond which power < pc) and a
//          16-bit mask of the cells its cutoff circle touches;
//   lists  wave ballots turn the masks into 16 ORDER-PRESERVING index lists (one per cell);
//   blend  every 16-lane group walks ITS OWN list -- lanes of one wave work on different
//          Gaussians in the same instruction (per-lane LDS gathers), so a wave's trip count is
//          the longest of its four cell lists (~1/4 of the batch) instead of the whole batch.
// The cutoffs only skip (pixel, Gaussian) pairs that the reference test `alpha < 1/255` skips,
// and per-pixel order is untouched, so the image stays bit-identical to the oracle.
typedef float f32x2 __attribute__((ext_vector_type(2)));
constexpr int CELL = 4;
constexpr int NCELL = (TILE / CELL) * (TILE / CELL);  // 16

template <typename T>
__device__ __forceinline__ T lds_at(const T* base, unsigned int byte_off) {
  return *reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + byte_off);
}
// fmaxf without the canonicalising v_max(x, x) in front (x is the result of an fma here: never a signalling NaN)
__device__ __forceinline__ float max_f32_raw(float a, float b) {
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

__device__ __forceinline__ float min_f32_raw(float a, float b) {  // fminf, same remark (a NaN operand yields the other one)
  float r;
  asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// One list entry up to alpha, in the oracle's scalar order: dx, dy, q, power, exp_det(power) (or the hardware exponential
// under FAST_EXP, see blend_kernel), opacity * e, min(., 0.99).  a = {px, py, conic x, conic z}, cy = conic y, op = opacity.
template <bool FAST_EXP>
__device__ __forceinline__ float entry_alpha(float4 a, float cy, float op, f32x2 pf, float& power) {
  // {dx, dy} and {cx dx, cz dy} are packed within the entry: their operands already sit in register pairs of the record.
  // The rest is scalar and written as instructions, so that the compiler does not pair it across the two entries of a
  // step (that needs eight v_mov per step to build the register pairs, more VALU cycles than it saves).
  const f32x2 d = f32x2{a.x, a.y} - pf;
  const f32x2 m = f32x2{a.z, a.w} * d;
  float q, t;
  asm("v_mul_f32 %0, %1, %2" : "=v"(q) : "v"(m.y), "v"(d.y));
  asm("v_fma_f32 %0, %1, %2, %0" : "+v"(q) : "v"(m.x), "v"(d.x));         // q = fma(cx dx, dx, (cz dy) dy)
  asm("v_mul_f32 %0, %1, %2" : "=v"(t) : "v"(cy), "v"(d.x));
  asm("v_mul_f32 %0, %0, %1" : "+v"(t) : "v"(d.y));
  asm("v_fma_f32 %0, -0.5, %1, -%2" : "=v"(power) : "v"(q), "v"(t));     // power = fma(-0.5, q, -((cy dx) dy))
  float e;
  if (FAST_EXP) {
    e = __builtin_amdgcn_exp2f(power * 1.44269504088896341f);
  } else {
    // exp_det(): 13 issue slots (the Cephes form of rounds 1 - 5 took 20)
    const float x = max_f32_raw(power, -86.0f);
    const float tm = x * 1.44269504088896341f + 12582912.0f;
    const float f = fmaf(x, 1.44269504088896341f, -(tm - 12582912.0f));
    float pl = fmaf(1.3264815788716078e-3f, f, 9.671512059867382e-3f);
    pl = fmaf(pl, f, 5.550733581185341e-2f);
    pl = fmaf(pl, f, 2.4022242426872253e-1f);
    pl = fmaf(pl, f, 6.931470036506653e-1f);
    pl = fmaf(pl, f, 1.0f);
    e = __uint_as_float(__float_as_uint(pl) + (__float_as_uint(tm) << 23));
  }
  return min_f32_raw(op * e, 0.99f);
}

// FAST_EXP: alpha = opacity * 2^(power * log2 e) on the hardware exponential (v_exp_f32, 1 ulp) instead of the oracle's
// deterministic polynomial exp_det() -- 2 issue slots per entry instead of 13.  The image is no longer bit-equal
// to oracle/rasterizer_oracle.c but stays within 1e-5 relative of it (tests/test_gpu_rasterizer_fast.py); opt-in
// (GR_RASTER_FAST_EXP flag of gr_raster_render_ex).
// KEEP (the autograd forward, gr_raster_render_keep): out_color is followed in the same allocation by the per-pixel final
// transmittance [V][H][W] (fp32) and n_contrib [V][H][W] (int32) = 1 + the index of the last blended entry in the tile's
// concatenated list (0 = none) -- the state rasterizer_backward.hip starts from.  (No extra kernel argument: the
// instances without KEEP keep their kernel-argument layout and compile to the instruction stream they had before.)
// AUX (gr_raster_render_aux): the walk also accumulates depth = sum w_i z_i (z_i: the view-space depth preprocess stored in
// rec[3].y), with the red channel's operation (D = fma(z, w, D)), and writes it and alpha = 1 - T beside the colour.  z is
// one more 4-byte plane s_z (entry e at byte 4 e, read with a ds_read_b32 only where the entry blends: the 16 lanes of a
// cell read one address): 20 368 bytes of LDS per workgroup, still 8 workgroups per CU.  The output pointers travel in
// BlendAux, which is empty without AUX: those instances keep their kernel arguments, their LDS and their instruction
// stream.  With AUX the kept state (KEEP) goes to aux.state (final_T, then n_contrib) instead of behind the colour.
template <bool AUX>
struct BlendAux {};  // (without AUX: the kernel-argument segment keeps its size)
template <>
struct BlendAux<true> {
  float* depth;  // [V][H][W]
  float* alpha;  // [V][H][W]
  float* state;  // final_T [V][H][W], n_contrib [V][H][W]; read only with KEEP
};

template <bool FAST_EXP, bool KEEP = false, bool AUX = false>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(8, 8))) void blend_kernel(
    int P, int W, int H, int nchunk, const DevView* __restrict__ views, const uint32_t* __restrict__ seg_off,
    const int32_t* __restrict__ point_list, const float4* __restrict__ rec, float* __restrict__ out_color,
    unsigned int list_cap, BlendAux<AUX> aux) {
  // One 40-byte record per entry, in three arrays, so that the walk reads an entry with two ds_read_b128 and one
  // ds_read_b64 (10 LDS-array cycles per wave) instead of ten ds_read_b32 (20):
  //   s_ga[e] = {px, py, conic x, conic z}   s_gb[e] = {conic y, opacity, power cutoff, red}   s_gc[e] = {green, blue}
  // Entry e sits at byte 16 e of s_ga / s_gb and 8 e of s_gc.  (Two entries read by one lane group of a ds_read_b128
  // share a bank only when their indices agree mod 16.)  Same 10 280 bytes as ten 257-entry planes: 8 workgroups per CU.
  __shared__ float4 s_ga[BLOCK + 1], s_gb[BLOCK + 1];
  __shared__ f32x2 s_gc[BLOCK + 1];
  __shared__ float s_z[AUX ? BLOCK + 1 : 1];  // AUX only: view-space depth of the entry (without AUX: never touched, no LDS)
  __shared__ unsigned short s_list[NCELL][BLOCK + 2];                   // byte offsets (16 * entry) into s_ga / s_gb
  __shared__ int s_cnt[NCELL][BLOCK / WAVE];      // per (cell, loading wave) counts
  __shared__ int s_alldone[BLOCK / WAVE];
  __shared__ int s_wpre[WAVE];                    // window of 64 chunks: inclusive prefix of this tile's segment lengths
  __shared__ unsigned int s_woff[WAVE];           //                      and where each segment starts in point_list
  const int gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE;
  // speculative launch: the list was sized before the instance count was known; if it is too short nothing is drawn (the
  // host repeats the render).  The grand total is the end of the last segment of the last view.
  if (list_cap != 0xffffffffu && nchunk > 0 &&
      seg_off[(int64_t)gridDim.z * nchunk * (gx * gy + 1) - 1] > list_cap) return;
  const int v = blockIdx.z;
  const int tile = blockIdx.y * gx + blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1), lw = tid / WAVE;
  const int cell = tid / (CELL * CELL), pin = tid % (CELL * CELL);
  const int lx = (cell % (TILE / CELL)) * CELL + pin % CELL;
  const int ly = (cell / (TILE / CELL)) * CELL + pin / CELL;
  const int pxi = blockIdx.x * TILE + lx, pyi = blockIdx.y * TILE + ly;
  const bool inside = pxi < W && pyi < H;
  const f32x2 pf = {(float)pxi, (float)pyi};
  const float tx0 = (float)(blockIdx.x * TILE), ty0 = (float)(blockIdx.y * TILE);
  const int tiles = gx * gy;
  const int64_t goff = (int64_t)v * P;
  bool done = !inside;
  // entry BLOCK: the pad entry of odd-length lists.  Cutoff +inf: `power < pc` holds, it never blends.
  if (tid == 0) {
    s_ga[BLOCK] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    s_gb[BLOCK] = make_float4(0.0f, 0.0f, INFINITY, 0.0f);
    s_gc[BLOCK] = f32x2{0.0f, 0.0f};
    if (AUX) s_z[BLOCK] = 0.0f;
  }
  float T = 1.0f, C0 = 0.f, Dz = 0.f;
  f32x2 C12 = {0.f, 0.f};
  // The tile's list = its segments of chunk 0, 1, 2, ... (depth order).  64 chunks are looked up at a time (one wave:
  // lane = chunk, two 4-byte loads give segment start and end); the batches of 256 entries are cut out of that window.
  int c_next = 0, w_pos = 0, w_total = 0;  // block-uniform
  int list_base = 0, batch_base = 0, last = 0;  // KEEP: where the window / the batch start in the tile's list; per pixel
  const uint32_t* seg_col = seg_off + (int64_t)v * nchunk * (tiles + 1) + tile;
  while (true) {
    // all 256 pixels saturated?  One ballot per wave, one flag per wave, one barrier (the later barriers of the batch
    // separate this read from the next write)
    const unsigned long long live = __ballot(!done);
    if (lane == 0) s_alldone[lw] = live == 0ull ? 1 : 0;
    __syncthreads();
    if (s_alldone[0] & s_alldone[1] & s_alldone[2] & s_alldone[3]) break;
    bool exhausted = false;
    while (w_pos >= w_total) {
      if (c_next >= nchunk) {
        exhausted = true;
        break;
      }
      if (tid < WAVE) {
        const int c = c_next + tid;
        unsigned int a = 0u, b = 0u;
        if (c < nchunk) {
          a = seg_col[(int64_t)c * (tiles + 1)];
          b = seg_col[(int64_t)c * (tiles + 1) + 1];
        }
        s_woff[tid] = a;
        s_wpre[tid] = wave_incl_scan_add_dpp((int)(b - a));
      }
      __syncthreads();
      if (KEEP) list_base += w_total;
      w_total = s_wpre[WAVE - 1];
      w_pos = 0;
      c_next += WAVE;
      __syncthreads();
    }
    if (exhausted) break;
    // ---- load + cutoffs + cell mask
    const int e = w_pos + tid;
    if (KEEP) batch_base = list_base + w_pos;
    w_pos += BLOCK;
    // reach[c]: the lanes of this wave whose entry can reach cell c -- 16 lane masks in scalar registers.  The rank of an
    // entry in a cell's list is a masked bit count of that mask and the list write runs under it as the exec mask
    // (inverse ballot): no per-lane bit field is built or taken apart.
    float ctr_x = 0.0f, ctr_y = 0.0f, rc2 = -1.0f, hx2 = 0.0f, hy2 = 0.0f;  // past the end of the list: reaches no cell
    if (e < w_total) {
      int lo = 0;  // first chunk of the window whose inclusive prefix exceeds e
#pragma unroll
      for (int st = WAVE / 2; st > 0; st >>= 1)
        if (s_wpre[lo + st - 1] <= e) lo += st;
      const int before = lo ? s_wpre[lo - 1] : 0;
      const float4* r = rec + 4 * (goff + point_list[s_woff[lo] + (unsigned int)(e - before)]);
      const float4 r0 = r[0];
      const float4 co = r[1];
      const float4 col = r[2];
      // Exact skip rules (they only ever skip what the reference test `alpha < 1/255` skips):
      //   power < pc = -ln(255 op) - 1e-3   ==>   op * exp(power) < 1/255
      //   |d|^2 > |pc| * col.w              ==>   power < pc            (see preprocess)
      // NaN / non-positive opacity make every comparison false: nothing is skipped early.
      const float pc = -__logf(255.0f * co.w) - 1.0e-3f;
      rc2 = -pc * col.w;
      // exact level set of the quadratic form, per axis (see preprocess): c' = |pc| + 2e-6 rc2 covers the fp32 error
      const float cpr = -pc + 1.0e-3f + 2.0e-6f * rc2;
      hx2 = cpr * r0.z;
      hy2 = cpr * r0.w;
      ctr_x = r0.x;
      ctr_y = r0.y;
      s_ga[tid] = make_float4(r0.x, r0.y, co.x, co.z);
      s_gb[tid] = make_float4(co.y, co.w, pc, col.x);
      s_gc[tid] = f32x2{col.y, col.z};
      if (AUX) s_z[tid] = r[3].y;
    }
    float ex2[TILE / CELL], ey2[TILE / CELL];
    bool xin[TILE / CELL], yin[TILE / CELL];
#pragma unroll
    for (int c = 0; c < TILE / CELL; ++c) {
      const float xlo = tx0 + (float)(c * CELL), ylo = ty0 + (float)(c * CELL);
      const float ex = fmaxf(fmaxf(xlo - ctr_x, ctr_x - (xlo + (float)(CELL - 1))), 0.0f);
      const float ey = fmaxf(fmaxf(ylo - ctr_y, ctr_y - (ylo + (float)(CELL - 1))), 0.0f);
      ex2[c] = ex * ex;
      ey2[c] = ey * ey;
      xin[c] = !(ex2[c] > hx2);
      yin[c] = !(ey2[c] > hy2);
    }
    // ---- order-preserving per-cell lists
    unsigned long long reach[NCELL];
    int cnt_lane = 0;  // lane c: how many entries of this wave reach cell c
#pragma unroll
    for (int c = 0; c < NCELL; ++c) {
      reach[c] = __ballot(!(ex2[c % (TILE / CELL)] + ey2[c / (TILE / CELL)] > rc2) && xin[c % (TILE / CELL)] &&
                          yin[c / (TILE / CELL)]);
      asm("v_writelane_b32 %0, %1, %2" : "+v"(cnt_lane) : "s"((int)__popcll(reach[c])), "n"(c));
    }
    if (lane < NCELL) s_cnt[lane][lw] = cnt_lane;
    __syncthreads();
    // every wave adds up the four per-wave counts itself (lane c: cell c) -- no second barrier for a 16-thread scan
    int base_lane = 0, tot_lane = 0;  // lane c: where this wave's entries start in list c; the list's length
    if (lane < NCELL) {
#pragma unroll
      for (int w = 0; w < BLOCK / WAVE; ++w) {
        const int n = s_cnt[lane][w];
        base_lane += w < lw ? n : 0;
        tot_lane += n;
      }
      // lists are walked in pairs: pad an odd one with the never-hit entry
      if (lw == 0 && (tot_lane & 1)) s_list[lane][tot_lane] = (unsigned short)(16 * BLOCK);
    }
#pragma unroll
    for (int c = 0; c < NCELL; ++c) {
      const int base = __builtin_amdgcn_readlane(base_lane, c);
      const unsigned int rank = __builtin_amdgcn_mbcnt_hi((unsigned int)(reach[c] >> 32),
                                                          __builtin_amdgcn_mbcnt_lo((unsigned int)reach[c], 0u));
      if (__builtin_amdgcn_inverse_ballot_w64(reach[c])) s_list[c][base + rank] = (unsigned short)(16 * tid);
    }
    __syncthreads();
    // ---- blend: each 16-lane group walks its own list
    const int len_cell = __shfl(tot_lane, (BLOCK / WAVE) * lw + lane / (CELL * CELL));  // cell = 4 lw + lane / 16
    const int n_cell = done ? 0 : len_cell;
    // Two list entries per step, each read as {px, py, cx, cz} + {cy, op, pc, r} + {g, b} and evaluated
    // on its own registers: dx, dy, q, power, the exponential and alpha are the oracle's scalar sequence per entry (the
    // compiler may pack the two entries' independent operations); only the order-dependent tail (transmittance test,
    // colour accumulation) is serial.
    // The next step's two offsets are read one step ahead (one 4-byte read per step; the row holds BLOCK + 2 of them,
    // so the read after the last step stays inside it), and the step's record reads do not wait behind the list read.
    const unsigned int* lp = reinterpret_cast<const unsigned int*>(&s_list[cell][0]);
    unsigned int pair = lp[0];
    for (int i = 0; i < n_cell && !done; i += 2) {
      const unsigned int o0 = pair & 0xffffu, o1 = pair >> 16;  // byte offsets of two entries (an odd list ends with the pad entry)
      pair = lp[i / 2 + 1];
      const float4 a0 = lds_at(s_ga, o0), b0 = lds_at(s_gb, o0);
      const float4 a1 = lds_at(s_ga, o1), b1 = lds_at(s_gb, o1);
      // {g, b} of both entries are read here, with the records, and not where an entry blends: the serial tail of the
      // step then holds no LDS read and no wait for one (z, AUX only, stays under the branch: the instance with AUX
      // and KEEP has no register left for it).
      const f32x2 c0 = lds_at(s_gc, o0 / 2), c1 = lds_at(s_gc, o1 / 2);
      // red and the cutoff are not used up to alpha: without this the compiler splits {cy, op, pc, r} into a ds_read_b64
      // and a ds_read_b32 instead of one ds_read_b128
      asm volatile("" ::"v"(b0.w), "v"(b1.w), "v"(b0.z), "v"(b1.z));
      float power0, power1;
      const float alpha0 = entry_alpha<FAST_EXP>(a0, b0.x, b0.y, pf, power0);
      const float alpha1 = entry_alpha<FAST_EXP>(a1, b1.x, b1.y, pf, power1);
      // the colours have arrived by now: the wait for them stands here, once, in front of the two predicated regions
      asm volatile("" ::"v"(c0.x), "v"(c0.y), "v"(c1.x), "v"(c1.y), "v"(alpha0), "v"(alpha1));
      // The oracle's two tests.  The cutoff `power < pc` is not tested here: it only ever skips what `alpha < 1/255` skips
      // (see the load above), alpha is computed either way, and the pad entry (opacity 0) has alpha = 0.
      const bool ok0 = !(power0 > 0.0f) && !(alpha0 < 1.0f / 255.0f);
      const bool ok1 = !(power1 > 0.0f) && !(alpha1 < 1.0f / 255.0f);
      // A pixel that saturates leaves the walk through the loop condition, not through a `break`: the wave's control flow
      // stays one counted loop with two predicated regions.
      if (ok0) {
        const float test_T = T * (1.0f - alpha0);
        if (test_T < 0.0001f) {
          done = true;
        } else {
          const float w = alpha0 * T;
          C0 = fmaf(b0.w, w, C0);
          C12 = __builtin_elementwise_fma(c0, f32x2{w, w}, C12);
          if (AUX) Dz = fmaf(lds_at(s_z, o0 / 4), w, Dz);
          T = test_T;
          if (KEEP) last = batch_base + (int)(o0 / 16) + 1;
        }
      }
      if (ok1 && !done) {
        const float test_T = T * (1.0f - alpha1);
        if (test_T < 0.0001f) {
          done = true;
        } else {
          const float w = alpha1 * T;
          C0 = fmaf(b1.w, w, C0);
          C12 = __builtin_elementwise_fma(c1, f32x2{w, w}, C12);
          if (AUX) Dz = fmaf(lds_at(s_z, o1 / 4), w, Dz);
          T = test_T;
          if (KEEP) last = batch_base + (int)(o1 / 16) + 1;
        }
      }
    }
  }
  if (inside) {
    const DevView& cam = views[v];
    float* o = out_color + (int64_t)v * 3 * H * W + (int64_t)pyi * W + pxi;
    o[0] = fmaf(T, cam.bg[0], C0);
    o[(int64_t)H * W] = fmaf(T, cam.bg[1], C12.x);
    o[2 * (int64_t)H * W] = fmaf(T, cam.bg[2], C12.y);
    if constexpr (AUX) {
      const int64_t q = ((int64_t)v * H + pyi) * W + pxi;
      aux.depth[q] = Dz;
      aux.alpha[q] = 1.0f - T;
    }
    if (KEEP) {
      const int64_t q = ((int64_t)v * H + pyi) * W + pxi, hw = (int64_t)gridDim.z * H * W;
      if constexpr (AUX) {
        aux.state[q] = T;
        reinterpret_cast<int32_t*>(aux.state)[hw + q] = last;
      } else {
        out_color[3 * hw + q] = T;                                                      // final_T
        reinterpret_cast<int32_t*>(out_color)[4 * hw + q] = last;                       // n_contrib
      }
    }
  }
}

__global__ __launch_bounds__(256) void mark_visible_kernel(int P, const float* __restrict__ means3D,
                                                           float v2, float v6, float v10, float v14,
                                                           uint8_t* __restrict__ present) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P) return;
  const float z = fmaf(v2, means3D[3 * (int64_t)i],
                       fmaf(v6, means3D[3 * (int64_t)i + 1], fmaf(v10, means3D[3 * (int64_t)i + 2], v14)));
  present[i] = z > 0.2f ? 1 : 0;
}

int check_views(const gr_raster_view* h_views, int num_views) {
  GR_REQUIRE(h_views != nullptr && num_views >= 1, "need at least one view");
  GR_REQUIRE(num_views <= MAX_VIEWS, "at most %d views per call (got %d)", MAX_VIEWS, num_views);
  for (int v = 0; v < num_views; ++v) {
    GR_REQUIRE(h_views[v].image_width == h_views[0].image_width &&
                   h_views[v].image_height == h_views[0].image_height &&
                   h_views[v].sh_degree == h_views[0].sh_degree,
               "all views of one call must share image size and sh_degree");
    GR_REQUIRE(h_views[v].image_width > 0 && h_views[v].image_height > 0, "bad image size");
    GR_REQUIRE(h_views[v].sh_degree >= 0 && h_views[v].sh_degree <= 3, "sh_degree must be 0..3");
  }
  return GR_OK;
}

// ------------------------------------------------------------------------------------ self-check of the ordered outputs
// The depth sort and the tile scatter take their stable ranks from the lane order of LDS atomics (a measured property of
// the device, common.hip).  The first frames of a process are therefore CHECKED on the device: depth order (ties: id) of
// every view, and every (chunk, tile) segment of the point list in depth order.  A failure demotes the device to explicit
// ballot ranking and the stage is redone.  GR_RASTER_VERIFY=1 checks every frame.
__global__ __launch_bounds__(256) void verify_depth_order_kernel(int P, int V, const int32_t* __restrict__ nvis,
                                                                 const uint32_t* __restrict__ dfield,
                                                                 const int32_t* __restrict__ ids, int32_t* __restrict__ rank,
                                                                 int* __restrict__ bad) {
  const int v = blockIdx.y;
  const int n = nvis[v];
  const int64_t o = (int64_t)v * P;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const int a = ids[o + i];
    rank[o + a] = i;
    if (i + 1 < n) {
      const int b = ids[o + i + 1];
      const uint32_t fa = dfield[o + a], fb = dfield[o + b];
      if (fa > fb || (fa == fb && a >= b)) atomicOr(bad, 1);
    }
  }
}

__global__ __launch_bounds__(256) void verify_tile_lists_kernel(int P, int V, int nchunk, int tiles,
                                                                const uint32_t* __restrict__ seg_off,
                                                                const int32_t* __restrict__ point_list,
                                                                const int32_t* __restrict__ rank, int* __restrict__ bad) {
  const int v = blockIdx.x / nchunk;
  const uint32_t* seg = seg_off + (int64_t)blockIdx.x * (tiles + 1);
  const int32_t* rk = rank + (int64_t)v * P;
  for (int t = threadIdx.x; t < tiles; t += 256) {
    int prev = -1;
    for (uint32_t e = seg[t]; e < seg[t + 1]; ++e) {
      const int r = rk[point_list[e]];
      if (r <= prev) atomicOr(bad, 2);
      prev = r;
    }
  }
}

}  // namespace
}  // namespace gr

namespace gr {
namespace {
std::atomic<int> g_frames[64];  // frames rendered per device

// The lane-ordered ranking (one ds_add_rtn per key, equal-address lanes served in lane order) rests on a measured property of
// the LDS, not on an architectural guarantee: besides the probe (common.hip), the REAL outputs of a frame -- every view's
// depth order, every per-tile list -- are checked on the device for the first three frames of a process and device and
// again on one frame in every 256 from then on (other occupancy, clocks or partition mode later in the life of a process
// would otherwise go unnoticed); a failed check demotes the process to ballot ranking and renders the frame again.
// GR_RASTER_VERIFY=1 checks every frame.
bool verify_this_frame() {
  static const bool always = getenv("GR_RASTER_VERIFY") && getenv("GR_RASTER_VERIFY")[0] == '1';
  if (lds_atomics_lane_ordered_state() != 1) return always;  // ballot ranking needs no such check (but may be asked for)
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 63;
  const int f = g_frames[dev].load();
  return always || f < 3 || (f & 255) == 0;
}

// calls left before the bucket depth sort (depth_sort.hip) is tried again after one of its buckets overflowed (a scene whose
// depths crowd into a sliver of the key range: every frame would be ordered twice); per host thread
thread_local int g_bucket_cooldown = 0;
constexpr int BUCKET_COOLDOWN_FRAMES = 256;
// One call of the waiting period.  The unit is library calls that COULD have used the bucket sort (`possible`), of few views
// or of many: a call the sort cannot serve (too many Gaussians for its id field) does not run the period down.
bool bucket_sort_allowed(bool possible) {
  if (!possible) return false;
  if (g_bucket_cooldown == 0) return true;
  --g_bucket_cooldown;
  return false;
}
void bucket_sort_overflowed() { g_bucket_cooldown = BUCKET_COOLDOWN_FRAMES; }

void frame_done() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 63;
  g_frames[dev].fetch_add(1);
}

// runs `launch_check(d_flag)` (which enqueues the check kernels), waits, returns the flag word
template <typename F>
int device_check(hipStream_t stream, F&& launch_check, int* h_flag) {
  int* d_bad = nullptr;
  GR_HIP(hipMallocAsync(reinterpret_cast<void**>(&d_bad), sizeof(int), stream));
  GR_HIP(hipMemsetAsync(d_bad, 0, sizeof(int), stream));
  launch_check(d_bad);
  GR_HIP(hipMemcpyAsync(h_flag, d_bad, sizeof(int), hipMemcpyDeviceToHost, stream));
  GR_HIP(hipStreamSynchronize(stream));
  GR_HIP(hipFreeAsync(d_bad, stream));
  return GR_OK;
}

// One host-to-device copy: the depth-overflow flag (cleared) and the camera table that follows it in the geometry buffer
// (Geom::totals layout).  The pinned staging buffer must stay untouched until the caller has synchronised the stream / event.
// Up to four cameras travel as KERNEL ARGUMENTS: a one-wave kernel writes the cleared flag words and the DevView records.
// (An H2D copy of the same 200 bytes occupies the stream for 4.6 us in front of every one-camera frame -- copy engine
// hand-over; the kernel costs a launch boundary.)  More cameras: one copy out of pinned staging, as before.
constexpr int VIEW_PACK = 4;
struct ViewPack {
  DevView v[VIEW_PACK];
};
__global__ void upload_views_kernel(ViewPack pack, int num_views, int32_t* __restrict__ d_flag) {
  const int t = threadIdx.x;
  if (t < 4) d_flag[t] = 0;
  constexpr int WORDS = sizeof(DevView) / 4;
  float* dst = reinterpret_cast<float*>(d_flag + 4);
  const float* src = reinterpret_cast<const float*>(&pack);
  for (int i = t; i < num_views * WORDS; i += blockDim.x) dst[i] = src[i];
}

static void fill_view(DevView& d, const gr_raster_view& s) {
  memcpy(d.view, s.viewmatrix, sizeof(d.view));
  memcpy(d.proj, s.projmatrix, sizeof(d.proj));
  memcpy(d.campos, s.campos, sizeof(d.campos));
  memcpy(d.bg, s.bg, sizeof(d.bg));
  d.tanx = s.tanfovx;
  d.tany = s.tanfovy;
  d.fx = (float)s.image_width / (2.0f * s.tanfovx);
  d.fy = (float)s.image_height / (2.0f * s.tanfovy);
  d.scale_mod = s.scale_modifier;
}

int upload_views(const gr_raster_view* h_views, int num_views, int32_t* d_flag, hipStream_t stream) {
  static_assert(sizeof(DevView) % 4 == 0, "DevView is copied word by word");
  if (num_views <= VIEW_PACK) {
    ViewPack pack;
    memset(&pack, 0, sizeof(pack));
    for (int v = 0; v < num_views; ++v) fill_view(pack.v[v], h_views[v]);
    hipLaunchKernelGGL(upload_views_kernel, dim3(1), dim3(WAVE), 0, stream, pack, num_views, d_flag);
    GR_LAUNCH_CHECK();
    return GR_OK;
  }
  char* raw = static_cast<char*>(pinned_scratch(0, 16 + sizeof(DevView) * num_views));
  GR_REQUIRE(raw != nullptr, "pinned staging buffer for %d views could not be allocated", num_views);
  memset(raw, 0, 16);
  DevView* stage = reinterpret_cast<DevView*>(raw + 16);
  for (int v = 0; v < num_views; ++v) fill_view(stage[v], h_views[v]);
  GR_HIP(hipMemcpyAsync(d_flag, raw, 16 + sizeof(DevView) * num_views, hipMemcpyHostToDevice, stream));
  return GR_OK;
}

}  // namespace
}  // namespace gr

using namespace gr;

static int64_t tiles_of(int width, int height) {
  return (int64_t)((width + TILE - 1) / TILE) * ((height + TILE - 1) / TILE);
}

extern "C" int gr_raster_lds_atomics_lane_ordered(void) { return lds_atomics_lane_ordered_state(); }
extern "C" int gr_raster_ballot_ranking(int on) { return lds_ballot_ranking_force(on); }

extern "C" size_t gr_raster_geom_bytes(int64_t P, int num_views, int width, int height) {
  if (P < 0 || num_views < 1 || width <= 0 || height <= 0) return 0;
  return carve_geom(nullptr, P, num_views, tiles_of(width, height)).bytes;
}

extern "C" int gr_raster_debug_geom_layout(int64_t P, int num_views, int width, int height, int64_t* h_offsets) {
  GR_REQUIRE(P >= 0 && num_views >= 1 && width > 0 && height > 0 && h_offsets != nullptr, "bad argument");
  char* const origin = reinterpret_cast<char*>(uintptr_t(1) << 32);  // never dereferenced: the carver only adds to it
  const Geom g = carve_geom(origin, P, num_views, tiles_of(width, height));
  h_offsets[0] = reinterpret_cast<char*>(g.dfield) - origin;
  h_offsets[1] = reinterpret_cast<char*>(g.order_b) - origin;
  h_offsets[2] = reinterpret_cast<char*>(g.rects) - origin;
  h_offsets[3] = reinterpret_cast<char*>(g.nvis) - origin;
  return 4;
}

extern "C" size_t gr_raster_bin_bytes(int64_t total_rendered, int width, int height, int num_views) {
  if (total_rendered < 0 || width <= 0 || height <= 0 || num_views < 1) return 0;
  return carve_bin(nullptr, total_rendered, tiles_of(width, height) * num_views).bytes;
}

// What travels between the two halves of a deferred (speculative) frame: its plan (raster_plan.hpp -- which launches count,
// whether the counts come by mail or behind the event, what the scatter reads) and what the wait for the counts needs.
struct Deferred {
  hipEvent_t ev;           // Transport::Event: follows the copy of the counts on the side stream
  volatile int32_t* mail;  // Transport::Mail: the words the counting kernel posts (null: this thread has no mailbox)
  int seq;                 // this frame's stamp (never 0)
  int far_seq;             // what a far depth leaves in the far word (a bucket overflow: its negative)
  FramePlan plan;
};

// the caller's arrays of one preprocess call
struct SceneArgs {
  int64_t P;
  int M;
  const float *means3D, *shs, *colors_precomp, *opacities, *scales, *rotations, *cov3D_precomp;
  int32_t* radii;
};

using PreprocessFn = decltype(&preprocess_kernel<false, false, false, false>);
static PreprocessFn preprocess_fn(bool has_sh, bool has_cov, bool sh16, PreprocessKind kind) {
  // rows (HAS_SH, HAS_COV, SH16); columns: PreprocessKind Late (a plan asks for it on SH16 rows only), Many, Plain
  static const PreprocessFn table[6][3] = {
      {preprocess_kernel<true, true, true, true>, preprocess_many_kernel<true, true, true>, preprocess_kernel<true, true, true, false>},
      {preprocess_kernel<true, true, false, false>, preprocess_many_kernel<true, true, false>, preprocess_kernel<true, true, false, false>},
      {preprocess_kernel<true, false, true, true>, preprocess_many_kernel<true, false, true>, preprocess_kernel<true, false, true, false>},
      {preprocess_kernel<true, false, false, false>, preprocess_many_kernel<true, false, false>, preprocess_kernel<true, false, false, false>},
      {preprocess_kernel<false, true, false, false>, preprocess_many_kernel<false, true, false>, preprocess_kernel<false, true, false, false>},
      {preprocess_kernel<false, false, false, false>, preprocess_many_kernel<false, false, false>, preprocess_kernel<false, false, false, false>}};
  const int row = has_sh ? (has_cov ? 0 : 2) + (sh16 ? 0 : 1) : has_cov ? 4 : 5;
  return table[row][kind == PreprocessKind::Late ? 0 : kind == PreprocessKind::Many ? 1 : 2];
}

static int launch_preprocess(const FramePlan& plan, const SceneArgs& a, int D, int W, int H, const Geom& g, const DevView& cam1,
                             int far_seq, hipStream_t stream) {
  const dim3 blk(256), grd((unsigned)((a.P + 255) / 256));
  {
    KernelTimer timer("raster_preprocess", stream);
    hipLaunchKernelGGL(preprocess_fn(a.shs != nullptr, a.cov3D_precomp != nullptr, plan.sh16, plan.preprocess), grd, blk, 0, stream,
                       (int)a.P, D, a.M, plan.V, g.views, a.means3D, a.shs, a.colors_precomp, a.opacities, a.scales, a.rotations,
                       a.cov3D_precomp, W, H, a.radii, g.rec, g.dfield, g.rect_raw, g.totals + 2 * plan.V, cam1, far_seq,
                       plan.msd ? g.key_mm : nullptr);
  }
  GR_LAUNCH_CHECK();
  return GR_OK;
}

// The counts on their way to the host.  Sync: they are in `tot` on return.  Event: a device-to-host copy on a SIDE stream,
// so the scatter and the blend that follow on `stream` do not queue behind it (it held the stream for 4.2 us + a 5.7 us
// hand-over gap, profiles/r03_single_view_timeline.txt).  Mail: nothing to do, the counting kernel mails them itself.
static int send_counts(const FramePlan& plan, const Geom& g, int32_t* tot, hipStream_t stream, const Deferred* d) {
  if (plan.transport == Transport::Mail) return GR_OK;
  const int V = plan.V;
  hipStream_t via = stream;
  if (plan.transport == Transport::Event) {
    static thread_local hipStream_t side = nullptr;
    static thread_local hipEvent_t counted = nullptr;
    if (side == nullptr) GR_HIP(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
    if (counted == nullptr) GR_HIP(hipEventCreateWithFlags(&counted, hipEventDisableTiming));
    GR_HIP(hipEventRecord(counted, stream));
    GR_HIP(hipStreamWaitEvent(side, counted, 0));
    via = side;
  }
  GR_HIP(hipMemcpyAsync(tot, g.totals, sizeof(int32_t) * (2 * V + 1), hipMemcpyDeviceToHost, via));
  if (!plan.short_rows) GR_HIP(hipMemcpyAsync(tot + 2 * V + 1, g.chunk_max, sizeof(int32_t), hipMemcpyDeviceToHost, via));
  if (plan.transport == Transport::Event)
    GR_HIP(hipEventRecord(d->ev, via));
  else
    GR_HIP(hipStreamSynchronize(stream));
  return GR_OK;
}

// Every view's visible Gaussians in depth order (ties: Gaussian id): ids -> order_b, rectangles -> rects.  Then the count
// launches of plan.route (DESIGN.md 3.3 has the table), and the counts on their way by plan.transport.
// d: the deferred frame this is the first half of (null: a plain frame).
static int sort_and_count(const FramePlan& plan, const Geom& g, int64_t P, int32_t* tot, hipStream_t stream, const Deferred* d) {
  const int V = plan.V, nchunk = plan.nchunk, tiles = plan.tiles;
  {
    KernelTimer timer("raster_depth_sort", stream);
    // a bucket that outgrows LDS raises the far word: bit 1 on a plain frame (which reads the counts itself and redoes the
    // ordering in place), the negative stamp on a deferred one (whose caller then takes the plain path)
    const DepthSortTotals ct{g.chunk_total, BIN_CHUNK, nchunk, g.rec, plan.gx, plan.gy};
    int rc = depth_sort_views(g.dfield, g.rect_raw, g.keys_a, g.keys_b, g.order_b, g.rects, g.nvis, P, V, plan.key_bits,
                              g.ds_table, g.ds_table_bytes, stream, plan.msd ? g.key_mm : nullptr,
                              V > 4 ? (int)((P + 255) / 256) * (256 / WAVE) : (int)((P + 255) / 256), g.totals + 2 * V,
                              d != nullptr ? -d->far_seq : 2,
                              plan.route == CountRoute::SelfRaw || plan.totals_sorted ? &ct : nullptr);
    if (rc != GR_OK) return rc;
  }
  if (plan.route == CountRoute::SelfRaw) return GR_OK;
  {
    KernelTimer timer("raster_bin", stream);
    // chunk bases inside each view (+ the per-view totals R_v and the largest chunk total, which sizes the scatter's
    // staging block), and every chunk's per-tile segment starts
    if (plan.route == CountRoute::CountScan) {
      if (tiles * sizeof(unsigned int) > 64 * 1024)
        GR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(tile_count_kernel),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      hipLaunchKernelGGL(tile_count_kernel, dim3((unsigned)bin_grid(V, nchunk)), dim3(BIN_T), tiles * sizeof(unsigned int),
                         stream, (int)P, V, plan.gx, plan.gy, nchunk, g.nvis, g.rects, g.order_b, g.rec, g.chunk_cnt,
                         g.chunk_total);
      const bool mail = plan.transport == Transport::Mail;
      hipLaunchKernelGGL(seg_scan_kernel<true>, dim3((unsigned)(V * nchunk)), dim3(256), 0, stream, V, tiles, nchunk,
                         g.chunk_cnt, g.chunk_total, g.totals, g.seg_off, mail ? const_cast<int32_t*>(d->mail) : nullptr,
                         mail ? d->seq : 0);
      GR_LAUNCH_CHECK();
    } else {
      if (!plan.totals_sorted)
        hipLaunchKernelGGL(chunk_total_kernel, dim3((unsigned)bin_grid(V, nchunk)), dim3(BIN_T), 0, stream, (int)P, V, plan.gx,
                           plan.gy, nchunk, g.nvis, g.rects, g.order_b, g.rec, g.chunk_total);
      if (!plan.short_rows)
        hipLaunchKernelGGL(chunk_max_kernel, dim3(1), dim3(1024), 0, stream, V * nchunk, g.chunk_total, g.chunk_max);
      GR_LAUNCH_CHECK();
      int rc = exclusive_scan_i32(g.chunk_total, g.chunk_total + (int64_t)V * nchunk, nchunk, V, nchunk, g.scan_ws, g.totals,
                                  stream, nullptr, plan.short_rows ? g.totals + V : nullptr);
      if (rc != GR_OK) return rc;
    }
  }
  return send_counts(plan, g, tot, stream, d);
}

// first frames of the process: is every view really in (depth, id) order?  1: it was not, and the process now ranks by ballot
static int check_depth_order(int64_t P, int V, const Geom& g, hipStream_t stream) {
  if (!verify_this_frame()) return GR_OK;
  int h_bad = 0;
  int rc = device_check(stream, [&](int* d_bad) {
    hipLaunchKernelGGL(verify_depth_order_kernel, dim3((unsigned)std::min<int64_t>((P + 255) / 256, 4096), V), dim3(256), 0,
                       stream, (int)P, V, g.nvis, g.dfield, g.order_b, reinterpret_cast<int32_t*>(g.keys_a), d_bad);
  }, &h_bad);
  if (rc != GR_OK) return rc;
  if (h_bad != 0 && lds_atomics_lane_ordered_state() == 1) {
    lds_order_demote();  // the lane-order property did not hold under load: explicit ranking from now on
    return 1;
  }
  GR_REQUIRE(h_bad == 0, "depth sort produced an unsorted order (internal error)");
  return GR_OK;
}

// A plain frame after its first sort_and_count: the redo rules, then the counts -> h_num_rendered.
static int redo_and_report(FramePlan plan, const SceneArgs& a, const Geom& g, int32_t* tot, hipStream_t stream,
                           int64_t* h_num_rendered) {
  const int V = plan.V;
  Counts c = decode_counts(tot, V, plan.short_rows, Transport::Sync, 0);
  int rc;
  if (c.bucket_overflow) {  // a bucket of the bucket depth sort overflowed: three passes, now and for a while
    bucket_sort_overflowed();
    GR_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(g.totals + 2 * V), c.far_depth ? 1 : 0, 1, stream));
    plan = plan.without_buckets();
    rc = sort_and_count(plan, g, a.P, tot, stream, nullptr);
    if (rc != GR_OK) return rc;
    c = decode_counts(tot, V, plan.short_rows, Transport::Sync, 0);
  }
  if (c.far_depth) {  // some depth >= 8192: redo the ordering with full-width keys
    hipLaunchKernelGGL(full_keys_kernel, dim3((unsigned)((a.P * V + 255) / 256)), dim3(256), 0, stream, a.P * V, g.rec, a.radii,
                       g.dfield);
    GR_LAUNCH_CHECK();
    plan = plan.with_full_keys();
    rc = sort_and_count(plan, g, a.P, tot, stream, nullptr);
    if (rc != GR_OK) return rc;
    c = decode_counts(tot, V, plan.short_rows, Transport::Sync, 0);
  }
  rc = check_depth_order(a.P, V, g, stream);
  if (rc == 1) {
    plan = plan.without_buckets();
    rc = sort_and_count(plan, g, a.P, tot, stream, nullptr);
    if (rc != GR_OK) return rc;
    c = decode_counts(tot, V, plan.short_rows, Transport::Sync, 0);
    rc = check_depth_order(a.P, V, g, stream);
    if (rc == 1) rc = GR_OK;
  }
  if (rc != GR_OK) return rc;
  for (int v = 0; v < V; ++v) h_num_rendered[v] = c.totals[v];
  h_num_rendered[V] = c.chunk_max;  // sizes the scatter's LDS staging block in gr_raster_render
  return GR_OK;
}

// defer != nullptr: everything is enqueued, the counts are on their way as defer->plan.transport says instead of behind a
// stream synchronise, and h_num_rendered is NOT filled -- the caller calls preprocess_collect().  bucket_sort: whether that
// frame takes the bucket depth sort (a plain call asks the cooldown itself).
static int preprocess_impl(const SceneArgs& a, const gr_raster_view* h_views, int num_views, void* geom, size_t geom_bytes,
                           int64_t* h_num_rendered, hipStream_t stream, Deferred* defer, bool bucket_sort) {
  int rc = check_views(h_views, num_views);
  if (rc != GR_OK) return rc;
  GR_REQUIRE(h_num_rendered != nullptr, "h_num_rendered is null");
  for (int v = 0; v <= num_views; ++v) h_num_rendered[v] = 0;
  GR_REQUIRE(a.P >= 0 && a.P < (1ll << 31) - 1, "P out of range");
  const int W = h_views[0].image_width, H = h_views[0].image_height;
  if (a.P == 0) {  // nothing to project, but the render call still needs the camera table (background)
    Geom g0 = carve_geom(geom, 0, num_views, tiles_of(W, H));
    if (!geom || geom_bytes < g0.bytes) {
      set_error("raster geometry buffer too small: need %zu bytes, got %zu", g0.bytes, geom_bytes);
      return GR_ERR_WORKSPACE;
    }
    rc = upload_views(h_views, num_views, g0.totals + 2 * num_views, stream);
    if (rc != GR_OK) return rc;
    GR_HIP(hipStreamSynchronize(stream));
    return GR_OK;
  }
  GR_REQUIRE(a.means3D && a.opacities && a.radii, "means3D / opacities / radii must be non-null");
  GR_REQUIRE((a.shs != nullptr) != (a.colors_precomp != nullptr),
             "Please provide excatly one of either SHs or precomputed colors!");
  GR_REQUIRE(((a.scales != nullptr && a.rotations != nullptr) != (a.cov3D_precomp != nullptr)) &&
                 ((a.scales != nullptr) == (a.rotations != nullptr)),
             "Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!");
  const int D = h_views[0].sh_degree;
  if (a.shs) GR_REQUIRE(a.M >= (D + 1) * (D + 1), "shs has %d coefficients, sh_degree %d needs %d", a.M, D, (D + 1) * (D + 1));
  const int gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE;
  GR_REQUIRE(gx <= 255 && gy <= 255, "image too large: at most 255 x 255 tiles of 16 px (got %d x %d)", gx, gy);
  const size_t bin_lds = (size_t)(BIN_T / WAVE) * gx * gy * sizeof(unsigned int);
  GR_REQUIRE(bin_lds <= 156 * 1024, "image too large: the per-wave tile cursors (%zu bytes) do not fit in LDS", bin_lds);
  const Geom g = carve_geom(geom, a.P, num_views, gx * gy);
  if (!geom || geom_bytes < g.bytes) {
    set_error("raster geometry buffer too small: need %zu bytes, got %zu", g.bytes, geom_bytes);
    return GR_ERR_WORKSPACE;
  }
  const bool sh16 = a.shs != nullptr && a.M == 16 && (reinterpret_cast<uintptr_t>(a.shs) % 16 == 0);
  const FramePlan plan = FramePlan::make(
      a.P, num_views, W, H, sh16, defer != nullptr, defer != nullptr && defer->mail != nullptr,
      defer != nullptr ? bucket_sort : bucket_sort_allowed(depth_sort_msd_possible(a.P, num_views, KEY_DEPTH_BITS)));
  DevView cam1;
  memset(&cam1, 0, sizeof(cam1));
  if (plan.preprocess == PreprocessKind::Late) fill_view(cam1, h_views[0]);  // that kernel always reads the camera from its arguments
  int far_seq = 1;
  if (plan.cam_in_args) {
    far_seq = defer->seq;
  } else {
    rc = upload_views(h_views, num_views, g.totals + 2 * num_views, stream);  // cameras + the cleared depth-overflow flag
    if (rc != GR_OK) return rc;
  }
  if (defer != nullptr) {
    defer->far_seq = far_seq;
    defer->plan = plan;
  }
  rc = launch_preprocess(plan, a, D, W, H, g, cam1, far_seq, stream);
  if (rc != GR_OK) return rc;
  int32_t* tot = static_cast<int32_t*>(pinned_scratch(1, sizeof(int32_t) * (2 * num_views + 2)));
  GR_REQUIRE(tot != nullptr, "pinned read-back buffer could not be allocated");
  rc = sort_and_count(plan, g, a.P, tot, stream, defer);
  if (rc != GR_OK || defer != nullptr) return rc;
  return redo_and_report(plan, a, g, tot, stream, h_num_rendered);
}

extern "C" int gr_raster_render(int64_t P, const gr_raster_view* h_views, int num_views,
                                const int64_t* h_num_rendered, const void* geom, size_t geom_bytes,
                                void* bin, size_t bin_bytes, float* out_color, void* stream_) {
  static const int env_flags = (getenv("GR_RASTER_FAST_EXP") && getenv("GR_RASTER_FAST_EXP")[0] == '1') ? GR_RASTER_FAST_EXP : 0;
  return gr_raster_render_ex(P, h_views, num_views, h_num_rendered, geom, geom_bytes, bin, bin_bytes, out_color, env_flags,
                             stream_);
}

extern "C" int gr_raster_preprocess(int64_t P, int M, const float* means3D, const float* shs,
                                    const float* colors_precomp, const float* opacities,
                                    const float* scales, const float* rotations,
                                    const float* cov3D_precomp, const gr_raster_view* h_views,
                                    int num_views, int32_t* radii, void* geom, size_t geom_bytes,
                                    int64_t* h_num_rendered, void* stream_) {
  const SceneArgs a{P, M, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, radii};
  return preprocess_impl(a, h_views, num_views, geom, geom_bytes, h_num_rendered, static_cast<hipStream_t>(stream_), nullptr,
                         false);
}

// has the counting kernel stamped every view's words with this frame's stamp?
static bool mail_stamped(const volatile int32_t* words, int V, int seq) {
  bool ready = true;
  for (int v = 0; v < V; ++v) ready = ready && __atomic_load_n(&words[mail_stamp_word(V, v)], __ATOMIC_ACQUIRE) == seq;
  return ready;
}

// waits for the counts of a deferred preprocess_impl (mailbox stamps or the event) and decodes them
static int preprocess_collect(const Deferred& d, hipStream_t stream, Counts* counts) {
  const int V = d.plan.V;
  const volatile int32_t* words = d.mail;
  if (d.plan.transport == Transport::Mail) {
    // the GPU is still drawing while the host spins here; no time limit of its own (a long or shared device is not an
    // error), but a stream that has drained or failed without the stamps is
    bool ready = false;
    for (unsigned long spin = 1; !ready; ++spin) {
      ready = mail_stamped(words, V, d.seq);
      if (!ready && (spin & 0xffff) == 0 && hipStreamQuery(stream) != hipErrorNotReady) {
        ready = mail_stamped(words, V, d.seq);
        GR_HIP(hipStreamSynchronize(stream));
        GR_REQUIRE(ready, "rasterizer: the counting kernel did not report its totals");
      }
    }
  } else {
    GR_HIP(hipEventSynchronize(d.ev));
    words = static_cast<const int32_t*>(pinned_scratch(1, sizeof(int32_t) * (2 * V + 2)));
    GR_REQUIRE(words != nullptr, "pinned read-back buffer missing");
  }
  *counts = decode_counts(words, V, d.plan.short_rows, d.plan.transport, d.far_seq);
  return GR_OK;
}

using ScatterFn = decltype(&tile_scatter_kernel<true, BIN_T, SEG_READ>);
static ScatterFn scatter_fn(bool lane_ordered, bool wide, int seg_mode) {
  // [lane ordered / ballot ranking][SEG_SELF_RAW, SEG_SELF_SCAN, SEG_READ][WIDE_T, BIN_T threads]
  static const ScatterFn table[2][3][2] = {
      {{tile_scatter_kernel<true, WIDE_T, SEG_SELF_RAW>, tile_scatter_kernel<true, BIN_T, SEG_SELF_RAW>},
       {tile_scatter_kernel<true, WIDE_T, SEG_SELF_SCAN>, tile_scatter_kernel<true, BIN_T, SEG_SELF_SCAN>},
       {tile_scatter_kernel<true, WIDE_T, SEG_READ>, tile_scatter_kernel<true, BIN_T, SEG_READ>}},
      {{tile_scatter_kernel<false, WIDE_T, SEG_SELF_RAW>, tile_scatter_kernel<false, BIN_T, SEG_SELF_RAW>},
       {tile_scatter_kernel<false, WIDE_T, SEG_SELF_SCAN>, tile_scatter_kernel<false, BIN_T, SEG_SELF_SCAN>},
       {tile_scatter_kernel<false, WIDE_T, SEG_READ>, tile_scatter_kernel<false, BIN_T, SEG_READ>}}};
  return table[lane_ordered ? 0 : 1][seg_mode == SEG_SELF_RAW ? 0 : seg_mode == SEG_SELF_SCAN ? 1 : 2][wide ? 0 : 1];
}

// the tile scatter of a frame; timed: as the "raster_bin" share of the frame (the launch after a demotion is not)
static int launch_scatter(bool lane_ordered, bool timed, const FramePlan& plan, const ScatterPlan& sp, const Geom& g, const Bin& b,
                          int64_t P, unsigned int list_cap, const SelfSeg& self, hipStream_t stream) {
  const ScatterFn kern = scatter_fn(lane_ordered, sp.threads == WIDE_T, plan.seg_mode);
  int tile_bits = 0;
  while ((1 << tile_bits) < plan.tiles) ++tile_bits;
  if (sp.lds > 64 * 1024)
    GR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                               160 * 1024 - 512));  // (the SELF variants hold a few static words as well)
  std::optional<KernelTimer> timer;
  if (timed) timer.emplace("raster_bin", stream);
  hipLaunchKernelGGL(kern, dim3((unsigned)bin_grid(plan.V, plan.nchunk)), dim3(sp.threads), (size_t)sp.lds, stream, (int)P, plan.V,
                     plan.gx, plan.gy, plan.nchunk, tile_bits, sp.stage_cap, g.nvis, g.rects, g.order_b, g.rec, g.seg_off,
                     b.point_list, list_cap, sp.elist_cap, self);
  GR_LAUNCH_CHECK();
  return GR_OK;
}

using BlendAuxFn = decltype(&blend_kernel<false, false, true>);
static BlendAuxFn blend_aux_fn(bool fast, bool keep) {
  static const BlendAuxFn table[2][2] = {{blend_kernel<true, true, true>, blend_kernel<false, true, true>},
                                         {blend_kernel<true, false, true>, blend_kernel<false, false, true>}};
  return table[keep ? 0 : 1][fast ? 0 : 1];
}
using BlendFn = decltype(&blend_kernel<false, false>);
static BlendFn blend_fn(bool fast, bool keep) {
  static const BlendFn table[2][2] = {{blend_kernel<true, true>, blend_kernel<false, true>},
                                      {blend_kernel<true, false>, blend_kernel<false, false>}};
  return table[keep ? 0 : 1][fast ? 0 : 1];
}

// spec_entries < 0: the instance counts in h_num_rendered are this call's (the normal render).
// spec_entries >= 0: speculative launch for gr_raster_forward (defer: that frame) -- the counts are not known on the host
// yet; `bin` holds spec_entries list entries, h_num_rendered[num_views] is only a hint for the staging block, and the kernels
// themselves refuse to run past the list (tile_scatter_kernel / blend_kernel list_cap).
static int render_impl(int64_t P, const gr_raster_view* h_views, int num_views, const int64_t* h_num_rendered,
                       const void* geom, size_t geom_bytes, void* bin, size_t bin_bytes, float* out_color, int flags,
                       int64_t spec_entries, hipStream_t stream, const Deferred* defer = nullptr, bool keep = false,
                       float* out_depth = nullptr, float* out_alpha = nullptr, float* aux_state = nullptr) {
  int rc = check_views(h_views, num_views);
  if (rc != GR_OK) return rc;
  GR_REQUIRE(out_color != nullptr && h_num_rendered != nullptr, "null argument");
  const bool spec = spec_entries >= 0;
  const int W = h_views[0].image_width, H = h_views[0].image_height;
  // (a plain render follows a plain preprocess: the plan of that frame, made again from the same sizes)
  const FramePlan plan = spec && defer != nullptr ? defer->plan : FramePlan::make(P, num_views, W, H, false, false, false, false);
  const int gx = plan.gx, gy = plan.gy, tiles = plan.tiles, nchunk = plan.nchunk;
  const int64_t vtiles = (int64_t)gx * gy * num_views;
  GR_REQUIRE(vtiles < (1ll << 31), "too many tiles");
  int64_t R = 0;
  if (spec) R = spec_entries;
  else
    for (int v = 0; v < num_views; ++v) R += h_num_rendered[v];
  GR_REQUIRE(R < (1ll << 31) - 1, "too many rendered instances (%lld)", (long long)R);
  Geom g = carve_geom(const_cast<void*>(geom), P, num_views, tiles);
  GR_REQUIRE(P == 0 || (geom && geom_bytes >= g.bytes), "geometry buffer missing or too small");
  Bin b = carve_bin(bin, R, vtiles);
  if (!bin || bin_bytes < b.bytes) {
    set_error("raster binning buffer too small: need %zu bytes, got %zu", b.bytes, bin_bytes);
    return GR_ERR_WORKSPACE;
  }
  const unsigned int list_cap = spec ? (unsigned int)R : 0xffffffffu;
  if (R > 0 || (spec && P > 0)) {
    const ScatterPlan sp = ScatterPlan::make(tiles, num_views, h_num_rendered[num_views], spec);
    bool ordered = false;
    rc = lds_atomics_lane_ordered(stream, &ordered);
    if (rc != GR_OK) return rc;
    const bool self_raw = plan.seg_mode == SEG_SELF_RAW;
    const SelfSeg self{g.chunk_total, g.totals, self_raw ? const_cast<int32_t*>(defer->mail) : nullptr, self_raw ? defer->seq : 0};
    rc = launch_scatter(ordered, true, plan, sp, g, b, P, list_cap, self, stream);
    if (rc != GR_OK) return rc;
    if (!spec && verify_this_frame()) {  // first frames: every (chunk, tile) segment in depth order?
      int h_bad = 0;
      rc = device_check(stream, [&](int* d_bad) {
        // (the depth check of gr_raster_preprocess left the depth rank of every Gaussian in keys_a)
        hipLaunchKernelGGL(verify_tile_lists_kernel, dim3((unsigned)(num_views * nchunk)), dim3(256), 0, stream, (int)P, num_views,
                           nchunk, tiles, g.seg_off, b.point_list, reinterpret_cast<const int32_t*>(g.keys_a), d_bad);
      }, &h_bad);
      if (rc != GR_OK) return rc;
      if (h_bad != 0 && ordered) {
        lds_order_demote();
        rc = launch_scatter(false, false, plan, sp, g, b, P, list_cap, self, stream);
        if (rc != GR_OK) return rc;
      } else {
        GR_REQUIRE(h_bad == 0, "tile binning produced an unsorted list (internal error)");
      }
    }
  }
  KernelTimer timer("raster_blend", stream);
  const bool fast = (flags & GR_RASTER_FAST_EXP) != 0;
  const int blend_chunks = (R > 0 || (spec && P > 0)) ? nchunk : 0;
  // GR_RASTER_SHARE (a caller that keeps another one-camera frame in flight next to this one): the blend alone fills all 32
  // wave slots of a CU (8 workgroups x 19 KB of LDS), and the next frame's front kernels -- the chain the host waits for --
  // queue behind it.  14 KB of unused dynamic LDS cap it at 4 workgroups per CU: the blend takes longer, out of sight behind
  // the other frame, and the front chain gets its slots (5 290 -> 5 450 views/s).
  const size_t blend_pad = (spec && (flags & GR_RASTER_SHARE)) ? 14000 : 0;
  if (out_depth != nullptr)  // gr_raster_render_aux: depth and alpha beside the colour
    hipLaunchKernelGGL(blend_aux_fn(fast, keep), dim3(gx, gy, num_views), dim3(BLOCK), 0, stream, (int)P, W, H, blend_chunks,
                       g.views, g.seg_off, b.point_list, g.rec, out_color, list_cap, BlendAux<true>{out_depth, out_alpha, aux_state});
  else
    hipLaunchKernelGGL(blend_fn(fast, keep), dim3(gx, gy, num_views), dim3(BLOCK), blend_pad, stream, (int)P, W, H, blend_chunks,
                       g.views, g.seg_off, b.point_list, g.rec, out_color, list_cap, BlendAux<false>{});
  GR_LAUNCH_CHECK();
  frame_done();
  return GR_OK;
}

extern "C" int gr_raster_render_ex(int64_t P, const gr_raster_view* h_views, int num_views,
                                   const int64_t* h_num_rendered, const void* geom, size_t geom_bytes,
                                   void* bin, size_t bin_bytes, float* out_color, int flags, void* stream_) {
  return render_impl(P, h_views, num_views, h_num_rendered, geom, geom_bytes, bin, bin_bytes, out_color, flags, -1,
                     static_cast<hipStream_t>(stream_));
}

extern "C" int gr_raster_render_keep(int64_t P, const gr_raster_view* h_views, int num_views,
                                     const int64_t* h_num_rendered, const void* geom, size_t geom_bytes,
                                     void* bin, size_t bin_bytes, float* out_state, int flags, void* stream_) {
  return render_impl(P, h_views, num_views, h_num_rendered, geom, geom_bytes, bin, bin_bytes, out_state, flags, -1,
                     static_cast<hipStream_t>(stream_), nullptr, true);
}

extern "C" int gr_raster_render_aux(int64_t P, const gr_raster_view* h_views, int num_views,
                                    const int64_t* h_num_rendered, const void* geom, size_t geom_bytes,
                                    void* bin, size_t bin_bytes, float* out_color, float* out_depth, float* out_alpha,
                                    float* out_state, int flags, void* stream_) {
  GR_REQUIRE(out_depth != nullptr && out_alpha != nullptr, "out_depth / out_alpha is null");
  return render_impl(P, h_views, num_views, h_num_rendered, geom, geom_bytes, bin, bin_bytes, out_color, flags, -1,
                     static_cast<hipStream_t>(stream_), nullptr, out_state != nullptr, out_depth, out_alpha, out_state);
}

namespace gr {
namespace {
struct Pending {  // a gr_raster_forward(GR_RASTER_SPLIT) of this thread whose counts have not been collected yet
  bool open;
  int64_t entries;
  Deferred d;
  hipStream_t stream;
};
thread_local Pending g_pending{false, 0, Deferred{}, nullptr};
}  // namespace
}  // namespace gr

extern "C" int gr_raster_debug_bucket_cooldown(int set) {
  const int left = gr::g_bucket_cooldown;
  if (set >= 0) gr::g_bucket_cooldown = set;
  return left;
}

// The second half of a deferred frame: its counts -> h_num_rendered, and what the caller does next.  GR_RETRY_FULL: a depth
// past the compact keys or an overflowed bucket -- the order is not valid, the frame takes the plain path; GR_RETRY_BIN: the
// list of `entries` was too short.
static int collect_deferred(const Deferred& d, int64_t entries, hipStream_t stream, int64_t* h_num_rendered) {
  Counts c;
  int rc = preprocess_collect(d, stream, &c);
  if (rc != GR_OK) return rc;
  if (c.bucket_overflow) bucket_sort_overflowed();
  int64_t R = 0;
  for (int v = 0; v < d.plan.V; ++v) R += h_num_rendered[v] = c.totals[v];
  h_num_rendered[d.plan.V] = c.chunk_max;
  if (c.far_depth) return GR_RETRY_FULL;
  return R <= entries ? GR_OK : GR_RETRY_BIN;
}

extern "C" int gr_raster_forward_finish(int64_t* h_num_rendered) {
  using namespace gr;
  GR_REQUIRE(g_pending.open, "gr_raster_forward_finish: no split gr_raster_forward is open on this thread");
  GR_REQUIRE(h_num_rendered != nullptr, "h_num_rendered is null");
  const Pending p = g_pending;
  g_pending.open = false;
  return collect_deferred(p.d, p.entries, p.stream, h_num_rendered);
}

extern "C" int gr_raster_forward(int64_t P, int M, const float* means3D, const float* shs, const float* colors_precomp,
                                 const float* opacities, const float* scales, const float* rotations,
                                 const float* cov3D_precomp, const gr_raster_view* h_views, int num_views, int32_t* radii,
                                 void* geom, size_t geom_bytes, void* bin, size_t bin_bytes, float* out_color, int flags,
                                 int64_t* h_num_rendered, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  GR_REQUIRE(h_num_rendered != nullptr, "h_num_rendered is null");
  GR_REQUIRE(!g_pending.open, "gr_raster_forward: the previous split call of this thread was not finished");
  const int64_t stage_hint = h_num_rendered[num_views > 0 ? num_views : 0];  // in: last frame's largest chunk (0 = unknown)
  const int64_t entries = bin && bin_bytes > 512 ? (int64_t)((bin_bytes - 512) / sizeof(int32_t)) - 64 : -1;
  // (only for a few views per call: at 32 views the host's share of a 3 ms frame is nothing, and the scatter measured 16 %
  // slower when launched this way -- 0.474 vs 0.405 ms)
  if (P > 0 && num_views <= 4 && entries > 0 && entries < (1ll << 31) - 1 && !verify_this_frame()) {
    // The host is not needed between the two halves of a frame: the counts are read back behind an event while the
    // binning scatter and the blend are launched right behind the counting kernels on a list sized by the caller
    // (last frame's count + 25 %).  The host then waits for the EVENT -- the GPU is still drawing -- and only a frame whose
    // count turns out larger than the list (the kernels refuse to run past it) is rendered again.
    static thread_local hipEvent_t ev = nullptr;
    if (ev == nullptr) GR_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    static thread_local int32_t* mail = nullptr;  // host-mapped, coherent: the counting kernel writes it, the host polls it
    if (mail == nullptr) {
      static const bool no_mail = getenv("GR_NO_MAILBOX") && getenv("GR_NO_MAILBOX")[0] == '1';  // (common.hip: the same switch)
      void* mp = nullptr;
      if (!no_mail && hipHostMalloc(&mp, 4096, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess) {
        memset(mp, 0, 4096);
        mail = static_cast<int32_t*>(mp);
      } else {
        (void)hipGetLastError();
      }
    }
    static std::atomic<int> frame_seq{0};
    int seq = frame_seq.fetch_add(1) + 1;
    if (seq > 0x7ffffff0) {  // (two billion frames: start over; a stale stamp of that age cannot be in flight)
      frame_seq.store(1);
      seq = 1;
    }
    Deferred d{ev, mail, seq, 1, FramePlan{}};
    const SceneArgs a{P, M, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, radii};
    int rc = preprocess_impl(a, h_views, num_views, geom, geom_bytes, h_num_rendered, stream, &d,
                             bucket_sort_allowed(depth_sort_msd_possible(P, num_views, KEY_DEPTH_BITS)));
    if (rc != GR_OK) return rc;
    h_num_rendered[num_views] = stage_hint;
    rc = render_impl(P, h_views, num_views, h_num_rendered, geom, geom_bytes, bin, bin_bytes, out_color, flags, entries, stream,
                     &d);
    if (rc != GR_OK) return rc;
    if (flags & GR_RASTER_SPLIT) {  // the caller comes back with gr_raster_forward_finish (same thread)
      g_pending = Pending{true, entries, d, stream};
      return GR_PENDING;
    }
    rc = collect_deferred(d, entries, stream, h_num_rendered);
    if (rc != GR_RETRY_FULL) return rc;
    // a depth >= 8192: the ordering has to be redone on full-width keys -- take the plain path for this frame
  }
  int rc = gr_raster_preprocess(P, M, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, h_views,
                                num_views, radii, geom, geom_bytes, h_num_rendered, stream);
  if (rc != GR_OK) return rc;
  int64_t R = 0;
  for (int v = 0; v < num_views; ++v) R += h_num_rendered[v];
  if (bin == nullptr || bin_bytes < gr_raster_bin_bytes(R, h_views[0].image_width, h_views[0].image_height, num_views))
    return GR_RETRY_BIN;  // the caller allocates gr_raster_bin_bytes(sum h_num_rendered) and calls gr_raster_render_ex
  return gr_raster_render_ex(P, h_views, num_views, h_num_rendered, geom, geom_bytes, bin, bin_bytes, out_color, flags, stream);
}

extern "C" int gr_raster_mark_visible(int64_t P, const float* means3D, const float* h_viewmatrix,
                                      uint8_t* present, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  GR_REQUIRE(P >= 0 && h_viewmatrix != nullptr, "bad argument");
  if (P == 0) return GR_OK;
  GR_REQUIRE(means3D && present, "null argument");
  hipLaunchKernelGGL(mark_visible_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, stream, (int)P, means3D,
                     h_viewmatrix[2], h_viewmatrix[6], h_viewmatrix[10], h_viewmatrix[14], present);
  GR_LAUNCH_CHECK();
  return GR_OK;
}
