// 3D-Gaussian-splatting rasterizer backward for MI355X (gfx950): the derivative of the forward in rasterizer.hip, with
// upstream's conventions (graphdeco-inria/diff-gaussian-rasterization backward.cu; contract in include/gaussreg_hip.h).
//
// Starts from what an autograd forward (gr_raster_render_keep) left behind: the geometry buffer (records, rectangles,
// camera table), the binning buffer (per-tile lists), and per pixel the final transmittance and n_contrib.
//   slot count     1 thread / (view, Gaussian): area of the tile rectangle the binning emitted -> block-local exclusive
//                  scan; a one-block pass scans the block totals.  Slot base(v, g) = local + block prefix.
//   render bwd     1 workgroup / (tile, view), 1 thread / pixel: walks the tile's list back to front from the tile's largest
//                  n_contrib, batches of 256 records staged in LDS, upstream's recurrences per (pixel, entry); the 9 floats
//                  of an entry are summed over the tile on chip in a fixed order (DPP inside the wave, then the four waves in
//                  order) and stored with plain stores into slot base(v, g) + (ty - y0) w + (tx - x0).  No float atomics:
//                  bitwise reproducible.  Slots of tiles the walk never reaches stay zero (memset).
//   preprocess bwd 1 thread / Gaussian: per view in order, sums its slots in rectangle order and applies the chain rule in
//                  fp32 (conic -> cov2D -> cov3D -> scale / quaternion, NDC mean -> mean, SH -> colour), accumulated over
//                  the views in registers; every output is written once.
#include <algorithm>
#include <type_traits>

#include "raster_shared.hpp"

namespace gr {
namespace {

constexpr int NF = 9;  // per (tile, entry): dL/d(px, py) (pixels), dL/dconic (a, b, c), dL/dopacity, dL/d(r, g, b)
constexpr int NF_AUX = 10;  // gr_raster_backward_aux: + dL/dz (view-space depth), the "colour" of the depth map
constexpr int NWAVE = BLOCK / WAVE;

// wave-wide fp32 sum on the DPP shift network, fixed order (the inclusive-scan pattern; lane 63 holds the total)
__device__ __forceinline__ float wave_sum_f32_dpp(float x) {
#define GR_F32_STEP(CTRL, ROWMASK) x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, ROWMASK, 0xf, false));
  GR_F32_STEP(0x111, 0xf) GR_F32_STEP(0x112, 0xf) GR_F32_STEP(0x114, 0xf) GR_F32_STEP(0x118, 0xf)
  GR_F32_STEP(0x142, 0xa) GR_F32_STEP(0x143, 0xc)
#undef GR_F32_STEP
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 63));
}

// ------------------------------------------------------------------------------------ slot bases
__global__ __launch_bounds__(256) void slot_count_kernel(int64_t n, int P, int gx, int gy, const uint32_t* __restrict__ rect_raw,
                                                         const float4* __restrict__ rec, int32_t* __restrict__ slot_local,
                                                         int32_t* __restrict__ block_sum) {
  __shared__ int s_w[256 / WAVE];
  const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int area = 0;
  if (o < n) {
    const uint32_t r = rect_raw[o];
    int x0, y0, w, h;
    const int64_t vbase = o / P * P;
    if (r != 0u && rect_decode(r, (int)(o - vbase), vbase, rec, gx, gy, x0, y0, w, h)) area = w * h;
  }
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
  const int incl = wave_incl_scan_add_dpp(area);
  if (lane == WAVE - 1) s_w[wv] = incl;
  __syncthreads();
  int before = 0;
  for (int w = 0; w < wv; ++w) before += s_w[w];
  if (o < n) slot_local[o] = before + incl - area;
  if (threadIdx.x == 0) block_sum[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// one workgroup: exclusive scan of the block totals, in place; block_pre[nb] = the grand total (checked against the
// instance count on the host before any slot is written)
__global__ __launch_bounds__(1024) void slot_block_scan_kernel(int nb, int32_t* __restrict__ block_pre) {
  __shared__ int s_w[1024 / WAVE];
  __shared__ int s_carry;
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
  if (threadIdx.x == 0) s_carry = 0;
  __syncthreads();
  for (int b0 = 0; b0 < nb; b0 += 1024) {
    const int b = b0 + threadIdx.x;
    const int x = b < nb ? block_pre[b] : 0;
    const int incl = wave_incl_scan_add_dpp(x);
    if (lane == WAVE - 1) s_w[wv] = incl;
    __syncthreads();
    int base = s_carry;
    for (int w = 0; w < wv; ++w) base += s_w[w];
    if (b < nb) block_pre[b] = base + incl - x;
    __syncthreads();
    if (threadIdx.x == 1023) s_carry = base + incl;
    __syncthreads();
  }
  if (threadIdx.x == 0) block_pre[nb] = s_carry;
}

// ------------------------------------------------------------------------------------ render backward
// AUX (gr_raster_backward_aux): the depth map is a fourth colour channel whose per-entry colour is z (rec[3].y) and whose
// background is 0, with its own accum / last recurrence; the alpha map adds +T_final / (1 - alpha) dL_dalpha_map to
// dL_dalpha (the background term with -dL_dalpha_map for bg_dot).  Ten floats per slot, z as an eleventh s_e plane.
// LDS: s_part and s_e grow by 5 120 bytes.  The slot index stays in a register (the thread that loads entry tid is the one
// that stores its sums) and the strip mask is a byte: 53 008 bytes.  Three workgroups per CU, as without AUX (50 704, whose
// layout is unchanged), need a margin below 160 KiB / 3: with 54 032 bytes (3 x = 162 096 < 163 840) only two were resident on
// the device, measured as 1.53 x the kernel time.  (Presumably the LDS is allocated in blocks; their size was not measured.)
// RenderBwdAux<false> is an empty struct: the instances without AUX keep their instruction stream; their kernel-argument
// segment grows by four bytes (an empty C++ object still has a size) that no instruction reads.
// Any of dL_dpix / aux.dL_ddepth / aux.dL_dalpha may be null with AUX (= zeros).
template <bool AUX>
struct RenderBwdAux {};
template <>
struct RenderBwdAux<true> {
  const float* dL_ddepth;  // [V][H][W] or null
  const float* dL_dalpha;  // [V][H][W] or null
};

template <bool FAST_EXP, bool AUX = false>
__global__ __launch_bounds__(BLOCK) void render_backward_kernel(
    int P, int W, int H, int nchunk, const DevView* __restrict__ views, const uint32_t* __restrict__ seg_off,
    const int32_t* __restrict__ point_list, const float4* __restrict__ rec, const uint32_t* __restrict__ rect_raw,
    const int32_t* __restrict__ slot_local, const int32_t* __restrict__ block_pre, int64_t slot_cap,
    const float* __restrict__ final_T, const int32_t* __restrict__ n_contrib, const float* __restrict__ dL_dpix,
    float* __restrict__ slots, RenderBwdAux<AUX> aux) {
  constexpr int NF = AUX ? NF_AUX : gr::NF;
  using mask_t = typename std::conditional<AUX, unsigned char, unsigned int>::type;
  __shared__ float s_e[AUX ? 11 : 10][BLOCK];  // px, py, pc, conic a, b, c, opacity, r, g, b (, z)
  __shared__ int64_t s_slot[AUX ? 1 : BLOCK];  // AUX: my_slot instead; the one-element array is never touched and takes no LDS
  int64_t my_slot = -1;
  __shared__ mask_t s_wmask[BLOCK];  // bit w: the entry can reach the pixel strip of wave w
  __shared__ float s_part[NWAVE][BLOCK][NF];
  __shared__ int s_wpre[WAVE];
  __shared__ unsigned int s_woff[WAVE];
  __shared__ int s_max[NWAVE];
  const int gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE;
  const int v = blockIdx.z;
  const int tile = blockIdx.y * gx + blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1), lw = tid / WAVE;
  // pixel of this thread: the forward's layout (16 lanes = one 4 x 4 cell, a wave = a 16 x 4 strip)
  constexpr int CELL = 4;
  const int cell = tid / (CELL * CELL), pin = tid % (CELL * CELL);
  const int lx = (cell % (TILE / CELL)) * CELL + pin % CELL;
  const int ly = (cell / (TILE / CELL)) * CELL + pin / CELL;
  const int pxi = blockIdx.x * TILE + lx, pyi = blockIdx.y * TILE + ly;
  const bool inside = pxi < W && pyi < H;
  const float pfx = (float)pxi, pfy = (float)pyi;
  const float tx0 = (float)(blockIdx.x * TILE), ty0 = (float)(blockIdx.y * TILE);
  const int tiles = gx * gy;
  const int64_t vbase = (int64_t)v * P;
  const int64_t q = ((int64_t)v * H + (inside ? pyi : 0)) * W + (inside ? pxi : 0);
  const int64_t hw = (int64_t)H * W;
  const float T_final = inside ? final_T[q] : 0.0f;
  const int last = inside ? n_contrib[q] : 0;
  float g[3] = {0.f, 0.f, 0.f};
  if (inside && (!AUX || dL_dpix != nullptr)) {
    const float* gp = dL_dpix + (int64_t)v * 3 * hw + (int64_t)pyi * W + pxi;
    g[0] = gp[0];
    g[1] = gp[hw];
    g[2] = gp[2 * hw];
  }
  float g_d = 0.f, g_a = 0.f, accum_d = 0.f, last_z = 0.f;  // AUX: dL/ddepth, dL/dalpha of the pixel; depth's recurrence
  if constexpr (AUX) {
    if (inside && aux.dL_ddepth != nullptr) g_d = aux.dL_ddepth[q];
    if (inside && aux.dL_dalpha != nullptr) g_a = aux.dL_dalpha[q];
  }
  const DevView& cam = views[v];
  const float bg_dot = cam.bg[0] * g[0] + cam.bg[1] * g[1] + cam.bg[2] * g[2];
  float T = T_final, accum[3] = {0.f, 0.f, 0.f}, last_col[3] = {0.f, 0.f, 0.f}, last_alpha = 0.f;
  // the tile's largest n_contrib: the walk starts there
  const int wmax = wave_max_i32_dpp(last);
  if (lane == 0) s_max[lw] = wmax;
  __syncthreads();
  const int max_n = max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
  if (max_n == 0 || nchunk == 0) return;  // block-uniform
  const uint32_t* seg_col = seg_off + (int64_t)v * nchunk * (tiles + 1) + tile;
  // window of 64 chunks starting at chunk c0: s_woff = segment starts, s_wpre = inclusive prefix of the segment lengths
  auto load_window = [&](int c0) -> int {
    if (tid < WAVE) {
      const int c = c0 + tid;
      unsigned int a = 0u, b = 0u;
      if (c < nchunk) {
        a = seg_col[(int64_t)c * (tiles + 1)];
        b = seg_col[(int64_t)c * (tiles + 1) + 1];
      }
      s_woff[tid] = a;
      s_wpre[tid] = wave_incl_scan_add_dpp((int)(b - a));
    }
    __syncthreads();
    return s_wpre[WAVE - 1];
  };
  // forward over the windows to the one holding entry max_n - 1 (base = its first entry's index in the tile's list)
  int c0 = 0, base = 0, w_total = 0;
  while (true) {
    w_total = load_window(c0);
    __syncthreads();
    if (base + w_total >= max_n || c0 + WAVE >= nchunk) break;
    base += w_total;
    c0 += WAVE;
  }
  int hi = min(max_n - base, w_total);
  while (true) {
    // (s_wpre / s_woff hold window c0 here)
    while (hi > 0) {
      const int lo = max(0, hi - BLOCK), n = hi - lo;
      // ---- load: entry lo + tid of the window
      if (tid < n) {
        const int e = lo + tid;
        int l = 0;
#pragma unroll
        for (int st = WAVE / 2; st > 0; st >>= 1)
          if (s_wpre[l + st - 1] <= e) l += st;
        const int before = l ? s_wpre[l - 1] : 0;
        const int id = point_list[s_woff[l] + (unsigned int)(e - before)];
        const float4* r = rec + 4 * (vbase + id);
        const float4 r0 = r[0], co = r[1], col = r[2];
        const float pc = -__logf(255.0f * co.w) - 1.0e-3f;
        const float rc2 = -pc * col.w;
        const float cpr = -pc + 1.0e-3f + 2.0e-6f * rc2;
        const float hx2 = cpr * r0.z, hy2 = cpr * r0.w;
        s_e[0][tid] = r0.x;
        s_e[1][tid] = r0.y;
        s_e[2][tid] = pc;
        s_e[3][tid] = co.x;
        s_e[4][tid] = co.y;
        s_e[5][tid] = co.z;
        s_e[6][tid] = co.w;
        s_e[7][tid] = col.x;
        s_e[8][tid] = col.y;
        s_e[9][tid] = col.z;
        if constexpr (AUX) s_e[10][tid] = r[3].y;
        // which wave strips (16 x 4 px) the entry can reach: the forward's cell test on the strip's box (a superset of
        // its four cells, so nothing the forward blended is skipped)
        const float ex = fmaxf(fmaxf(tx0 - r0.x, r0.x - (tx0 + (float)(TILE - 1))), 0.0f);
        unsigned int m = 0u;
#pragma unroll
        for (int s = 0; s < NWAVE; ++s) {
          const float ylo = ty0 + (float)(s * CELL);
          const float ey = fmaxf(fmaxf(ylo - r0.y, r0.y - (ylo + (float)(CELL - 1))), 0.0f);
          if (!(ex * ex + ey * ey > rc2) && !(ex * ex > hx2) && !(ey * ey > hy2)) m |= 1u << s;
        }
        s_wmask[tid] = (mask_t)m;
        int x0, y0, w, h;
        int64_t slot = -1;
        if (rect_decode(rect_raw[vbase + id], id, vbase, rec, gx, gy, x0, y0, w, h)) {
          const int64_t o = vbase + id;
          slot = (int64_t)slot_local[o] + block_pre[o >> 8] + (int64_t)((int)blockIdx.y - y0) * w + ((int)blockIdx.x - x0);
        }
        if (AUX) my_slot = slot; else s_slot[tid] = slot;
      }
      __syncthreads();
      // ---- back to front over the batch
      for (int j = n - 1; j >= 0; --j) {
        float* part = s_part[lw][j];
        if (!((s_wmask[j] >> lw) & 1u)) {  // wave-uniform
          if (lane < NF) part[lane] = 0.0f;
          continue;
        }
        const int gidx = base + lo + j;
        const float dx = s_e[0][j] - pfx, dy = s_e[1][j] - pfy;
        const float cx = s_e[3][j], cy = s_e[4][j], cz = s_e[5][j], op = s_e[6][j];
        // alpha exactly as the forward evaluates it
        const float qf = fmaf(cx * dx, dx, (cz * dy) * dy);
        const float power = fmaf(-0.5f, qf, -((cy * dx) * dy));
        const float G = FAST_EXP ? __builtin_amdgcn_exp2f(power * 1.44269504088896341f) : exp_det(power);
        const float alpha = fminf(op * G, 0.99f);
        const bool hit = inside && gidx < last && !(power > 0.0f) && !(power < s_e[2][j]) && !(alpha < 1.0f / 255.0f);
        float val[NF];
#pragma unroll
        for (int f = 0; f < NF; ++f) val[f] = 0.0f;
        if (hit) {
          T = T / (1.0f - alpha);
          const float dchannel_dcolor = alpha * T;
          float dL_dalpha = 0.0f;
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) {
            const float c = s_e[7 + ch][j];
            accum[ch] = last_alpha * last_col[ch] + (1.0f - last_alpha) * accum[ch];
            last_col[ch] = c;
            dL_dalpha += (c - accum[ch]) * g[ch];
            val[6 + ch] = dchannel_dcolor * g[ch];
          }
          if constexpr (AUX) {
            const float z = s_e[10][j];
            accum_d = last_alpha * last_z + (1.0f - last_alpha) * accum_d;
            last_z = z;
            dL_dalpha += (z - accum_d) * g_d;
            val[9] = dchannel_dcolor * g_d;
          }
          dL_dalpha *= T;
          last_alpha = alpha;
          dL_dalpha += (-T_final / (1.0f - alpha)) * bg_dot;
          if constexpr (AUX) dL_dalpha += (T_final / (1.0f - alpha)) * g_a;
          const float dL_dG = op * dL_dalpha;  // straight-through 0.99 clamp
          const float gdx = G * dx, gdy = G * dy;
          val[0] = dL_dG * (-gdx * cx - gdy * cy);
          val[1] = dL_dG * (-gdy * cz - gdx * cy);
          val[2] = -0.5f * gdx * dx * dL_dG;
          val[3] = -gdx * dy * dL_dG;
          val[4] = -0.5f * gdy * dy * dL_dG;
          val[5] = G * dL_dalpha;
        }
        if (__ballot(hit) == 0ull) {
          if (lane < NF) part[lane] = 0.0f;
          continue;
        }
#pragma unroll
        for (int f = 0; f < NF; ++f) {
          const float s = wave_sum_f32_dpp(val[f]);
          if (lane == 0) part[f] = s;
        }
      }
      __syncthreads();
      // ---- the four waves' partial sums, in wave order -> the entry's slot
      if (tid < n) {
        const int64_t slot = AUX ? my_slot : s_slot[tid];
        if (slot >= 0 && slot < slot_cap) {  // (always: the host checked the slot layout against the instance count)
          float* dst = slots + NF * slot;
#pragma unroll
          for (int f = 0; f < NF; ++f)
            dst[f] = ((s_part[0][tid][f] + s_part[1][tid][f]) + s_part[2][tid][f]) + s_part[3][tid][f];
        }
      }
      __syncthreads();
      hi = lo;
    }
    if (c0 == 0) break;
    c0 -= WAVE;
    w_total = load_window(c0);
    base -= w_total;
    hi = w_total;
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------ preprocess backward
// SH basis and its derivatives along the normalised view direction (x, y, z)
__device__ __forceinline__ void sh_basis_grad(int deg, float x, float y, float z, float* B, float* Bx, float* By, float* Bz) {
#pragma unroll
  for (int k = 0; k < 16; ++k) B[k] = Bx[k] = By[k] = Bz[k] = 0.0f;
  B[0] = SH_C0;
  if (deg > 0) {
    B[1] = -SH_C1 * y; By[1] = -SH_C1;
    B[2] = SH_C1 * z;  Bz[2] = SH_C1;
    B[3] = -SH_C1 * x; Bx[3] = -SH_C1;
    if (deg > 1) {
      const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
      B[4] = SH_C2[0] * xy;                 Bx[4] = SH_C2[0] * y;          By[4] = SH_C2[0] * x;
      B[5] = SH_C2[1] * yz;                 By[5] = SH_C2[1] * z;          Bz[5] = SH_C2[1] * y;
      B[6] = SH_C2[2] * (2.f * zz - xx - yy); Bx[6] = -2.f * SH_C2[2] * x; By[6] = -2.f * SH_C2[2] * y; Bz[6] = 4.f * SH_C2[2] * z;
      B[7] = SH_C2[3] * xz;                 Bx[7] = SH_C2[3] * z;          Bz[7] = SH_C2[3] * x;
      B[8] = SH_C2[4] * (xx - yy);          Bx[8] = 2.f * SH_C2[4] * x;    By[8] = -2.f * SH_C2[4] * y;
      if (deg > 2) {
        B[9] = SH_C3[0] * y * (3.f * xx - yy);
        Bx[9] = SH_C3[0] * 6.f * xy;            By[9] = SH_C3[0] * 3.f * (xx - yy);
        B[10] = SH_C3[1] * xy * z;
        Bx[10] = SH_C3[1] * yz;                 By[10] = SH_C3[1] * xz;            Bz[10] = SH_C3[1] * xy;
        B[11] = SH_C3[2] * y * (4.f * zz - xx - yy);
        Bx[11] = SH_C3[2] * -2.f * xy;          By[11] = SH_C3[2] * (4.f * zz - xx - 3.f * yy); Bz[11] = SH_C3[2] * 8.f * yz;
        B[12] = SH_C3[3] * z * (2.f * zz - 3.f * xx - 3.f * yy);
        Bx[12] = SH_C3[3] * -6.f * xz;          By[12] = SH_C3[3] * -6.f * yz;     Bz[12] = SH_C3[3] * (6.f * zz - 3.f * xx - 3.f * yy);
        B[13] = SH_C3[4] * x * (4.f * zz - xx - yy);
        Bx[13] = SH_C3[4] * (4.f * zz - 3.f * xx - yy); By[13] = SH_C3[4] * -2.f * xy; Bz[13] = SH_C3[4] * 8.f * xz;
        B[14] = SH_C3[5] * z * (xx - yy);
        Bx[14] = SH_C3[5] * 2.f * xz;           By[14] = SH_C3[5] * -2.f * yz;     Bz[14] = SH_C3[5] * (xx - yy);
        B[15] = SH_C3[6] * x * (xx - 3.f * yy);
        Bx[15] = SH_C3[6] * 3.f * (xx - yy);    By[15] = SH_C3[6] * -6.f * xy;
      }
    }
  }
}

struct BwdOut {
  float* means3D;   // (P, 3)
  float* means2D;   // (V, P, 3) or null
  float* shs;       // (P, M, 3)
  float* colors;    // (P, 3)
  float* opacity;   // (P)
  float* scales;    // (P, 3)
  float* rotations; // (P, 4)
  float* cov3D;     // (P, 6)
};

// AUX: the slots hold NF_AUX floats; the tenth, dL/dz, reaches the mean through the third row of the view matrix
// (z = view[2] p0 + view[6] p1 + view[10] p2 + view[14]).
template <bool HAS_SH, bool HAS_COV, bool AUX = false>
__global__ __launch_bounds__(256) void preprocess_backward_kernel(
    int P, int D, int M, int V, int W, int H, const DevView* __restrict__ views, const float* __restrict__ means3D,
    const float* __restrict__ shs, const float* __restrict__ scales, const float* __restrict__ rotations,
    const float* __restrict__ cov3D_precomp, const uint32_t* __restrict__ rect_raw, const float4* __restrict__ rec,
    const int32_t* __restrict__ slot_local, const int32_t* __restrict__ block_pre, int64_t slot_cap,
    const float* __restrict__ slots, BwdOut out) {
  constexpr int NF = AUX ? NF_AUX : gr::NF;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P) return;
  const int gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE;
  const int K = (D + 1) * (D + 1);
  const float p[3] = {means3D[3 * (int64_t)i], means3D[3 * (int64_t)i + 1], means3D[3 * (int64_t)i + 2]};
  float sc[3] = {0.f, 0.f, 0.f}, rot[4] = {0.f, 0.f, 0.f, 0.f}, c6[6];
  if (HAS_COV) {
#pragma unroll
    for (int k = 0; k < 6; ++k) c6[k] = cov3D_precomp[6 * (int64_t)i + k];
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) sc[k] = scales[3 * (int64_t)i + k];
#pragma unroll
    for (int k = 0; k < 4; ++k) rot[k] = rotations[4 * (int64_t)i + k];
  }
  float shr[HAS_SH ? 48 : 1], dsh[HAS_SH ? 48 : 1];
  if (HAS_SH) {
#pragma unroll
    for (int k = 0; k < 48; ++k) {
      shr[k] = k < 3 * K ? shs[(int64_t)i * M * 3 + k] : 0.0f;
      dsh[k] = 0.0f;
    }
  }
  float dmean[3] = {0.f, 0.f, 0.f}, dcol[3] = {0.f, 0.f, 0.f}, dop = 0.f, dscale[3] = {0.f, 0.f, 0.f};
  float drot[4] = {0.f, 0.f, 0.f, 0.f}, dcov[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int v = 0; v < V; ++v) {
    const int64_t o = (int64_t)v * P + i;
    const int64_t vbase = (int64_t)v * P;
    float* m2 = out.means2D != nullptr ? out.means2D + 3 * o : nullptr;
    int x0, y0, w, h;
    const uint32_t rr = rect_raw[o];
    if (rr == 0u || !rect_decode(rr, i, vbase, rec, gx, gy, x0, y0, w, h)) {
      if (m2) m2[0] = m2[1] = m2[2] = 0.0f;
      continue;
    }
    // this (view, Gaussian)'s slots, in rectangle order
    const int64_t s0 = (int64_t)slot_local[o] + block_pre[o >> 8];
    const int n = w * h;
    float gs[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) gs[f] = 0.0f;
    for (int k = 0; k < n; ++k) {
      if (s0 + k >= slot_cap) break;  // (never: see render_backward_kernel)
      const float* s = slots + NF * (s0 + k);
#pragma unroll
      for (int f = 0; f < NF; ++f) gs[f] += s[f];
    }
    const DevView& cam = views[v];
    // ---- forward quantities (same fp32 operations as preprocess_kernel)
    float pv[3], ph[4];
    xform4x3(cam.view, p, pv);
    xform4x4(cam.proj, p, ph);
    const float pw = 1.0f / (ph[3] + 0.0000001f);
    if (!HAS_COV) cov3d_from_scale_rot(sc, cam.scale_mod, rot, c6);
    const float tz = pv[2];
    const float limx = 1.3f * cam.tanx, limy = 1.3f * cam.tany;
    const float ux = pv[0] / tz, uy = pv[1] / tz;
    const float cux = fminf(limx, fmaxf(-limx, ux)), cuy = fminf(limy, fmaxf(-limy, uy));
    const float txp = cux * tz, typ = cuy * tz;
    const float J00 = cam.fx / tz, J02 = -(cam.fx * txp) / (tz * tz);
    const float J11 = cam.fy / tz, J12 = -(cam.fy * typ) / (tz * tz);
    const float* Vm = cam.view;
    float A0[3], A1[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      A0[j] = fmaf(J00, Vm[j * 4 + 0], J02 * Vm[j * 4 + 2]);
      A1[j] = fmaf(J11, Vm[j * 4 + 1], J12 * Vm[j * 4 + 2]);
    }
    const float S[3][3] = {{c6[0], c6[1], c6[2]}, {c6[1], c6[3], c6[4]}, {c6[2], c6[4], c6[5]}};
    float SA0[3], SA1[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      SA0[k] = fmaf(S[k][0], A0[0], fmaf(S[k][1], A0[1], S[k][2] * A0[2]));
      SA1[k] = fmaf(S[k][0], A1[0], fmaf(S[k][1], A1[1], S[k][2] * A1[2]));
    }
    const float a = fmaf(A0[0], SA0[0], fmaf(A0[1], SA0[1], A0[2] * SA0[2])) + 0.3f;
    const float b = fmaf(A1[0], SA0[0], fmaf(A1[1], SA0[1], A1[2] * SA0[2]));
    const float c = fmaf(A1[0], SA1[0], fmaf(A1[1], SA1[1], A1[2] * SA1[2])) + 0.3f;
    // ---- conic (c, -b, a) / det -> 2-D covariance
    const float det = a * c - b * b;
    const float inv2 = 1.0f / (det * det);
    const float gA = gs[2], gB = gs[3], gC = gs[4];
    const float ga = (-c * c * gA + b * c * gB - b * b * gC) * inv2;
    const float gb = (2.f * b * c * gA - (a * c + b * b) * gB + 2.f * a * b * gC) * inv2;
    const float gc = (-b * b * gA + a * b * gB - a * a * gC) * inv2;
    // ---- 2-D covariance = A S A^T -> 3-D covariance and A = J W
    float dc6[6];
    dc6[0] = A0[0] * A0[0] * ga + A1[0] * A0[0] * gb + A1[0] * A1[0] * gc;
    dc6[3] = A0[1] * A0[1] * ga + A1[1] * A0[1] * gb + A1[1] * A1[1] * gc;
    dc6[5] = A0[2] * A0[2] * ga + A1[2] * A0[2] * gb + A1[2] * A1[2] * gc;
    dc6[1] = 2.f * A0[0] * A0[1] * ga + (A1[0] * A0[1] + A1[1] * A0[0]) * gb + 2.f * A1[0] * A1[1] * gc;
    dc6[2] = 2.f * A0[0] * A0[2] * ga + (A1[0] * A0[2] + A1[2] * A0[0]) * gb + 2.f * A1[0] * A1[2] * gc;
    dc6[4] = 2.f * A0[1] * A0[2] * ga + (A1[1] * A0[2] + A1[2] * A0[1]) * gb + 2.f * A1[1] * A1[2] * gc;
    float dJ00 = 0.f, dJ02 = 0.f, dJ11 = 0.f, dJ12 = 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float gA0 = 2.f * ga * SA0[j] + gb * SA1[j];
      const float gA1 = gb * SA0[j] + 2.f * gc * SA1[j];
      dJ00 += gA0 * Vm[j * 4 + 0];
      dJ02 += gA0 * Vm[j * 4 + 2];
      dJ11 += gA1 * Vm[j * 4 + 1];
      dJ12 += gA1 * Vm[j * 4 + 2];
    }
    // J -> view-space mean t (the 1.3 tan(fov) clamp of x/z, y/z masks d/dt_x, d/dt_y where active)
    const float tz2 = tz * tz, tz3 = tz2 * tz;
    const float dtxp = -cam.fx / tz2 * dJ02, dtyp = -cam.fy / tz2 * dJ12;
    float dt[3];
    dt[2] = -cam.fx / tz2 * dJ00 - cam.fy / tz2 * dJ11 + 2.f * cam.fx * txp / tz3 * dJ02 + 2.f * cam.fy * typ / tz3 * dJ12;
    const bool inx = ux >= -limx && ux <= limx, iny = uy >= -limy && uy <= limy;
    dt[0] = inx ? dtxp : 0.0f;
    dt[1] = iny ? dtyp : 0.0f;
    if (!inx) dt[2] += dtxp * cux;
    if (!iny) dt[2] += dtyp * cuy;
    // ---- NDC mean (means2D.grad: dL/dNDC, upstream's 0.5 W / 0.5 H factors) -> homogeneous projection
    const float dnx = gs[0] * (0.5f * (float)W), dny = gs[1] * (0.5f * (float)H);
    if (m2) m2[0] = dnx, m2[1] = dny, m2[2] = 0.0f;
    const float dph0 = dnx * pw, dph1 = dny * pw;
    const float dph3 = -(dnx * ph[0] + dny * ph[1]) * pw * pw;
    const float* Pm = cam.proj;
#pragma unroll
    for (int j = 0; j < 3; ++j)
      dmean[j] += Pm[j * 4 + 0] * dph0 + Pm[j * 4 + 1] * dph1 + Pm[j * 4 + 3] * dph3 +
                  Vm[j * 4 + 0] * dt[0] + Vm[j * 4 + 1] * dt[1] + Vm[j * 4 + 2] * dt[2];
    if constexpr (AUX) {
#pragma unroll
      for (int j = 0; j < 3; ++j) dmean[j] += gs[9] * Vm[j * 4 + 2];
    }
    dop += gs[5];
    // ---- colour
    if (HAS_SH) {
      float rgb[3];
      sh_to_rgb(D, p, cam.campos, [&](int k, int ch) { return shr[k * 3 + ch]; }, rgb);  // the forward's clamp decision
      const float d0 = p[0] - cam.campos[0], d1 = p[1] - cam.campos[1], d2 = p[2] - cam.campos[2];
      const float len = sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
      const float x = d0 / len, y = d1 / len, z = d2 / len;
      float B[16], Bx[16], By[16], Bz[16];
      sh_basis_grad(D, x, y, z, B, Bx, By, Bz);
      float ddx = 0.f, ddy = 0.f, ddz = 0.f;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const float gcol = rgb[ch] > 0.0f ? gs[6 + ch] : 0.0f;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          dsh[k * 3 + ch] += B[k] * gcol;
          ddx += Bx[k] * shr[k * 3 + ch] * gcol;
          ddy += By[k] * shr[k * 3 + ch] * gcol;
          ddz += Bz[k] * shr[k * 3 + ch] * gcol;
        }
      }
      const float dot = x * ddx + y * ddy + z * ddz;
      dmean[0] += (ddx - x * dot) / len;
      dmean[1] += (ddy - y * dot) / len;
      dmean[2] += (ddz - z * dot) / len;
    } else {
      dcol[0] += gs[6];
      dcol[1] += gs[7];
      dcol[2] += gs[8];
    }
    // ---- 3-D covariance
    if (HAS_COV) {
#pragma unroll
      for (int k = 0; k < 6; ++k) dcov[k] += dc6[k];
    } else {
      const float mod = cam.scale_mod;
      const float s[3] = {mod * sc[0], mod * sc[1], mod * sc[2]};
      const float r = rot[0], x = rot[1], y = rot[2], z = rot[3];
      float R[3][3];
      R[0][0] = 1.f - 2.f * (y * y + z * z);
      R[0][1] = 2.f * (x * y - r * z);
      R[0][2] = 2.f * (x * z + r * y);
      R[1][0] = 2.f * (x * y + r * z);
      R[1][1] = 1.f - 2.f * (x * x + z * z);
      R[1][2] = 2.f * (y * z - r * x);
      R[2][0] = 2.f * (x * z - r * y);
      R[2][1] = 2.f * (y * z + r * x);
      R[2][2] = 1.f - 2.f * (x * x + y * y);
      // Sigma = Mt^T Mt with Mt[k][i] = s_k R[i][k]; symmetric upstream gradient Gs (off-diagonals carry half of dc6)
      const float Gs[3][3] = {{dc6[0], 0.5f * dc6[1], 0.5f * dc6[2]},
                              {0.5f * dc6[1], dc6[3], 0.5f * dc6[4]},
                              {0.5f * dc6[2], 0.5f * dc6[4], dc6[5]}};
      float dR[3][3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        float ds = 0.f;
#pragma unroll
        for (int ii = 0; ii < 3; ++ii) {
          float dM = 0.f;  // dL/dMt[k][ii] = 2 sum_j Mt[k][j] Gs[j][ii]
#pragma unroll
          for (int j = 0; j < 3; ++j) dM += s[k] * R[j][k] * Gs[j][ii];
          dM *= 2.f;
          ds += dM * R[ii][k];
          dR[ii][k] = s[k] * dM;
        }
        dscale[k] += mod * ds;
      }
      drot[0] += 2.f * (-z * dR[0][1] + y * dR[0][2] + z * dR[1][0] - x * dR[1][2] - y * dR[2][0] + x * dR[2][1]);
      drot[1] += 2.f * (y * dR[0][1] + z * dR[0][2] + y * dR[1][0] - 2.f * x * dR[1][1] - r * dR[1][2] + z * dR[2][0] +
                        r * dR[2][1] - 2.f * x * dR[2][2]);
      drot[2] += 2.f * (-2.f * y * dR[0][0] + x * dR[0][1] + r * dR[0][2] + x * dR[1][0] + z * dR[1][2] - r * dR[2][0] +
                        z * dR[2][1] - 2.f * y * dR[2][2]);
      drot[3] += 2.f * (-2.f * z * dR[0][0] - r * dR[0][1] + x * dR[0][2] + r * dR[1][0] - 2.f * z * dR[1][1] + y * dR[1][2] +
                        x * dR[2][0] + y * dR[2][1]);
    }
  }
  if (out.means3D)
    for (int k = 0; k < 3; ++k) out.means3D[3 * (int64_t)i + k] = dmean[k];
  if (out.opacity) out.opacity[i] = dop;
  if (HAS_SH && out.shs) {
    float* dst = out.shs + (int64_t)i * M * 3;
#pragma unroll
    for (int k = 0; k < 48; ++k)
      if (k < 3 * M) dst[k] = dsh[k];
    for (int k = 48; k < 3 * M; ++k) dst[k] = 0.0f;  // coefficients past degree 3
  }
  if (!HAS_SH && out.colors)
    for (int k = 0; k < 3; ++k) out.colors[3 * (int64_t)i + k] = dcol[k];
  if (HAS_COV && out.cov3D)
    for (int k = 0; k < 6; ++k) out.cov3D[6 * (int64_t)i + k] = dcov[k];
  if (!HAS_COV) {
    if (out.scales)
      for (int k = 0; k < 3; ++k) out.scales[3 * (int64_t)i + k] = dscale[k];
    if (out.rotations)
      for (int k = 0; k < 4; ++k) out.rotations[4 * (int64_t)i + k] = drot[k];
  }
}

struct BwdScratch {
  int32_t* slot_local;  // [V * P]
  int32_t* block_pre;   // [ceil(V * P / 256)]
  float* slots;         // [R][NF] (NF_AUX for gr_raster_backward_aux)
  size_t bytes;
};

BwdScratch carve_bwd(void* p, int64_t P, int V, int64_t R, int nf = NF) {
  BwdScratch s;
  Carver c(p);
  s.slot_local = c.take<int32_t>(P * V);
  s.block_pre = c.take<int32_t>((P * V + 255) / 256 + 1);  // + the grand total
  s.slots = c.take<float>(R * nf);
  s.bytes = c.used();
  return s;
}

int64_t total_rendered(const int64_t* h_num_rendered, int V) {
  int64_t R = 0;
  for (int v = 0; v < V; ++v) R += std::max<int64_t>(h_num_rendered[v], 0);
  return R;
}

}  // namespace
}  // namespace gr

using namespace gr;

extern "C" size_t gr_raster_backward_bytes(int64_t P, int num_views, int width, int height, const int64_t* h_num_rendered) {
  if (P < 0 || num_views < 1 || width <= 0 || height <= 0 || h_num_rendered == nullptr) return 0;
  return carve_bwd(nullptr, P, num_views, total_rendered(h_num_rendered, num_views)).bytes;
}

extern "C" size_t gr_raster_backward_aux_bytes(int64_t P, int num_views, int width, int height,
                                               const int64_t* h_num_rendered) {
  if (P < 0 || num_views < 1 || width <= 0 || height <= 0 || h_num_rendered == nullptr) return 0;
  return carve_bwd(nullptr, P, num_views, total_rendered(h_num_rendered, num_views), NF_AUX).bytes;
}

// aux: gr_raster_backward_aux -- ten floats per slot, gradients of the depth and alpha maps; any map gradient may be null
static int backward_impl(bool aux, const float* dL_ddepth, const float* dL_dalpha, int64_t P, int M, const float* means3D,
                         const float* shs, const float* colors_precomp, const float* opacities, const float* scales,
                         const float* rotations, const float* cov3D_precomp, const gr_raster_view* h_views, int num_views,
                         const void* geom, size_t geom_bytes, const void* bin, size_t bin_bytes,
                         const int64_t* h_num_rendered, const float* final_T, const int32_t* n_contrib,
                         const float* dL_dcolor, int flags, float* dL_dmeans3D, float* dL_dmeans2D, float* dL_dshs,
                         float* dL_dcolors, float* dL_dopacity, float* dL_dscales, float* dL_drotations, float* dL_dcov3D,
                         void* scratch, size_t scratch_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  GR_REQUIRE(h_views != nullptr && num_views >= 1 && num_views <= MAX_VIEWS, "need 1 .. %d views", MAX_VIEWS);
  GR_REQUIRE(h_num_rendered != nullptr, "h_num_rendered is null");
  GR_REQUIRE(P >= 0 && P < (1ll << 31) - 1, "P out of range");
  const int W = h_views[0].image_width, H = h_views[0].image_height, D = h_views[0].sh_degree;
  for (int v = 0; v < num_views; ++v)
    GR_REQUIRE(h_views[v].image_width == W && h_views[v].image_height == H && h_views[v].sh_degree == D,
               "all views of one call must share image size and sh_degree");
  GR_REQUIRE(W > 0 && H > 0 && D >= 0 && D <= 3, "bad image size or sh_degree");
  if (P == 0) return GR_OK;
  GR_REQUIRE(means3D != nullptr, "means3D is null");
  GR_REQUIRE((shs != nullptr) != (colors_precomp != nullptr), "exactly one of shs / colors_precomp");
  GR_REQUIRE((scales != nullptr && rotations != nullptr) != (cov3D_precomp != nullptr),
             "exactly one of (scales, rotations) / cov3D_precomp");
  if (shs) GR_REQUIRE(M >= (D + 1) * (D + 1), "shs has %d coefficients, sh_degree %d needs %d", M, D, (D + 1) * (D + 1));
  const int gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE;
  const int tiles = gx * gy;
  const int64_t R = total_rendered(h_num_rendered, num_views);
  GR_REQUIRE(R < (1ll << 31) - 1, "too many rendered instances");
  const Geom g = carve_geom(const_cast<void*>(geom), P, num_views, tiles);
  GR_REQUIRE(geom != nullptr && geom_bytes >= g.bytes, "geometry buffer missing or too small");
  const Bin bn = carve_bin(const_cast<void*>(bin), R, (int64_t)tiles * num_views);
  GR_REQUIRE(R == 0 || (bin != nullptr && bin_bytes >= bn.bytes), "binning buffer missing or too small");
  GR_REQUIRE(R == 0 || (final_T != nullptr && n_contrib != nullptr && (aux || dL_dcolor != nullptr)), "null per-pixel state");
  const int nf = aux ? NF_AUX : NF;
  const BwdScratch s = carve_bwd(scratch, P, num_views, R, nf);
  if (!scratch || scratch_bytes < s.bytes) {
    set_error("raster backward scratch too small: need %zu bytes, got %zu", s.bytes, scratch_bytes);
    return GR_ERR_WORKSPACE;
  }
  const int64_t n = P * num_views;
  const int nb = (int)((n + 255) / 256);
  {
    KernelTimer timer("raster_bwd_slots", stream);
    hipLaunchKernelGGL(slot_count_kernel, dim3((unsigned)nb), dim3(256), 0, stream, n, (int)P, gx, gy, g.rect_raw, g.rec,
                       s.slot_local, s.block_pre);
    GR_LAUNCH_CHECK();
    hipLaunchKernelGGL(slot_block_scan_kernel, dim3(1), dim3(1024), 0, stream, nb, s.block_pre);
    GR_LAUNCH_CHECK();
    // The slot layout (scan of the emitted rectangles) must hold exactly the R instances the binning counted; a mismatch
    // would misplace gradients, so it is an error, not something the kernels' bounds checks quietly absorb.
    int32_t* h_tot = static_cast<int32_t*>(pinned_scratch(9, sizeof(int32_t)));  // (slot 9: this entry point's own)
    GR_REQUIRE(h_tot != nullptr, "pinned read-back buffer could not be allocated");
    *h_tot = -1;
    GR_HIP(hipMemcpyAsync(h_tot, s.block_pre + nb, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    GR_HIP(hipStreamSynchronize(stream));
    const int32_t h_total = *h_tot;
    GR_REQUIRE(h_total == R, "raster backward: the tile rectangles hold %d instances, the forward binned %lld (geom / "
               "h_num_rendered not from the same forward call?)", h_total, (long long)R);
    if (R > 0) GR_HIP(hipMemsetAsync(s.slots, 0, sizeof(float) * nf * R, stream));
  }
  const int nchunk = (int)((P + BIN_CHUNK - 1) / BIN_CHUNK);
  if (R > 0) {
    KernelTimer timer("raster_bwd_render", stream);
#define GR_RBWD(FE, AUX, ...)                                                                                              \
  hipLaunchKernelGGL((render_backward_kernel<FE, AUX>), dim3(gx, gy, num_views), dim3(BLOCK), 0, stream, (int)P, W, H, nchunk, \
                     g.views, g.seg_off, bn.point_list, g.rec, g.rect_raw, s.slot_local, s.block_pre, R, final_T, n_contrib,  \
                     dL_dcolor, s.slots, RenderBwdAux<AUX>{__VA_ARGS__})
    const bool fast = (flags & GR_RASTER_FAST_EXP) != 0;
    if (aux) { if (fast) GR_RBWD(true, true, dL_ddepth, dL_dalpha); else GR_RBWD(false, true, dL_ddepth, dL_dalpha); }
    else if (fast) GR_RBWD(true, false); else GR_RBWD(false, false);
#undef GR_RBWD
    GR_LAUNCH_CHECK();
  }
  const BwdOut out{dL_dmeans3D, dL_dmeans2D, dL_dshs, dL_dcolors, dL_dopacity, dL_dscales, dL_drotations, dL_dcov3D};
  {
    KernelTimer timer("raster_bwd_preprocess", stream);
    const dim3 grd((unsigned)((P + 255) / 256)), blk(256);
#define GR_PBWD_(SH, COV, AUX)                                                                                            \
  hipLaunchKernelGGL((preprocess_backward_kernel<SH, COV, AUX>), grd, blk, 0, stream, (int)P, D, M, num_views, W, H,      \
                     g.views, means3D, shs, scales, rotations, cov3D_precomp, g.rect_raw, g.rec, s.slot_local,            \
                     s.block_pre, R, s.slots, out)
#define GR_PBWD(SH, COV) do { if (aux) GR_PBWD_(SH, COV, true); else GR_PBWD_(SH, COV, false); } while (0)
    if (shs && cov3D_precomp) GR_PBWD(true, true);
    else if (shs) GR_PBWD(true, false);
    else if (cov3D_precomp) GR_PBWD(false, true);
    else GR_PBWD(false, false);
#undef GR_PBWD
#undef GR_PBWD_
    GR_LAUNCH_CHECK();
  }
  (void)opacities;
  return GR_OK;
}

extern "C" int gr_raster_backward(int64_t P, int M, const float* means3D, const float* shs, const float* colors_precomp,
                                  const float* opacities, const float* scales, const float* rotations,
                                  const float* cov3D_precomp, const gr_raster_view* h_views, int num_views, const void* geom,
                                  size_t geom_bytes, const void* bin, size_t bin_bytes, const int64_t* h_num_rendered,
                                  const float* final_T, const int32_t* n_contrib, const float* dL_dcolor, int flags,
                                  float* dL_dmeans3D, float* dL_dmeans2D, float* dL_dshs, float* dL_dcolors,
                                  float* dL_dopacity, float* dL_dscales, float* dL_drotations, float* dL_dcov3D,
                                  void* scratch, size_t scratch_bytes, void* stream_) {
  return backward_impl(false, nullptr, nullptr, P, M, means3D, shs, colors_precomp, opacities, scales, rotations,
                       cov3D_precomp, h_views, num_views, geom, geom_bytes, bin, bin_bytes, h_num_rendered, final_T, n_contrib,
                       dL_dcolor, flags, dL_dmeans3D, dL_dmeans2D, dL_dshs, dL_dcolors, dL_dopacity, dL_dscales,
                       dL_drotations, dL_dcov3D, scratch, scratch_bytes, stream_);
}

extern "C" int gr_raster_backward_aux(int64_t P, int M, const float* means3D, const float* shs, const float* colors_precomp,
                                      const float* opacities, const float* scales, const float* rotations,
                                      const float* cov3D_precomp, const gr_raster_view* h_views, int num_views,
                                      const void* geom, size_t geom_bytes, const void* bin, size_t bin_bytes,
                                      const int64_t* h_num_rendered, const float* final_T, const int32_t* n_contrib,
                                      const float* dL_dcolor, const float* dL_ddepth, const float* dL_dalpha, int flags,
                                      float* dL_dmeans3D, float* dL_dmeans2D, float* dL_dshs, float* dL_dcolors,
                                      float* dL_dopacity, float* dL_dscales, float* dL_drotations, float* dL_dcov3D,
                                      void* scratch, size_t scratch_bytes, void* stream_) {
  return backward_impl(true, dL_ddepth, dL_dalpha, P, M, means3D, shs, colors_precomp, opacities, scales, rotations,
                       cov3D_precomp, h_views, num_views, geom, geom_bytes, bin, bin_bytes, h_num_rendered, final_T, n_contrib,
                       dL_dcolor, flags, dL_dmeans3D, dL_dmeans2D, dL_dshs, dL_dcolors, dL_dopacity, dL_dscales,
                       dL_drotations, dL_dcov3D, scratch, scratch_bytes, stream_);
}
