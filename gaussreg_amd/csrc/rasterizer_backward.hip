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
//   camera         (gr_raster_backward_cam) a preprocess bwd kernel of its own that also sums, per view, the 27 non-zero
//                  entries of dL/d(viewmatrix, projmatrix, campos) over the workgroup (DPP inside the wave, the four waves in
//                  order through LDS) into per-(view, workgroup) partials; a second kernel adds the partials of a view in a
//                  fixed order.  No float atomics here either.
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

// Camera gradients.  With p_3 = 1, per (view, Gaussian):
//   ph[c] = sum_j proj[j * 4 + c] p_j (c = 0, 1, 3; column 2 is never read)  ->  dproj[j * 4 + c] = p_j dph[c]
//   t[c]  = sum_j view[j * 4 + c] p_j (c = 0 .. 2; column 3 is never read)   ->  dview[j * 4 + c] = p_j dt[c], to dt[2] the
//           depth map adds gs[9] (AUX)
//   A0[j] = J00 view[j * 4] + J02 view[j * 4 + 2], A1[j] = J11 view[j * 4 + 1] + J12 view[j * 4 + 2], j = 0 .. 2
//                                          ->  dview[j * 4 + (0, 1, 2)] += (gA0_j J00, gA1_j J11, gA0_j J02 + gA1_j J12)
//   SH direction = (p - campos) / |.|      ->  dcampos = -(the direction's share of dmean)
// NCAM = 27 sums per view, in the order of the partials: view (j, c) at 3 j + c, proj (j, c in {0, 1, 3}) at 12 + 3 j + k,
// campos at 24 + k.  A thread keeps the 18 factors (NCAMF) of a view until the end of that view's iteration, where all 64
// lanes of the wave are back together (the DPP sums need the whole wave), forms the products there and sums them; a wave
// in which no lane has a rectangle for the view writes zeros instead.  Per (view, wave) sums wait in LDS (432 bytes per
// view, dynamic) for the end of the kernel: no barrier inside the view loop.
constexpr int NCAM = 27;
constexpr int NCAMF = 18;  // dph0, dph1, dph3; dt[0 .. 2]; the covariance path's 3 x 3; dcampos[0 .. 2]

struct PreBwdCam {
  float* partial;  // [V][gridDim.x][NCAM]
};

// AUX: the slots hold NF_AUX floats; the tenth, dL/dz, reaches the mean through the third row of the view matrix
// (z = view[2] p0 + view[6] p1 + view[10] p2 + view[14]).
// CAM: threads past P stay (as lanes that have no rectangle in any view) until the sums are done.
// The body (preprocess_backward_body.hpp) is included in preprocess_backward_kernel (CAM = false: the kernel as it was)
// and in preprocess_backward_cam_kernel (CAM = true), a kernel of its own.
template <bool HAS_SH, bool HAS_COV, bool AUX = false>
__global__ __launch_bounds__(256) void preprocess_backward_kernel(
    int P, int D, int M, int V, int W, int H, const DevView* __restrict__ views, const float* __restrict__ means3D,
    const float* __restrict__ shs, const float* __restrict__ scales, const float* __restrict__ rotations,
    const float* __restrict__ cov3D_precomp, const uint32_t* __restrict__ rect_raw, const float4* __restrict__ rec,
    const int32_t* __restrict__ slot_local, const int32_t* __restrict__ block_pre, int64_t slot_cap,
    const float* __restrict__ slots, BwdOut out) {
  constexpr bool CAM = false;
  const PreBwdCam cam_out{nullptr};  // (never read)
#define GR_PREPROCESS_BACKWARD_BODY_OK
#include "preprocess_backward_body.hpp"
#undef GR_PREPROCESS_BACKWARD_BODY_OK
}

// + the camera sums; dynamic LDS: 4 * NCAM floats per view
template <bool HAS_SH, bool HAS_COV, bool AUX>
__global__ __launch_bounds__(256) void preprocess_backward_cam_kernel(
    int P, int D, int M, int V, int W, int H, const DevView* __restrict__ views, const float* __restrict__ means3D,
    const float* __restrict__ shs, const float* __restrict__ scales, const float* __restrict__ rotations,
    const float* __restrict__ cov3D_precomp, const uint32_t* __restrict__ rect_raw, const float4* __restrict__ rec,
    const int32_t* __restrict__ slot_local, const int32_t* __restrict__ block_pre, int64_t slot_cap,
    const float* __restrict__ slots, BwdOut out, PreBwdCam cam_out) {
  constexpr bool CAM = true;
#define GR_PREPROCESS_BACKWARD_BODY_OK
#include "preprocess_backward_body.hpp"
#undef GR_PREPROCESS_BACKWARD_BODY_OK
}

// one workgroup per view: the partials of the view's nb workgroups, summed in a fixed order (row r of 32 takes workgroups
// r, r + 32, ... in order; then the 32 rows in order).  Columns the forward never reads (3 of viewmatrix, 2 of
// projmatrix) get zeros.  Null outputs are not written.
__global__ __launch_bounds__(1024) void camera_sum_kernel(int nb, const float* __restrict__ partial, float* __restrict__ dview,
                                                          float* __restrict__ dproj, float* __restrict__ dcampos) {
  __shared__ float s_row[32][32];
  __shared__ float s_tot[NCAM];
  const int v = blockIdx.x, f = threadIdx.x & 31, r = threadIdx.x >> 5;
  float acc = 0.0f;
  if (f < NCAM) {
    const float* src = partial + (int64_t)v * nb * NCAM + f;
    for (int b = r; b < nb; b += 32) acc += src[(int64_t)b * NCAM];
  }
  s_row[r][f] = acc;
  __syncthreads();
  if (threadIdx.x < NCAM) {
    float t = 0.0f;
    for (int k = 0; k < 32; ++k) t += s_row[k][threadIdx.x];
    s_tot[threadIdx.x] = t;
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < 16) {
    const int j = t >> 2, c = t & 3;
    if (dview) dview[v * 16 + t] = c < 3 ? s_tot[3 * j + c] : 0.0f;
    if (dproj) dproj[v * 16 + t] = c == 2 ? 0.0f : s_tot[12 + 3 * j + (c == 3 ? 2 : c)];
  } else if (t < 19 && dcampos) {
    dcampos[v * 3 + (t - 16)] = s_tot[24 + (t - 16)];
  }
}

struct BwdScratch {
  int32_t* slot_local;  // [V * P]
  int32_t* block_pre;   // [ceil(V * P / 256)]
  float* slots;         // [R][NF] (NF_AUX for gr_raster_backward_aux)
  float* cam_partial;   // [V][ceil(P / 256)][NCAM] (gr_raster_backward_cam only)
  size_t bytes;
};

BwdScratch carve_bwd(void* p, int64_t P, int V, int64_t R, int nf = NF, bool cam = false) {
  BwdScratch s;
  Carver c(p);
  s.slot_local = c.take<int32_t>(P * V);
  s.block_pre = c.take<int32_t>((P * V + 255) / 256 + 1);  // + the grand total
  s.slots = c.take<float>(R * nf);
  s.cam_partial = cam ? c.take<float>((P + 255) / 256 * V * NCAM) : nullptr;
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

extern "C" size_t gr_raster_backward_cam_bytes(int64_t P, int num_views, int width, int height,
                                               const int64_t* h_num_rendered, int flags) {
  if (P < 0 || num_views < 1 || width <= 0 || height <= 0 || h_num_rendered == nullptr) return 0;
  const int nf = (flags & GR_RASTER_BWD_COLOR_ONLY) ? NF : NF_AUX;
  return carve_bwd(nullptr, P, num_views, total_rendered(h_num_rendered, num_views), nf, true).bytes;
}

// the three camera outputs of gr_raster_backward_cam, each nullable; all null: the instances without camera sums run
struct CamGrads {
  float* view = nullptr;    // (V, 16)
  float* proj = nullptr;    // (V, 16)
  float* campos = nullptr;  // (V, 3)
  bool any() const { return view != nullptr || proj != nullptr || campos != nullptr; }
};

// aux: gr_raster_backward_aux -- ten floats per slot, gradients of the depth and alpha maps; any map gradient may be null
static int backward_impl(bool aux, const CamGrads& cam, const float* dL_ddepth, const float* dL_dalpha, int64_t P, int M,
                         const float* means3D,
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
  if (P == 0) {
    if (cam.view) GR_HIP(hipMemsetAsync(cam.view, 0, sizeof(float) * 16 * num_views, stream));
    if (cam.proj) GR_HIP(hipMemsetAsync(cam.proj, 0, sizeof(float) * 16 * num_views, stream));
    if (cam.campos) GR_HIP(hipMemsetAsync(cam.campos, 0, sizeof(float) * 3 * num_views, stream));
    return GR_OK;
  }
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
  const BwdScratch s = carve_bwd(scratch, P, num_views, R, nf, cam.any());
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
    const size_t cam_lds = sizeof(float) * NCAM * 4 * num_views;  // (at most 27 648 bytes: num_views <= MAX_VIEWS)
#define GR_PBWD_(SH, COV, AUX)                                                                                            \
  do {                                                                                                                    \
    if (cam.any())                                                                                                        \
      hipLaunchKernelGGL((preprocess_backward_cam_kernel<SH, COV, AUX>), grd, blk, cam_lds, stream, (int)P, D, M,         \
                         num_views, W, H, g.views, means3D, shs, scales, rotations, cov3D_precomp, g.rect_raw, g.rec,     \
                         s.slot_local, s.block_pre, R, s.slots, out, PreBwdCam{s.cam_partial});                     \
    else                                                                                                                  \
      hipLaunchKernelGGL((preprocess_backward_kernel<SH, COV, AUX>), grd, blk, 0, stream, (int)P, D, M, num_views, W, H,  \
                         g.views, means3D, shs, scales, rotations, cov3D_precomp, g.rect_raw, g.rec, s.slot_local,        \
                         s.block_pre, R, s.slots, out);                                                                   \
  } while (0)
#define GR_PBWD(SH, COV) do { if (aux) GR_PBWD_(SH, COV, true); else GR_PBWD_(SH, COV, false); } while (0)
    if (shs && cov3D_precomp) GR_PBWD(true, true);
    else if (shs) GR_PBWD(true, false);
    else if (cov3D_precomp) GR_PBWD(false, true);
    else GR_PBWD(false, false);
#undef GR_PBWD
#undef GR_PBWD_
    GR_LAUNCH_CHECK();
    if (cam.any()) {
      hipLaunchKernelGGL(camera_sum_kernel, dim3((unsigned)num_views), dim3(1024), 0, stream, (int)grd.x, s.cam_partial,
                         cam.view, cam.proj, cam.campos);
      GR_LAUNCH_CHECK();
    }
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
  return backward_impl(false, CamGrads{}, nullptr, nullptr, P, M, means3D, shs, colors_precomp, opacities, scales, rotations,
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
  return backward_impl(true, CamGrads{}, dL_ddepth, dL_dalpha, P, M, means3D, shs, colors_precomp, opacities, scales, rotations,
                       cov3D_precomp, h_views, num_views, geom, geom_bytes, bin, bin_bytes, h_num_rendered, final_T, n_contrib,
                       dL_dcolor, flags, dL_dmeans3D, dL_dmeans2D, dL_dshs, dL_dcolors, dL_dopacity, dL_dscales,
                       dL_drotations, dL_dcov3D, scratch, scratch_bytes, stream_);
}

extern "C" int gr_raster_backward_cam(int64_t P, int M, const float* means3D, const float* shs, const float* colors_precomp,
                                      const float* opacities, const float* scales, const float* rotations,
                                      const float* cov3D_precomp, const gr_raster_view* h_views, int num_views,
                                      const void* geom, size_t geom_bytes, const void* bin, size_t bin_bytes,
                                      const int64_t* h_num_rendered, const float* final_T, const int32_t* n_contrib,
                                      const float* dL_dcolor, const float* dL_ddepth, const float* dL_dalpha, int flags,
                                      float* dL_dmeans3D, float* dL_dmeans2D, float* dL_dshs, float* dL_dcolors,
                                      float* dL_dopacity, float* dL_dscales, float* dL_drotations, float* dL_dcov3D,
                                      float* dL_dviewmatrix, float* dL_dprojmatrix, float* dL_dcampos, void* scratch,
                                      size_t scratch_bytes, void* stream_) {
  const bool colour_only = (flags & GR_RASTER_BWD_COLOR_ONLY) != 0;
  if (colour_only && (dL_ddepth != nullptr || dL_dalpha != nullptr)) {
    set_error("gr_raster_backward_cam: GR_RASTER_BWD_COLOR_ONLY takes no dL_ddepth / dL_dalpha");
    return GR_ERR_INVALID;
  }
  CamGrads cam;
  cam.view = dL_dviewmatrix, cam.proj = dL_dprojmatrix, cam.campos = dL_dcampos;
  return backward_impl(!colour_only, cam, dL_ddepth, dL_dalpha, P, M, means3D, shs, colors_precomp, opacities, scales,
                       rotations, cov3D_precomp, h_views, num_views, geom, geom_bytes, bin, bin_bytes, h_num_rendered,
                       final_T, n_contrib, dL_dcolor, flags, dL_dmeans3D, dL_dmeans2D, dL_dshs, dL_dcolors, dL_dopacity,
                       dL_dscales, dL_drotations, dL_dcov3D, scratch, scratch_bytes, stream_);
}
