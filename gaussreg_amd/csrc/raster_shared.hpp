// Device helpers and buffer layouts shared by the rasterizer forward (rasterizer.hip) and backward
// (rasterizer_backward.hip).  Numerics contract: oracle/rasterizer_oracle.c (see rasterizer.hip).
#pragma once

#include "common.hpp"
#include "raster_plan.hpp"  // BIN_T, BIN_CHUNK and the other constants the frame plan needs

namespace gr {
namespace {

constexpr int TILE = 16;
constexpr int BLOCK = TILE * TILE;
constexpr int MAX_VIEWS = 64;  // cameras per preprocess launch (constant-memory table)

struct DevView {
  float view[16];
  float proj[16];
  float campos[3];
  float tanx, tany;
  float fx, fy;
  float scale_mod;
  float bg[3];
};

__device__ __constant__ float SH_C0 = 0.28209479177387814f;
__device__ __constant__ float SH_C1 = 0.4886025119029199f;
__device__ __constant__ float SH_C2[5] = {1.0925484305920792f, -1.0925484305920792f,
                                          0.31539156525252005f, -1.0925484305920792f,
                                          0.5462742152960396f};
__device__ __constant__ float SH_C3[7] = {-0.5900435899266435f, 2.890611442640554f,
                                          -0.4570457994644658f, 0.3731763325901154f,
                                          -0.4570457994644658f, 1.445305721320277f,
                                          -0.5900435899266435f};

// Deterministic expf (x <= 0): identical operation sequence to oracle_exp_det().
__device__ __forceinline__ float exp_det(float x) {
  x = fmaxf(x, -86.0f);
  const float L2E = 1.44269504088896341f, MAGIC = 12582912.0f;
  const float t = x * L2E;
  const float tm = t + MAGIC;
  const float nf = tm - MAGIC;
  const float f = fmaf(x, L2E, -nf);
  float p = 1.3264815788716078e-3f;
  p = fmaf(p, f, 9.671512059867382e-3f);
  p = fmaf(p, f, 5.550733581185341e-2f);
  p = fmaf(p, f, 2.4022242426872253e-1f);
  p = fmaf(p, f, 6.931470036506653e-1f);
  p = fmaf(p, f, 1.0f);
  return __uint_as_float(__float_as_uint(p) + (__float_as_uint(tm) << 23));
}

__device__ __forceinline__ void xform4x3(const float* M, const float* p, float* o) {
  o[0] = fmaf(M[0], p[0], fmaf(M[4], p[1], fmaf(M[8], p[2], M[12])));
  o[1] = fmaf(M[1], p[0], fmaf(M[5], p[1], fmaf(M[9], p[2], M[13])));
  o[2] = fmaf(M[2], p[0], fmaf(M[6], p[1], fmaf(M[10], p[2], M[14])));
}
__device__ __forceinline__ void xform4x4(const float* M, const float* p, float* o) {
  o[0] = fmaf(M[0], p[0], fmaf(M[4], p[1], fmaf(M[8], p[2], M[12])));
  o[1] = fmaf(M[1], p[0], fmaf(M[5], p[1], fmaf(M[9], p[2], M[13])));
  o[2] = fmaf(M[2], p[0], fmaf(M[6], p[1], fmaf(M[10], p[2], M[14])));
  o[3] = fmaf(M[3], p[0], fmaf(M[7], p[1], fmaf(M[11], p[2], M[15])));
}

__device__ __forceinline__ void cov3d_from_scale_rot(const float* sc, float mod, const float* q,
                                                     float* c6) {
  const float s0 = mod * sc[0], s1 = mod * sc[1], s2 = mod * sc[2];
  const float r = q[0], x = q[1], y = q[2], z = q[3];
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
  float M[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    M[0][i] = s0 * R[i][0];
    M[1][i] = s1 * R[i][1];
    M[2][i] = s2 * R[i][2];
  }
#define GR_SIG(i, j) fmaf(M[0][i], M[0][j], fmaf(M[1][i], M[1][j], M[2][i] * M[2][j]))
  c6[0] = GR_SIG(0, 0);
  c6[1] = GR_SIG(0, 1);
  c6[2] = GR_SIG(0, 2);
  c6[3] = GR_SIG(1, 1);
  c6[4] = GR_SIG(1, 2);
  c6[5] = GR_SIG(2, 2);
#undef GR_SIG
}

__device__ __forceinline__ void cov2d(const float* t_in, float fx, float fy, float tanx, float tany,
                                      const float* c6, const float* V, float* out3) {
  float t[3] = {t_in[0], t_in[1], t_in[2]};
  const float limx = 1.3f * tanx, limy = 1.3f * tany;
  const float txtz = t[0] / t[2], tytz = t[1] / t[2];
  t[0] = fminf(limx, fmaxf(-limx, txtz)) * t[2];
  t[1] = fminf(limy, fmaxf(-limy, tytz)) * t[2];
  const float J00 = fx / t[2];
  const float J02 = -(fx * t[0]) / (t[2] * t[2]);
  const float J11 = fy / t[2];
  const float J12 = -(fy * t[1]) / (t[2] * t[2]);
  float A0[3], A1[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    A0[j] = fmaf(J00, V[j * 4 + 0], J02 * V[j * 4 + 2]);
    A1[j] = fmaf(J11, V[j * 4 + 1], J12 * V[j * 4 + 2]);
  }
  const float S[3][3] = {{c6[0], c6[1], c6[2]}, {c6[1], c6[3], c6[4]}, {c6[2], c6[4], c6[5]}};
  float B0[3], B1[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    B0[k] = fmaf(S[k][0], A0[0], fmaf(S[k][1], A0[1], S[k][2] * A0[2]));
    B1[k] = fmaf(S[k][0], A1[0], fmaf(S[k][1], A1[1], S[k][2] * A1[2]));
  }
  out3[0] = fmaf(A0[0], B0[0], fmaf(A0[1], B0[1], A0[2] * B0[2])) + 0.3f;
  out3[1] = fmaf(A1[0], B0[0], fmaf(A1[1], B0[1], A1[2] * B0[2]));
  out3[2] = fmaf(A1[0], B1[0], fmaf(A1[1], B1[1], A1[2] * B1[2])) + 0.3f;
}

// sh: this Gaussian's coefficients, (M,3) row-major, already in registers/local memory
template <typename ShLoad>
__device__ __forceinline__ void sh_to_rgb(int deg, const float* pos, const float* campos,
                                          ShLoad S, float* rgb) {
  const float dx = pos[0] - campos[0], dy = pos[1] - campos[1], dz = pos[2] - campos[2];
  const float len = sqrtf(dx * dx + dy * dy + dz * dz);
  const float x = dx / len, y = dy / len, z = dz / len;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float res = SH_C0 * S(0, c);
    if (deg > 0) {
      res = res - SH_C1 * y * S(1, c) + SH_C1 * z * S(2, c) - SH_C1 * x * S(3, c);
      if (deg > 1) {
        const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
        res = res + SH_C2[0] * xy * S(4, c) + SH_C2[1] * yz * S(5, c) +
              SH_C2[2] * (2.0f * zz - xx - yy) * S(6, c) + SH_C2[3] * xz * S(7, c) +
              SH_C2[4] * (xx - yy) * S(8, c);
        if (deg > 2) {
          res = res + SH_C3[0] * y * (3.0f * xx - yy) * S(9, c) + SH_C3[1] * xy * z * S(10, c) +
                SH_C3[2] * y * (4.0f * zz - xx - yy) * S(11, c) +
                SH_C3[3] * z * (2.0f * zz - 3.0f * xx - 3.0f * yy) * S(12, c) +
                SH_C3[4] * x * (4.0f * zz - xx - yy) * S(13, c) +
                SH_C3[5] * z * (xx - yy) * S(14, c) + SH_C3[6] * x * (xx - 3.0f * yy) * S(15, c);
        }
      }
    }
    res += 0.5f;
    rgb[c] = fmaxf(res, 0.0f);
  }
}

// geometry state: one 64-byte record per (view, Gaussian) so that the blend's per-instance gather
// (ids arrive in depth order, i.e. random in memory) touches ONE 64-B sector instead of three lines:
//   rec[0] = {px, py, sxx, syy (axis cull factors)}   rec[1] = {conic.x, conic.y, conic.z, opacity}
//   rec[2] = {r, g, b, kc (cull factor)}              rec[3] = {radius (int bits), view-space depth z, 0, 0}
// rec[3].y is what the depth map blends and what its backward differentiates (gr_raster_render_aux / _backward_aux).
struct Geom {
  float4* rec;           // [V][P][4]
  uint32_t* dfield;      // [V*P] depth-sort field: rebased depth bits (see KEY_DEPTH_BITS), 0 = culled
  uint32_t* rect_raw;    // [V*P] packed tile rectangle of every (view, Gaussian), Gaussian order
  uint64_t* keys_a;      // [V*P] x 2: (field << 32 | id) ping-pong buffers of the depth sort
  uint64_t* keys_b;
  int32_t* order_a;      // (unused: the sort generates ids on the fly); order_b = per-view front-to-back order
  int32_t* order_b;
  uint32_t* rects;       // [V*P] depth-ordered tile rectangles (26-bit packing of the key's high bits)
  uint16_t* chunk_cnt;   // [V][nchunk][tiles] instances per (chunk of BIN_CHUNK depth-ordered Gaussians, tile)
  uint32_t* seg_off;     // [V][nchunk][tiles + 1] position of segment (chunk, tile) in the point list (+ end sentinel)
  int32_t* chunk_total;  // [V][nchunk] instances per chunk, then [V][nchunk] exclusive prefix inside the view
  int32_t* chunk_max;    // [1] largest chunk total
  void* ds_table;        // depth-sort histograms / offsets
  size_t ds_table_bytes;
  int2* key_mm;          // [V][ceil(P / 256)] smallest / largest depth field of a preprocess block (up to four views per call),
                         // [V][4 ceil(P / 256)] of a preprocess wave (more views)
  int32_t* nvis;         // [V] visible (depth-ordered) Gaussians per view
  int32_t* totals;       // [V] instances per view, [V] largest chunk total of every view, [1] depth-overflow flag, [3] pad --
  DevView* views;        // -- immediately followed by the [MAX_VIEWS] camera table: ONE upload clears the flag and sets the cameras
  int32_t* scan_ws;
  size_t bytes;
};

Geom carve_geom(void* p, int64_t P, int V, int64_t tiles) {
  Geom g;
  Carver c(p);
  const int64_t nchunk = (P + BIN_CHUNK - 1) / BIN_CHUNK;
  g.rec = c.take<float4>(P * V * 4);
  g.dfield = c.take<uint32_t>(P * V);
  g.rect_raw = c.take<uint32_t>(P * V);
  g.keys_a = c.take<uint64_t>(P * V);
  g.keys_b = c.take<uint64_t>(P * V);
  g.order_a = nullptr;
  g.order_b = c.take<int32_t>(P * V);
  g.rects = c.take<uint32_t>(P * V);
  g.chunk_cnt = c.take<uint16_t>(V * nchunk * tiles);
  g.seg_off = c.take<uint32_t>(V * nchunk * (tiles + 1));
  g.chunk_total = c.take<int32_t>(2 * V * nchunk);
  g.chunk_max = c.take<int32_t>(1);
  g.ds_table_bytes = depth_sort_table_bytes(P, V);
  g.ds_table = c.take<char>(g.ds_table_bytes);
  // (depth_sort_msd_possible; more than four views: a pair per wave of the preprocess, not per block)
  g.key_mm = c.take<int2>(V <= 4 ? V * ((P + 255) / 256) : P <= (1ll << 20) ? V * ((P + 255) / 256) * (256 / WAVE) : 0);
  g.nvis = c.take<int32_t>(V);
  g.totals = c.take<int32_t>(2 * V + 4 + MAX_VIEWS * (sizeof(DevView) / sizeof(int32_t)));
  g.views = reinterpret_cast<DevView*>(g.totals ? g.totals + 2 * V + 4 : nullptr);
  static_assert(sizeof(DevView) % sizeof(int32_t) == 0, "camera table follows an int array");
  g.scan_ws = c.take<int32_t>(V * scan_ws_ints(nchunk));
  g.bytes = c.used();
  return g;
}

struct Bin {
  int32_t* point_list;  // [R] Gaussian ids: chunk-major, tile-sorted inside a chunk, depth order inside a segment
  size_t bytes;
};

Bin carve_bin(void* p, int64_t R, int64_t vtiles) {
  Bin b;
  Carver c(p);
  (void)vtiles;
  b.point_list = c.take<int32_t>(R + 64);
  b.bytes = c.used();
  return b;
}

}  // namespace
}  // namespace gr
