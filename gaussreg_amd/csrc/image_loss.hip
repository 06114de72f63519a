// Fused photometric loss of Gaussian-splatting training: (1 - lambda) L1 + lambda (1 - SSIM), 11 x 11 Gaussian window
// (sigma 1.5), zero padding, optional per-pixel weight; forward and the gradient to the first image.
//
// Forward, one workgroup per 32 x 16 tile of one (view, channel) plane:
//   1. both images of the tile plus the 5-pixel halo -> LDS (zeros outside the image)
//   2. horizontal 11-tap pass over the 26 staged rows: E[x], E[y], E[xx], E[yy], E[xy] -> LDS
//   3. vertical 11-tap pass (a thread owns two vertically adjacent pixels and reads 12 rows for them), the SSIM value,
//      the three per-pixel derivative maps the backward needs (weight folded in; written only with a keep buffer)
//   4. the tile's sums of w |x - y|, w ssim and w -> one slot per tile; image_loss_reduce_kernel adds a view's slots in
//      a fixed order.  No atomics anywhere: the result does not depend on scheduling or on the other views of the call.
// Backward, same tiling: the same separable window over the three kept maps, then
//   dL/dx = dL/dloss_v / (C S) * ((1 - lambda) w sign(x - y) - lambda (G*dmu + 2 x G*dsx + y G*dsxy)).
//
// LDS reads are conflict-free by construction: in every pass the 32 lanes of a bank group read 32 consecutive floats.
#include "common.hpp"

namespace gr {
namespace {

constexpr int TW = 32, TH = 16;  // output tile
constexpr int RAD = 5, TAPS = 11;
constexpr int SW = TW + 2 * RAD;  // staged width 42
constexpr int SH = TH + 2 * RAD;  // staged height 26
constexpr int THREADS = 256;
constexpr int ROWS_PER_THREAD = TH / (THREADS / TW);  // 2
static_assert(ROWS_PER_THREAD == 2, "the vertical pass is written for two rows per thread");

// g[i] = exp(-(i - 5)^2 / (2 * 1.5^2)), normalised in float64, rounded once to fp32 (tests/image_loss_f64.py window();
// tests/test_image_loss_f64_reference.py compares this table with it)
// IMAGE_LOSS_WINDOW_BEGIN
#define GR_IMAGE_LOSS_WINDOW                                                                                        \
  1.028380124e-03f, 7.598758209e-03f, 3.600077331e-02f, 1.093606874e-01f, 2.130055428e-01f, 2.660117149e-01f,      \
      2.130055428e-01f, 1.093606874e-01f, 3.600077331e-02f, 7.598758209e-03f, 1.028380124e-03f
// IMAGE_LOSS_WINDOW_END
constexpr float SSIM_C1 = (float)(0.01 * 0.01);
constexpr float SSIM_C2 = (float)(0.03 * 0.03);

// fixed-order sum over the workgroup (xor butterfly inside a wave, waves 0..3 in order); valid in thread 0
__device__ __forceinline__ float block_sum(float v, float* red /*[THREADS / WAVE]*/) {
#pragma unroll
  for (int d = WAVE / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, WAVE);
  __syncthreads();  // red may still be read from the previous call
  if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = v;
  __syncthreads();
  float s = red[0];
#pragma unroll
  for (int w = 1; w < THREADS / WAVE; ++w) s += red[w];
  return s;
}

// stage the (SH x SW) neighbourhood of tile (x0, y0) of one plane, zeros outside the image
__device__ __forceinline__ void stage_plane(const float* __restrict__ plane, int H, int W, int x0, int y0, float* dst) {
  for (int i = threadIdx.x; i < SH * SW; i += THREADS) {
    const int r = i / SW, c = i - r * SW;
    const int gy = y0 - RAD + r, gx = x0 - RAD + c;
    float v = 0.f;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = plane[(int64_t)gy * W + gx];
    dst[i] = v;
  }
}

// six waves per SIMD (what the LDS allows): holds the kernel at 80 VGPRs, one fewer than it takes unasked, without scratch
__global__ __launch_bounds__(THREADS, 6) void image_loss_forward_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                                         const float* __restrict__ Wt, int C, int H, int W,
                                                                         float* __restrict__ keep, int64_t map_stride,
                                                                         float* __restrict__ slots) {
  __shared__ float sx[SH * SW], sy[SH * SW];
  __shared__ float hq[5][SH * TW];
  __shared__ float red[THREADS / WAVE];
  const float g[TAPS] = {GR_IMAGE_LOSS_WINDOW};
  const int vc = blockIdx.z, v = vc / C;
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
  const int64_t plane = (int64_t)vc * H * W;
  stage_plane(X + plane, H, W, x0, y0, sx);
  stage_plane(Y + plane, H, W, x0, y0, sy);
  __syncthreads();

  for (int i = threadIdx.x; i < SH * TW; i += THREADS) {
    const int r = i / TW, c = i - r * TW;
    const float* px = sx + r * SW + c;
    const float* py = sy + r * SW + c;
    float ex = 0.f, ey = 0.f, exx = 0.f, eyy = 0.f, exy = 0.f;
#pragma unroll
    for (int k = 0; k < TAPS; ++k) {
      const float a = px[k], b = py[k];
      ex = fmaf(g[k], a, ex);
      ey = fmaf(g[k], b, ey);
      exx = fmaf(g[k], a * a, exx);
      eyy = fmaf(g[k], b * b, eyy);
      exy = fmaf(g[k], a * b, exy);
    }
    hq[0][i] = ex, hq[1][i] = ey, hq[2][i] = exx, hq[3][i] = eyy, hq[4][i] = exy;
  }
  __syncthreads();

  const int tx = threadIdx.x & (TW - 1), r0 = (threadIdx.x / TW) * ROWS_PER_THREAD;
  float e[5][2];
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    float a0 = 0.f, a1 = 0.f;
#pragma unroll
    for (int j = 0; j <= TAPS; ++j) {  // rows r0 .. r0 + 11 feed taps 0..10 of row r0 and of row r0 + 1, each in tap order
      const float val = hq[q][(r0 + j) * TW + tx];
      if (j < TAPS) a0 = fmaf(g[j], val, a0);
      if (j > 0) a1 = fmaf(g[j - 1], val, a1);
    }
    e[q][0] = a0, e[q][1] = a1;
  }

  float s_l1 = 0.f, s_ss = 0.f, s_w = 0.f;
  const int gx = x0 + tx;
#pragma unroll
  for (int o = 0; o < 2; ++o) {
    const int gy = y0 + r0 + o;
    if (gx < W && gy < H) {
      const float mx = e[0][o], my = e[1][o];
      const float sxx = e[2][o] - mx * mx, syy = e[3][o] - my * my, sxy = e[4][o] - mx * my;
      const float A1 = 2.f * (mx * my) + SSIM_C1, A2 = 2.f * sxy + SSIM_C2;
      const float B1 = (mx * mx + my * my) + SSIM_C1, B2 = (sxx + syy) + SSIM_C2;
      const float den = B1 * B2;
      const float ssim = (A1 * A2) / den;
      const int64_t pix = (int64_t)gy * W + gx;
      const float w = Wt ? Wt[(int64_t)v * H * W + pix] : 1.f;
      const float xv = sx[(r0 + o + RAD) * SW + tx + RAD], yv = sy[(r0 + o + RAD) * SW + tx + RAD];
      s_l1 += w * fabsf(xv - yv);
      s_ss += w * ssim;
      s_w += w;
      if (keep) {
        const float dsxy = (2.f * A1) / den;                                   // d ssim / d sigma_xy
        const float dsx = -(ssim / B2);                                        // d ssim / d sigma_x^2
        const float dmu_direct = (2.f * my * A2) / den - (ssim * (2.f * mx)) / B1;  // d ssim / d mu_x at fixed sigmas
        // sigma_x^2 = E[xx] - mu_x^2 and sigma_xy = E[xy] - mu_x mu_y: total derivative to mu_x at fixed E[xx], E[xy]
        const float dmu = dmu_direct - (2.f * mx) * dsx - my * dsxy;
        keep[plane + pix] = w * dmu;
        keep[map_stride + plane + pix] = w * dsx;
        keep[2 * map_stride + plane + pix] = w * dsxy;
      }
    }
  }
  const float t_l1 = block_sum(s_l1, red), t_ss = block_sum(s_ss, red), t_w = block_sum(s_w, red);
  if (threadIdx.x == 0) {
    const int64_t tile = ((int64_t)vc * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    slots[3 * tile] = t_l1, slots[3 * tile + 1] = t_ss, slots[3 * tile + 2] = t_w;
  }
}

// one workgroup per view: its C * tiles slots in a fixed order (thread t takes slots t, t + 256, ..; then a tree), in double
__global__ __launch_bounds__(THREADS) void image_loss_reduce_kernel(const float* __restrict__ slots, int C, int tiles,
                                                                     float lambda, float* __restrict__ out_loss,
                                                                     float* __restrict__ out_terms) {
  __shared__ double sm[3][THREADS];
  const int v = blockIdx.x;
  const float* s = slots + (int64_t)v * C * tiles * 3;
  double a = 0., b = 0., w = 0.;
  for (int i = threadIdx.x; i < C * tiles; i += THREADS) {
    a += (double)s[3 * i];
    b += (double)s[3 * i + 1];
    if (i < tiles) w += (double)s[3 * i + 2];  // S counts every pixel once: channel 0's tiles
  }
  sm[0][threadIdx.x] = a, sm[1][threadIdx.x] = b, sm[2][threadIdx.x] = w;
  __syncthreads();
  for (int d = THREADS / 2; d > 0; d >>= 1) {
    if ((int)threadIdx.x < d) {
#pragma unroll
      for (int q = 0; q < 3; ++q) sm[q][threadIdx.x] += sm[q][threadIdx.x + d];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double S = sm[2][0];
    double l1 = 0., ss = 0., loss = 0.;
    if (S > 0.) {
      l1 = sm[0][0] / ((double)C * S);
      ss = sm[1][0] / ((double)C * S);
      loss = (1. - (double)lambda) * l1 + (double)lambda * (1. - ss);
    }
    out_loss[v] = (float)loss;
    if (out_terms) out_terms[3 * v] = (float)l1, out_terms[3 * v + 1] = (float)ss, out_terms[3 * v + 2] = (float)S;
  }
}

__global__ __launch_bounds__(THREADS) void image_loss_backward_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                                       const float* __restrict__ Wt, int C, int H, int W,
                                                                       float lambda, const float* __restrict__ keep,
                                                                       int64_t map_stride, const float* __restrict__ terms,
                                                                       const float* __restrict__ dL_dloss,
                                                                       float* __restrict__ dX) {
  __shared__ float sk[3][SH * SW];
  __shared__ float hq[3][SH * TW];
  const float g[TAPS] = {GR_IMAGE_LOSS_WINDOW};
  const int vc = blockIdx.z, v = vc / C;
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
  const int64_t plane = (int64_t)vc * H * W;
  const int tx = threadIdx.x & (TW - 1), r0 = (threadIdx.x / TW) * ROWS_PER_THREAD;
  const int gx = x0 + tx;
  const float S = terms[3 * v + 2];
  if (!(S > 0.f)) {  // uniform over the workgroup: a view without weight has a gradient of exact zeros
#pragma unroll
    for (int o = 0; o < 2; ++o) {
      const int gy = y0 + r0 + o;
      if (gx < W && gy < H) dX[plane + (int64_t)gy * W + gx] = 0.f;
    }
    return;
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) stage_plane(keep + q * map_stride + plane, H, W, x0, y0, sk[q]);
  __syncthreads();
  for (int i = threadIdx.x; i < SH * TW; i += THREADS) {
    const int r = i / TW, c = i - r * TW;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const float* p = sk[q] + r * SW + c;
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < TAPS; ++k) acc = fmaf(g[k], p[k], acc);
      hq[q][i] = acc;
    }
  }
  __syncthreads();
  float e[3][2];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    float a0 = 0.f, a1 = 0.f;
#pragma unroll
    for (int j = 0; j <= TAPS; ++j) {
      const float val = hq[q][(r0 + j) * TW + tx];
      if (j < TAPS) a0 = fmaf(g[j], val, a0);
      if (j > 0) a1 = fmaf(g[j - 1], val, a1);
    }
    e[q][0] = a0, e[q][1] = a1;
  }
  const float scale = dL_dloss[v] / ((float)C * S);
#pragma unroll
  for (int o = 0; o < 2; ++o) {
    const int gy = y0 + r0 + o;
    if (gx < W && gy < H) {
      const int64_t pix = (int64_t)gy * W + gx;
      const float xv = X[plane + pix], yv = Y[plane + pix];
      const float w = Wt ? Wt[(int64_t)v * H * W + pix] : 1.f;
      const float d = xv - yv;
      const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
      const float dssim = e[0][o] + (2.f * xv) * e[1][o] + yv * e[2][o];
      dX[plane + pix] = scale * ((1.f - lambda) * (w * sgn) - lambda * dssim);
    }
  }
}

struct Shape {
  int tiles_x, tiles_y;
  int64_t tiles, planes, elems;
};

int shape_of(int V, int C, int H, int W, Shape* s) {
  GR_REQUIRE(V >= 1 && (C == 1 || C == 3) && H >= 1 && W >= 1, "image loss: V >= 1, C in {1, 3}, H, W >= 1 (got %d %d %d %d)",
             V, C, H, W);
  GR_REQUIRE((int64_t)V * C <= 65535, "image loss: V * C = %lld exceeds 65535 planes per call", (long long)V * C);
  s->tiles_x = (W + TW - 1) / TW;
  s->tiles_y = (H + TH - 1) / TH;
  GR_REQUIRE(s->tiles_y <= 65535, "image loss: H = %d needs more than 65535 tile rows", H);
  s->tiles = (int64_t)s->tiles_x * s->tiles_y;
  s->planes = (int64_t)V * C;
  s->elems = s->planes * H * W;
  GR_REQUIRE(s->tiles * C < (1ll << 31), "image loss: too many tiles per view");
  return GR_OK;
}

}  // namespace
}  // namespace gr

using namespace gr;

extern "C" size_t gr_image_loss_workspace_bytes(int V, int C, int H, int W) {
  Shape s;
  if (shape_of(V, C, H, W, &s) != GR_OK) return 0;
  return align_up((size_t)s.planes * s.tiles * 3 * sizeof(float), 256);
}

extern "C" size_t gr_image_loss_keep_bytes(int V, int C, int H, int W) {
  Shape s;
  if (shape_of(V, C, H, W, &s) != GR_OK) return 0;
  return (size_t)s.elems * 3 * sizeof(float);
}

extern "C" int gr_image_loss_forward(const float* image, const float* target, const float* weight, int V, int C, int H, int W,
                                     float lambda_dssim, float* out_loss, float* out_terms, void* keep, size_t keep_bytes,
                                     void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  Shape s;
  if (int rc = shape_of(V, C, H, W, &s)) return rc;
  GR_REQUIRE(image && target && out_loss && workspace, "image loss forward: null argument");
  GR_REQUIRE(lambda_dssim >= 0.f && lambda_dssim <= 1.f, "image loss: lambda_dssim %g outside [0, 1]", (double)lambda_dssim);
  if (workspace_bytes < gr_image_loss_workspace_bytes(V, C, H, W)) {
    set_error("image loss forward: workspace %zu < %zu bytes", workspace_bytes, gr_image_loss_workspace_bytes(V, C, H, W));
    return GR_ERR_WORKSPACE;
  }
  if (keep && keep_bytes < gr_image_loss_keep_bytes(V, C, H, W)) {
    set_error("image loss forward: keep buffer %zu < %zu bytes", keep_bytes, gr_image_loss_keep_bytes(V, C, H, W));
    return GR_ERR_WORKSPACE;
  }
  float* slots = static_cast<float*>(workspace);
  {
    KernelTimer timer("image_loss_forward", stream);
    hipLaunchKernelGGL(image_loss_forward_kernel, dim3(s.tiles_x, s.tiles_y, (unsigned)s.planes), dim3(THREADS), 0, stream, image,
                       target, weight, C, H, W, static_cast<float*>(keep), s.elems, slots);
    GR_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(image_loss_reduce_kernel, dim3(V), dim3(THREADS), 0, stream, slots, C, (int)s.tiles, lambda_dssim, out_loss,
                     out_terms);
  GR_LAUNCH_CHECK();
  return GR_OK;
}

extern "C" int gr_image_loss_backward(const float* image, const float* target, const float* weight, int V, int C, int H, int W,
                                      float lambda_dssim, const void* keep, size_t keep_bytes, const float* out_terms,
                                      const float* dL_dloss, float* dL_dimage, void* workspace, size_t workspace_bytes,
                                      void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  (void)workspace, (void)workspace_bytes;  // the backward needs no scratch of its own
  Shape s;
  if (int rc = shape_of(V, C, H, W, &s)) return rc;
  GR_REQUIRE(image && target && keep && out_terms && dL_dloss && dL_dimage, "image loss backward: null argument");
  GR_REQUIRE(lambda_dssim >= 0.f && lambda_dssim <= 1.f, "image loss: lambda_dssim %g outside [0, 1]", (double)lambda_dssim);
  if (keep_bytes < gr_image_loss_keep_bytes(V, C, H, W)) {
    set_error("image loss backward: keep buffer %zu < %zu bytes", keep_bytes, gr_image_loss_keep_bytes(V, C, H, W));
    return GR_ERR_WORKSPACE;
  }
  KernelTimer timer("image_loss_backward", stream);
  hipLaunchKernelGGL(image_loss_backward_kernel, dim3(s.tiles_x, s.tiles_y, (unsigned)s.planes), dim3(THREADS), 0, stream, image,
                     target, weight, C, H, W, lambda_dssim, static_cast<const float*>(keep), s.elems, out_terms, dL_dloss,
                     dL_dimage);
  GR_LAUNCH_CHECK();
  return GR_OK;
}
