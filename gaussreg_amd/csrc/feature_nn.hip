// Nearest neighbours in feature space: for every row of x the nearest row of y and for every row of y the nearest row of x,
// under the distance of gr_pairwise_distance, without ever writing the n x m matrix (include/gaussreg_hip_feature_nn.h,
// DESIGN.md 3.12).
//
// Replaces the cKDTree searches of
//   geotransformer/utils/registration.py:210-265   extract_corr_indices_from_feats / extract_correspondences_from_feats
//
// The contraction is pairwise_big_kernel's (superpoint_matching.hip): 128 x 128 per workgroup, four waves of 2 x 2
// accumulators of 32 x 32, k-slabs of 16 through two LDS buffers, the same three fetches -- so every d(i, j) has the bits
// of gr_pairwise_distance.  A workgroup owns ONE row tile and sweeps a strip of consecutive column tiles:
//   rows     every lane keeps a running (d, j) minimum per accumulator row (32 of them) across the whole strip -- lane-local
//            compares, j ascending, strict <, so the lowest index wins -- and the 32 lanes of a half-wave are folded once per
//            strip, not once per tile;
//   columns  a lane owns a column of each 32 x 32 block: 32 lane-local compares per block, one exchange between the two
//            half-waves, one LDS exchange between the two wave rows, per tile.
// Both leave through ONE 64-bit integer atomicMin per row per strip / per column per tile on the packed key
// (bits(d) << 32 | index): d >= 0 so the bit pattern is monotone, and the minimum over a total order does not depend on
// the order of arrival.  An atomic is skipped when the key already stored is not larger (a relaxed atomic load: keys only
// ever decrease, so an older value can only cause an atomic too many, never one too few).  No float atomics.
#include <algorithm>

#include "../../include/gaussreg_hip_feature_nn.h"
#include "common.hpp"
#include "mfma_tile.hpp"

namespace gr {
namespace {

constexpr int FN_T = 128;  // output tile per workgroup
constexpr int FN_K = 16;   // k-slab
constexpr int FN_LD = FN_K + 1;
constexpr int64_t FN_MAX_C = GR_FEATURE_NN_MAX_C;
constexpr uint32_t FN_INF = 0x7f800000u;
typedef unsigned long long u64;

// The strip: how many consecutive column tiles one workgroup sweeps.  Long enough that the once-per-strip fold of the row
// minima is amortised (8 tiles where the matrix has them), short enough that about 4096 workgroups exist for the 512 slots
// of the chip (256 CUs x 2): the tail of the last round is then a small share of the run.
inline int fn_strip_tiles(int64_t rt, int64_t ct) {
  const int64_t strips = std::min(std::max<int64_t>((4096 + rt - 1) / rt, 1), ct);
  const int64_t by_target = (ct + strips - 1) / strips;
  const int64_t by_fill = std::min<int64_t>(8, rt * ct / 512);
  return (int)std::min(std::max<int64_t>(std::max(by_target, by_fill), 1), ct);
}

// squared norms of the rows, summed exactly as sqnorm_kernel of superpoint_matching.hip sums them (one wave per row, lanes
// stride the channels, xor butterfly 32 .. 1)
__global__ __launch_bounds__(256) void fn_sqnorm_kernel(const float* __restrict__ x, int n, int C, float* __restrict__ out) {
  const int row = blockIdx.x * (256 / WAVE) + (int)(threadIdx.x / WAVE), lane = threadIdx.x & (WAVE - 1);
  if (row >= n) return;
  const float* r = x + (int64_t)row * C;
  float s = 0.f;
  for (int k = lane; k < C; k += WAVE) {
    const float v = r[k];
    s += v * v;
  }
#pragma unroll
  for (int d = WAVE / 2; d > 0; d >>= 1) s += __shfl_xor(s, d, WAVE);
  if (lane == 0) out[row] = s;
}

// pd_distance<EPI_DIST> of superpoint_matching.hip, then the order key: the clamp at 0, the sign bit dropped (-0 and +0
// are one distance), NaN -- only a norm that overflowed can make one from finite features -- ordered and reported as +inf.
// `normalized` enters as x2 = 2, y2 = 0: (2 - 2 xy) + 0 has the bits of 2 - 2 xy.  A row or column outside the matrix
// enters as a norm of +inf: its key is +inf's and its index exceeds every real one, so it loses to every real candidate.
__device__ __forceinline__ uint32_t fn_key(float xy, float x2, float y2) {
  float d = (x2 - 2.0f * xy) + y2;
  d = d < 0.0f ? 0.0f : d;
  return min(__float_as_uint(d) & 0x7fffffffu, FN_INF);
}

__device__ __forceinline__ void fn_push(u64* __restrict__ slot, u64 key) {
  if (key < __atomic_load_n(slot, __ATOMIC_RELAXED)) atomicMin(slot, key);
}

template <bool ALIGNED, bool ROWS, bool COLS>
__global__ __launch_bounds__(256, 2) void feature_nn_kernel(const float* __restrict__ x, const float* __restrict__ y, int n,
                                                            int m, int C, int normalized, const float* __restrict__ x2,
                                                            const float* __restrict__ y2, int strip_tiles,
                                                            u64* __restrict__ row_key, u64* __restrict__ col_key) {
  __shared__ float sx[2][FN_T][FN_LD];
  __shared__ float sy[2][FN_T][FN_LD];
  __shared__ float s_x2[FN_T];
  __shared__ u64 s_ckey[2][FN_T];  // [wave row][column of the tile]
  __shared__ u64 s_rkey[2][FN_T];  // [wave column][row of the tile]
  const int i0 = blockIdx.x * FN_T;
  const int ct = (m + FN_T - 1) / FN_T;
  const int t_begin = blockIdx.y * strip_tiles, t_end = min(ct, t_begin + strip_tiles);
  if (i0 >= n || t_begin >= t_end) return;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wr = w >> 1, wc = w & 1;
  const int wi = wr * 64, wj = wc * 64;  // wave's 64 x 64 sub-tile
  // staging: thread -> (row sr + 64 u, four consecutive k), as pairwise_big_kernel
  const int sr = tid >> 2, sk = (tid & 3) * 4;
  const float* xrow[2];
  const float* yrow[2];
  bool xok[2], yok[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int gi = i0 + sr + 64 * u;
    xok[u] = gi < n;
    xrow[u] = x + (int64_t)(xok[u] ? gi : 0) * C;
  }
  auto aim = [&](int t) {  // the y rows of column tile t
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int gj = t * FN_T + sr + 64 * u;
      yok[u] = gj < m;
      yrow[u] = y + (int64_t)(yok[u] ? gj : 0) * C;
    }
  };
  const bool vec = (C % 4 == 0) && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) % 16 == 0);
  auto fetch = [&](const float* row, bool ok, int k0) -> float4 {
    const int gk = k0 + sk;
    if (ALIGNED) {
      const float4 t = *reinterpret_cast<const float4*>(row + gk);  // rows out of range read row 0 and are zeroed here
      return ok ? t : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    const int ce = ok ? C : 0;  // a row out of range has no channels
    if (vec && gk + 4 <= ce) {
      v = *reinterpret_cast<const float4*>(row + gk);
    } else {
      if (gk < ce) v.x = row[gk];
      if (gk + 1 < ce) v.y = row[gk + 1];
      if (gk + 2 < ce) v.z = row[gk + 2];
      if (gk + 3 < ce) v.w = row[gk + 3];
    }
    return v;
  };
  auto stash = [&](float (*dst)[FN_LD], int u, const float4 v) {
    float* d = &dst[sr + 64 * u][sk];
    d[0] = v.x;
    d[1] = v.y;
    d[2] = v.z;
    d[3] = v.w;
  };
  f32x16 acc[2][2];
  mfma_zero(acc);
  // the running row minima of the strip: (a, r) -> the smallest key this lane has seen in its columns, and where
  uint32_t bru[2][16];
  int brj[2][16];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) bru[a][r] = 0xffffffffu, brj[a][r] = 0x7fffffff;
  float4 rx[2], ry[2];
  aim(t_begin);
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    rx[u] = fetch(xrow[u], xok[u], 0);
    ry[u] = fetch(yrow[u], yok[u], 0);
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    stash(sx[0], u, rx[u]);
    stash(sy[0], u, ry[u]);
  }
  if (tid < FN_T) s_x2[tid] = i0 + tid < n ? (normalized ? 2.0f : x2[i0 + tid]) : __uint_as_float(FN_INF);
  __syncthreads();
  const int slabs = (C + FN_K - 1) / FN_K;
  int cur = 0;

  // one tile's distances into the minima
  float yy[2];  // the squared norms of the lane's two columns, requested before the tile's k loop
  auto epilogue = [&](int j0) {
    int gjb[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) gjb[b] = mfma_col(j0 + wj + 32 * b, lane);
    uint32_t cu[2] = {0xffffffffu, 0xffffffffu};
    int ci[2] = {0x7fffffff, 0x7fffffff};
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int li = mfma_row(wi + 32 * a, r, lane), gi = i0 + li;
        const float xx = s_x2[li];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const uint32_t u = fn_key(acc[a][b][r], xx, yy[b]);
          if (ROWS && u < bru[a][r]) bru[a][r] = u, brj[a][r] = gjb[b];  // j ascends along the sweep: the first of equals stays
          if (COLS && u < cu[b]) cu[b] = u, ci[b] = gi;                   // i ascends with (a, r)
        }
      }
    if (COLS) {
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        u64 key = ((u64)cu[b] << 32) | (uint32_t)ci[b];
        key = min(key, (u64)__shfl_xor(key, 32, WAVE));
        if (lane < 32) s_ckey[wr][wj + 32 * b + lane] = key;
      }
      __syncthreads();  // (the next write of s_ckey comes after the barrier of the next tile's first slab)
      if (tid < FN_T && j0 + tid < m) fn_push(col_key + j0 + tid, min(s_ckey[0][tid], s_ckey[1][tid]));
    }
  };

  for (int t = t_begin; t < t_end; ++t) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int gj = mfma_col(t * FN_T + wj + 32 * b, lane);
      yy[b] = gj < m ? (normalized ? 0.f : y2[gj]) : __uint_as_float(FN_INF);
    }
    for (int sidx = 0; sidx < slabs; ++sidx) {
      const bool last = sidx + 1 == slabs;
      const bool more = !last || t + 1 < t_end;  // the next slab: of this tile, or the first of the next
      if (more) {
        if (last) aim(t + 1);
        const int k0 = last ? 0 : (sidx + 1) * FN_K;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          rx[u] = fetch(xrow[u], xok[u], k0);
          ry[u] = fetch(yrow[u], yok[u], k0);
        }
      }
      mfma_slab<FN_K>(acc, sx[cur], sy[cur], wi, wj, lane);
      if (more) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          stash(sx[cur ^ 1], u, rx[u]);
          stash(sy[cur ^ 1], u, ry[u]);
        }
      }
      __syncthreads();
      cur ^= 1;
    }
    const int j0 = t * FN_T;
    epilogue(j0);
    mfma_zero(acc);
  }

  if (ROWS) {  // once per strip: fold the 32 lanes of each half-wave, then the two wave columns
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        u64 key = ((u64)bru[a][r] << 32) | (uint32_t)brj[a][r];
#pragma unroll
        for (int d = 16; d > 0; d >>= 1) key = min(key, (u64)__shfl_xor(key, d, WAVE));
        if ((lane & 31) == 0) s_rkey[wc][mfma_row(wi + 32 * a, r, lane)] = key;
      }
    __syncthreads();
    if (tid < FN_T && i0 + tid < n) fn_push(row_key + i0 + tid, min(s_rkey[0][tid], s_rkey[1][tid]));
  }
}

// keys -> (index, dist2); a key nobody lowered (the other side is empty) -> -1 / +inf
__global__ __launch_bounds__(256) void fn_finish_kernel(const u64* __restrict__ row_key, int64_t n, const u64* __restrict__ col_key,
                                                        int64_t m, int64_t* __restrict__ row_index, float* __restrict__ row_dist2,
                                                        int64_t* __restrict__ col_index, float* __restrict__ col_dist2) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool is_row = e < n;
  const int64_t k = is_row ? e : e - n;
  if (!is_row && k >= m) return;
  const u64 key = is_row ? row_key[k] : col_key[k];
  const bool none = key == ~0ull;
  (is_row ? row_index : col_index)[k] = none ? -1 : (int64_t)(key & 0xffffffffull);
  (is_row ? row_dist2 : col_dist2)[k] = __uint_as_float(none ? FN_INF : (uint32_t)(key >> 32));
}

inline bool fn_shape_ok(int64_t n, int64_t m, int64_t c) {
  return n >= 0 && m >= 0 && n < (1ll << 31) - FN_T && m < (1ll << 31) - FN_T && c >= 1 && c <= FN_MAX_C;
}

}  // namespace
}  // namespace gr

using namespace gr;

// row keys, column keys (8 B each), squared norms (4 B each), four 256-byte carves
extern "C" size_t gr_feature_nn_workspace_bytes(int64_t n, int64_t m, int64_t c) {
  if (!fn_shape_ok(n, m, c)) return 0;
  Carver cv(nullptr);
  cv.take<u64>((size_t)n);
  cv.take<u64>((size_t)m);
  cv.take<float>((size_t)n);
  cv.take<float>((size_t)m);
  return std::max<size_t>(cv.used(), 256);
}

extern "C" int gr_feature_nn(const float* x, int64_t n, const float* y, int64_t m, int64_t c, int normalized,
                             int64_t* row_index, float* row_dist2, int64_t* col_index, float* col_dist2, void* ws,
                             size_t ws_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  GR_REQUIRE(fn_shape_ok(n, m, c), "feature_nn: bad sizes (0 <= n, m < 2^31 - 128, 1 <= c <= %lld)", (long long)FN_MAX_C);
  GR_REQUIRE((row_index != nullptr) == (row_dist2 != nullptr) && (col_index != nullptr) == (col_dist2 != nullptr),
             "feature_nn: an index output and its dist2 output are given together or not at all");
  const bool rows = row_index != nullptr, cols = col_index != nullptr;
  GR_REQUIRE(rows || cols, "feature_nn: neither the row nor the column outputs are requested");
  GR_REQUIRE((x || n == 0) && (y || m == 0), "feature_nn: null argument");
  const int64_t nr = rows ? n : 0, nc = cols ? m : 0;
  if (nr + nc == 0) return GR_OK;
  if (!ws || ws_bytes < gr_feature_nn_workspace_bytes(n, m, c)) {
    set_error("feature_nn workspace too small");
    return GR_ERR_WORKSPACE;
  }
  Carver cv(ws);
  u64* row_key = cv.take<u64>((size_t)n);
  u64* col_key = cv.take<u64>((size_t)m);
  float* x2 = cv.take<float>((size_t)n);
  float* y2 = cv.take<float>((size_t)m);
  if (nr) GR_HIP(hipMemsetAsync(row_key, 0xff, sizeof(u64) * (size_t)n, stream));
  if (nc) GR_HIP(hipMemsetAsync(col_key, 0xff, sizeof(u64) * (size_t)m, stream));
  if (n > 0 && m > 0) {
    if (!normalized) {
      hipLaunchKernelGGL(fn_sqnorm_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream, x, (int)n, (int)c, x2);
      hipLaunchKernelGGL(fn_sqnorm_kernel, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, stream, y, (int)m, (int)c, y2);
    } else {
      x2 = y2 = nullptr;
    }
    KernelTimer timer("feature_nn", stream);
    const int64_t rt = (n + FN_T - 1) / FN_T, ct = (m + FN_T - 1) / FN_T;
    const int strip = fn_strip_tiles(rt, ct);
    const dim3 grid((unsigned)rt, (unsigned)((ct + strip - 1) / strip));
    const bool aligned = c % FN_K == 0 && (reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) % 16 == 0;
    auto kern = rows && cols ? (aligned ? feature_nn_kernel<true, true, true> : feature_nn_kernel<false, true, true>)
                : rows       ? (aligned ? feature_nn_kernel<true, true, false> : feature_nn_kernel<false, true, false>)
                             : (aligned ? feature_nn_kernel<true, false, true> : feature_nn_kernel<false, false, true>);
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, stream, x, y, (int)n, (int)m, (int)c, normalized, (const float*)x2,
                       (const float*)y2, strip, row_key, col_key);
    GR_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(fn_finish_kernel, dim3((unsigned)((nr + nc + 255) / 256)), dim3(256), 0, stream, row_key, nr, col_key, nc,
                     row_index, row_dist2, col_index, col_dist2);
  GR_LAUNCH_CHECK();
  return GR_OK;
}
