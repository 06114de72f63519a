// The per-axis quantile grid over a SUPPORT cloud and the exact search in it, shared by scene_init.hip,
// cloud_nn.hip (3.10) and cloud_icp.hip (3.11).  The kernels that build the grid live in cloud_nn.hip; this header holds the
// constants, the device helpers of the search, and the host functions that size and build the support's half of the
// structure.
//
// The grid: D x D x D cells whose boundaries are, per axis, quantiles of a fixed sample of the support's coordinates
// (D ~ cbrt(ns / 3), at most DMAX).  Boundaries are coordinates and cells are found by comparing floats, so there is no
// rounding between a point and its cell:  cell_a(x) = #{c in 1 .. D-1 : B_a[c] <= x}.  The outermost cells are unbounded.
//
// The result of every search is defined by exhaustive enumeration: d(q, p) = ((dx*dx + dy*dy) + dz*dz) in fp32, candidates
// ordered by (d, j).  That order is total, so any search that meets every point that can be among the answer gives the
// same bits.
//
// Face bound, exact in fp32 without slack.  A point p in a cell above c' on axis x has x_p >= B[c' + 1]; if B[c' + 1] >= x_q
// then, fp32 subtraction, multiplication and addition of non-negative terms being monotone,
//   fl(x_p - x_q) >= g = fl(B[c' + 1] - x_q),  fl(dx dx) >= fl(g g),  d(q, p) >= fl(dx dx) >= fl(g g).
// Downwards x_p < B[c'] <= x_q gives the same with g = fl(x_q - B[c']).  After shell r of shell_search the scanned block is
// cells [c - r, c + r] per axis, clamped to the block [L, H] the search is confined to; a point outside it lies behind one
// of the (at most six) faces that still have cells of [L, H] behind them, and bound = min over those faces of fl(g g).  The
// search stops iff best[CAP - 1].d < bound -- strictly, since a point at the same distance with a lower index would
// displace it -- or when the block is exhausted.  What a cap and the support's bounding box add to this is in cloud_nn.hip;
// what the self search leaves out is in scene_init.hip.
#pragma once
#include <cmath>

#include "common.hpp"

namespace gr {

// The support's half of the search structure, carved from a caller's workspace.  count .. misc are contiguous, so one
// memset of zero_bytes from `count` clears them (the caller may carve more words between cursor and misc).
struct SupportGrid {
  float* B;           // (3, DMAX) boundaries
  int32_t* count;     // cells + 1, then the exclusive prefix in place: start of every cell in `sorted`
  int32_t* cursor;    // cells
  int32_t* misc;      // [0] finiteness flag, [4..9] the support's bounding box (cloud_box_kernel); the rest is the caller's
  int32_t* scan_ws;   // scan_ws_ints(cells + 1) at least
  int32_t* cell;      // ns
  float4* sorted;     // ns: (x, y, z, index) in cell order
  int32_t* sorted_cell = nullptr;  // ns: the cell of sorted[s], for a support that is its own query cloud; null: not kept
};

int cloud_grid_dim(int64_t ns);
// memset of [zero_from, zero_from + zero_bytes), boundaries, box (unless !with_box: a search that never reads it), cells,
// scan, scatter of the support; raises misc[0] for a non-finite coordinate
int cloud_build_support_grid(const float* support, int64_t ns, const SupportGrid& g, void* zero_from, size_t zero_bytes,
                             hipStream_t stream, bool with_box = true);

namespace {

constexpr int THREADS = 256;
constexpr int QUERY_THREADS = 128;
constexpr int DMAX = 128;            // cells per axis, at most
constexpr int MAX_SHELLS = 8;
constexpr int FALLBACK_BLOCKS = 4096;  // of THREADS / WAVE waves each, striding over the list
constexpr int32_t NONE = 0x7fffffff;
constexpr int MISC = 12;             // ints of small per-call state behind the cell tables

// #{c in 1 .. D-1 : b[c] <= x}
__device__ __forceinline__ int axis_cell(const float* b, int D, float x) {
  int lo = 0, hi = D - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (b[mid] <= x) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// B -> b[3 * DMAX] in LDS, by the THREADS threads of a workgroup; entries that are no boundary read 0
__device__ __forceinline__ void stage_boundaries(const float* __restrict__ B, int D, float* b) {
  for (int t = threadIdx.x; t < 3 * DMAX; t += THREADS) b[t] = (t % DMAX) >= 1 && (t % DMAX) < D ? B[t] : 0.f;
  __syncthreads();
}

// fl(g g) for the distance of q from the support's extent [lo, hi] on one axis, 0 inside it: every support point p has
// fl((p - q)^2) >= it, by the monotonicity the face bound rests on
__device__ __forceinline__ float axis_base(const uint32_t* __restrict__ box, int a, float q) {
  const float lo = ord2f(~box[a]), hi = ord2f(box[3 + a]);
  const float g = q < lo ? lo - q : q > hi ? q - hi : 0.f;
  return g * g;
}

template <int CAP>
__device__ __forceinline__ void clear_best(float (&bd)[CAP], int32_t (&bj)[CAP]) {
#pragma unroll
  for (int t = 0; t < CAP; ++t) {
    bd[t] = INFINITY;
    bj[t] = NONE;
  }
}

// insert (d, j) into the ascending list of the CAP best under the order (d, j); indices are compile-time after unrolling
template <int CAP>
__device__ __forceinline__ void consider(float (&bd)[CAP], int32_t (&bj)[CAP], float d, int32_t j) {
  if (d < bd[CAP - 1] || (d == bd[CAP - 1] && j < bj[CAP - 1])) {
    bd[CAP - 1] = d;
    bj[CAP - 1] = j;
#pragma unroll
    for (int t = CAP - 1; t > 0; --t) {
      const bool up = bd[t] < bd[t - 1] || (bd[t] == bd[t - 1] && bj[t] < bj[t - 1]);
      const float d0 = bd[t - 1], d1 = bd[t];
      const int32_t j0 = bj[t - 1], j1 = bj[t];
      bd[t - 1] = up ? d1 : d0;
      bd[t] = up ? d0 : d1;
      bj[t - 1] = up ? j1 : j0;
      bj[t] = up ? j0 : j1;
    }
  }
}

// SELF = false: the candidates are the points with d <= cap.  SELF = true (the support is the query cloud, no cap): they
// are the points other than `self`, and cap is not read.
template <int CAP, bool SELF = false>
__device__ __forceinline__ void scan_range(const float4* __restrict__ sorted, int32_t begin, int32_t end, float qx, float qy,
                                           float qz, float cap, float (&bd)[CAP], int32_t (&bj)[CAP], int32_t self = NONE) {
  for (int32_t s = begin; s < end; ++s) {
    const float4 p = sorted[s];
    const float dx = p.x - qx, dy = p.y - qy, dz = p.z - qz;
    const float d = (dx * dx + dy * dy) + dz * dz;
    if (SELF ? __float_as_int(p.w) != self : d <= cap) consider<CAP>(bd, bj, d, __float_as_int(p.w));
  }
}

// cells [L, H] of one axis that a point with d <= cap can lie in; c = the query's cell
__device__ __forceinline__ void axis_reach(const float* __restrict__ b, int D, int c, float q, float cap, int& L, int& H) {
  if (cap == INFINITY) {
    L = 0;
    H = D - 1;
    return;
  }
  L = H = c;
  while (H + 1 <= D - 1) {  // cell H + 1 begins at b[H + 1] > q
    const float g = b[H + 1] - q;
    if (!(g * g <= cap)) break;
    ++H;
  }
  while (L - 1 >= 0) {  // cell L - 1 ends at b[L] <= q
    const float g = q - b[L];
    if (!(g * g <= cap)) break;
    --L;
  }
}

// fl(g g) of the two faces of one axis behind which there are cells of the block [L, H]
__device__ __forceinline__ float axis_bound(const float* __restrict__ b, int L, int H, int c, int r, float q) {
  float bound = INFINITY;
  if (c + r + 1 <= H) {
    const float g = b[c + r + 1] - q;
    bound = g * g;
  }
  if (c - r - 1 >= L) {
    const float g = q - b[c - r];
    bound = fminf(bound, g * g);
  }
  return bound;
}

// The face-bound shell loop: Chebyshev shells of cells around cell c of the query (qx, qy, qz), the CAP best under (d, j)
// among the candidates of scan_range in bd / bj (which the caller has cleared).  true: the result is final; false: no rule
// stopped the search within MAX_SHELLS shells, and bd / bj are to be discarded.  SELF: the block is the whole grid and the
// box is not read -- a support point lies inside the support's box, so every axis_base term would be +0.
template <int CAP, bool SELF = false>
__device__ __forceinline__ bool shell_search(const float4* __restrict__ s_sorted, const int32_t* __restrict__ s_start,
                                             const float* __restrict__ B, const uint32_t* __restrict__ box, int D, int32_t c,
                                             float qx, float qy, float qz, float cap, float (&bd)[CAP], int32_t (&bj)[CAP],
                                             int32_t self = NONE) {
  const int cx = c % D, cy = (c / D) % D, cz = c / (D * D);
  int Lx, Hx, Ly, Hy, Lz, Hz;
  float base_x, base_y, base_z;
  if constexpr (SELF) {
    Lx = Ly = Lz = 0;
    Hx = Hy = Hz = D - 1;
    base_x = base_y = base_z = 0.f;
  } else {
    axis_reach(B, D, cx, qx, cap, Lx, Hx);
    axis_reach(B + DMAX, D, cy, qy, cap, Ly, Hy);
    axis_reach(B + 2 * DMAX, D, cz, qz, cap, Lz, Hz);
    base_x = axis_base(box, 0, qx), base_y = axis_base(box, 1, qy), base_z = axis_base(box, 2, qz);
  }
  for (int r = 0;; ++r) {
    const int x0 = max(cx - r, Lx), x1 = min(cx + r, Hx);
    const int y0 = max(cy - r, Ly), y1 = min(cy + r, Hy);
    const int z0 = max(cz - r, Lz), z1 = min(cz + r, Hz);
    for (int z = z0; z <= z1; ++z) {
      for (int y = y0; y <= y1; ++y) {
        const int32_t row = (z * D + y) * D;
        if (z == cz - r || z == cz + r || y == cy - r || y == cy + r) {  // a face of the shell: cells x0 .. x1 are contiguous
          scan_range<CAP, SELF>(s_sorted, s_start[row + x0], s_start[row + x1 + 1], qx, qy, qz, cap, bd, bj, self);
        } else {  // inside: the two end cells (r > 0 here)
          if (cx - r >= Lx)
            scan_range<CAP, SELF>(s_sorted, s_start[row + cx - r], s_start[row + cx - r + 1], qx, qy, qz, cap, bd, bj, self);
          if (cx + r <= Hx)
            scan_range<CAP, SELF>(s_sorted, s_start[row + cx + r], s_start[row + cx + r + 1], qx, qy, qz, cap, bd, bj, self);
        }
      }
    }
    // a point behind a face of axis a is at least the face away on a and at least the extent's distance on the others;
    // the three lower bounds are added in d's own association, so the sum is a lower bound of d in fp32
    const float fx = axis_bound(B, Lx, Hx, cx, r, qx), fy = axis_bound(B + DMAX, Ly, Hy, cy, r, qy),
                fz = axis_bound(B + 2 * DMAX, Lz, Hz, cz, r, qz);
    const float bound = SELF ? fminf(fx, fminf(fy, fz))
                             : fminf((fx + base_y) + base_z, fminf((base_x + fy) + base_z, (base_x + base_y) + fz));
    if (bd[CAP - 1] < bound) return true;
    // the whole block has been scanned (from L = 0 its extent alone says so, in half the compares)
    if (SELF ? x1 - x0 == Hx && y1 - y0 == Hy && z1 - z0 == Hz
             : x0 == Lx && x1 == Hx && y0 == Ly && y1 == Hy && z0 == Lz && z1 == Hz)
      return true;
    if (r + 1 == MAX_SHELLS) return false;
  }
}

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t u = __shfl_xor((unsigned long long)v, o);
    v = u < v ? u : v;
  }
  return v;
}

}  // namespace
}  // namespace gr
