// The per-axis quantile grid over a SUPPORT cloud and the exact capped search in it, shared by cloud_nn.hip (DESIGN.md 3.10:
// the definition, the face bound and its proof are at the top of that file) and cloud_icp.hip (3.11).  The kernels that
// build the grid live in cloud_nn.hip; this header holds the constants, the device helpers of the search, and the host
// functions that size and build the support's half of the structure.
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
};

int cloud_grid_dim(int64_t ns);
// memset of [zero_from, zero_from + zero_bytes), boundaries, box, cells, scan, scatter of the support; raises misc[0] for
// a non-finite coordinate
int cloud_build_support_grid(const float* support, int64_t ns, const SupportGrid& g, void* zero_from, size_t zero_bytes,
                             hipStream_t stream);

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

// fl(g g) for the distance of q from the support's extent [lo, hi] on one axis, 0 inside it: every support point p has
// fl((p - q)^2) >= it, by the monotonicity the face bound rests on
__device__ __forceinline__ float axis_base(const uint32_t* __restrict__ box, int a, float q) {
  const float lo = ord2f(~box[a]), hi = ord2f(box[3 + a]);
  const float g = q < lo ? lo - q : q > hi ? q - hi : 0.f;
  return g * g;
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

template <int CAP>
__device__ __forceinline__ void scan_range(const float4* __restrict__ sorted, int32_t begin, int32_t end, float qx, float qy,
                                           float qz, float cap, float (&bd)[CAP], int32_t (&bj)[CAP]) {
  for (int32_t s = begin; s < end; ++s) {
    const float4 p = sorted[s];
    const float dx = p.x - qx, dy = p.y - qy, dz = p.z - qz;
    const float d = (dx * dx + dy * dy) + dz * dz;
    if (d <= cap) consider<CAP>(bd, bj, d, __float_as_int(p.w));
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
// among the points with d <= cap in bd / bj (which the caller has set to +inf / NONE).  true: the result is final; false:
// no rule stopped the search within MAX_SHELLS shells, and bd / bj are to be discarded.
template <int CAP>
__device__ __forceinline__ bool shell_search(const float4* __restrict__ s_sorted, const int32_t* __restrict__ s_start,
                                             const float* __restrict__ B, const uint32_t* __restrict__ box, int D, int32_t c,
                                             float qx, float qy, float qz, float cap, float (&bd)[CAP], int32_t (&bj)[CAP]) {
  const int cx = c % D, cy = (c / D) % D, cz = c / (D * D);
  int Lx, Hx, Ly, Hy, Lz, Hz;
  axis_reach(B, D, cx, qx, cap, Lx, Hx);
  axis_reach(B + DMAX, D, cy, qy, cap, Ly, Hy);
  axis_reach(B + 2 * DMAX, D, cz, qz, cap, Lz, Hz);
  const float base_x = axis_base(box, 0, qx), base_y = axis_base(box, 1, qy), base_z = axis_base(box, 2, qz);
  for (int r = 0;; ++r) {
    const int x0 = max(cx - r, Lx), x1 = min(cx + r, Hx);
    const int y0 = max(cy - r, Ly), y1 = min(cy + r, Hy);
    const int z0 = max(cz - r, Lz), z1 = min(cz + r, Hz);
    for (int z = z0; z <= z1; ++z) {
      for (int y = y0; y <= y1; ++y) {
        const int32_t row = (z * D + y) * D;
        if (z == cz - r || z == cz + r || y == cy - r || y == cy + r) {  // a face of the shell: cells x0 .. x1 are contiguous
          scan_range<CAP>(s_sorted, s_start[row + x0], s_start[row + x1 + 1], qx, qy, qz, cap, bd, bj);
        } else {  // inside: the two end cells (r > 0 here)
          if (cx - r >= Lx) scan_range<CAP>(s_sorted, s_start[row + cx - r], s_start[row + cx - r + 1], qx, qy, qz, cap, bd, bj);
          if (cx + r <= Hx) scan_range<CAP>(s_sorted, s_start[row + cx + r], s_start[row + cx + r + 1], qx, qy, qz, cap, bd, bj);
        }
      }
    }
    // a point behind a face of axis a is at least the face away on a and at least the extent's distance on the others;
    // the three lower bounds are added in d's own association, so the sum is a lower bound of d in fp32
    const float fx = axis_bound(B, Lx, Hx, cx, r, qx), fy = axis_bound(B + DMAX, Ly, Hy, cy, r, qy),
                fz = axis_bound(B + 2 * DMAX, Lz, Hz, cz, r, qz);
    const float bound = fminf((fx + base_y) + base_z, fminf((base_x + fy) + base_z, (base_x + base_y) + fz));
    if (bd[CAP - 1] < bound) return true;
    if (x0 == Lx && x1 == Hx && y0 == Ly && y1 == Hy && z0 == Lz && z1 == Hz) return true;  // the whole block has been scanned
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
