// Radius search, stage 1 (included by radius_neighbors.hip inside namespace gr::{anonymous}): the uniform grid of the
// supports, the binning of supports and queries into it, and the workspace layout every later stage reads.
//   bbox        per-cloud bounding box of the supports: per-block partial boxes, folded by grid_setup (no atomics)
//   grid_setup  per-cloud cell edge (>= radius, coarsened so cells <= max(4096, 4 n_b)), dims, cell and super-cell bases
//   binning     counting sort in two levels: points -> super-cells of SUP_CELLS consecutive cells (block-local LDS histograms,
//               one global atomic per block and non-empty super-cell), then one workgroup per super-cell sorts its points by
//               cell in LDS and writes the cell table and the cell-ordered float4 {x,y,z,orig index} array
#pragma once

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
  for (int d = WAVE / 2; d > 0; d >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, d, WAVE));
  return v;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
  for (int d = WAVE / 2; d > 0; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d, WAVE));
  return v;
}

struct BatchGrid {  // 64 bytes: copied to LDS as four int4
  double org[3];
  double inv_cell;    // y and z: cells of edge >= r (1 + 2^-10)
  double inv_cell_x;  // x: `xk` sub-cells per cell -- the x window of a query shrinks from 3 r to (2 + 1/xk) r while every
                      // (y, z) row of cells stays one contiguous range of the cell-sorted supports (x is the fastest index)
  int dim[3];         // dim[0] counts the fine x cells
  int cell_base;
  int xk;
  int sup_base;  // first super-cell (SUP_CELLS consecutive cells) of this cloud
};
static_assert(sizeof(BatchGrid) == 64, "BatchGrid is staged in LDS as four int4");

struct RadiusHdr {
  unsigned int max_count;
  unsigned int max_block_hits;
  int total_cells;
  int total_sup;  // super-cells of all clouds
  int slow_sum;   // (thread-per-query kernel) queries the network could not finish: finished exactly by their wave
};

constexpr int RT = 128;
constexpr int SUP_SHIFT = 9, SUP_CELLS = 1 << SUP_SHIFT;
constexpr int COARSE_PTS = 2048;   // points per block of the coarse passes
constexpr int COARSE_BINS = 4096;  // super-cell range a block can histogram in LDS
constexpr int BBOX_PTS = 2048;     // points per block of the bounding-box pass  // queries per block in count/fill (3 threads per query)

struct RadiusWs {
  RadiusHdr* hdr;
  int32_t* q_off;
  int32_t* s_off;
  uint32_t* bbox;
  uint32_t* bbox_partial;  // [blocks][6]
  int32_t* blk_off;
  BatchGrid* grids;
  int32_t* sup_off;    // [batch+1] first super-cell of every cloud
  int32_t* sup_zero;   // [4][nsup+1]: counts (s, q) and cursors (s, q) -- cleared per call
  int32_t* sup_start;  // [2][nsup+1]
  int32_t* s_cell;
  int32_t* q_cell;
  int2* pairs_s;  // (point index, cell), grouped by super-cell
  int2* pairs_q;
  int32_t* start;  // [2][ccap+1] cell starts in the sorted arrays (supports; the query row is unused)
  float4* sorted_s;
  float4* sorted_q;
  int32_t* q_count;    // [3][nq] hits per (z-slab, query)
  int2* q_rng;         // [3 dy][3 slab][nq] candidate range (p0, p1) per band
  unsigned long long* q_mask;  // [3 slab][nq] hit bits in candidate enumeration order
  int32_t* blk_stats;  // [blocks][2]
  float* plane_x;      // [ns + 8] cell-ordered coordinate planes of the supports (tq_kernel)
  float* plane_y;
  float* plane_z;
  uint32_t* tiles;     // [nq rounded up to 64][TQ_ROW_CAP] sorted neighbour indices per query, cell order (tq_kernel, compact mode)
  int64_t ccap;
  int64_t nsup;  // upper bound of the number of super-cells
  size_t bytes;
};

RadiusWs carve(void* ws, int64_t nq, int64_t ns, int64_t batch) {
  RadiusWs w;
  Carver c(ws);
  w.ccap = 4096 * batch + 4 * ns;
  w.nsup = w.ccap / SUP_CELLS + batch + 2;
  w.hdr = c.take<RadiusHdr>(1);
  w.q_off = c.take<int32_t>(3 * (batch + 1));  // q offsets | s offsets | bbox block offsets: one host-to-device copy
  w.s_off = w.q_off + (batch + 1);
  w.blk_off = w.s_off + (batch + 1);
  w.bbox = c.take<uint32_t>(batch * 6);
  w.bbox_partial = c.take<uint32_t>(6 * (ns / BBOX_PTS + batch + 1));
  w.grids = c.take<BatchGrid>(batch);
  w.sup_off = c.take<int32_t>(batch + 1);
  // support side first (sizes depend on ns and batch only): a later call with other queries finds it in place
  w.sup_zero = c.take<int32_t>(4 * (w.nsup + 1));
  w.sup_start = c.take<int32_t>(2 * (w.nsup + 1));
  w.s_cell = c.take<int32_t>(ns);
  w.pairs_s = c.take<int2>(ns);
  w.start = c.take<int32_t>(2 * (w.ccap + 1));
  w.sorted_s = c.take<float4>(ns);
  w.plane_x = c.take<float>(ns + 8);
  w.plane_y = c.take<float>(ns + 8);
  w.plane_z = c.take<float>(ns + 8);
  // query side
  w.q_cell = c.take<int32_t>(nq);
  w.pairs_q = c.take<int2>(nq);
  w.sorted_q = c.take<float4>(nq);
  w.q_count = c.take<int32_t>(3 * nq);
  w.q_rng = c.take<int2>(9 * nq);
  w.q_mask = c.take<unsigned long long>(3 * nq);
  w.blk_stats = c.take<int32_t>(2 * ((nq + 63) / 64 + 8));  // fused_kernel runs 64 queries per workgroup
  w.tiles = c.take<uint32_t>((size_t)((nq + 63) / 64) * 64 * 64);
  w.bytes = c.used();
  return w;
}

// ---------------------------------------------------------------- grid setup
// Per-cloud bounding boxes without atomics: a block reduces one BBOX_PTS-point slice of ONE cloud into six words of
// `partial` (same-address global atomics cost ~60 ns each across XCDs: the shared bbox_kernel of common.hip, six atomics
// per 1024 points, took 32 us of the 8 x 200 k binning); grid_setup_kernel folds the partials.
// Offsets of a call with few clouds travel in the kernel arguments of the FIRST launch (q offsets | s offsets | bbox block
// offsets, nb + 1 entries each): no host -> device copy in front of the binning (a copy-engine operation and the hand-over to
// the first kernel: ~8 us of a 0.36 ms search); block 0 leaves them in the workspace for the launches behind.
constexpr int KARG_CLOUDS = 64;
struct OffsetArgs {
  int32_t v[3 * (KARG_CLOUDS + 1)];
};

template <bool KARG>
__global__ __launch_bounds__(256) void bbox_partial_kernel(const float* __restrict__ pts, const int32_t* __restrict__ off_dev,
                                                           const int32_t* __restrict__ blk_off_dev, int nb,
                                                           uint32_t* __restrict__ partial, int32_t* __restrict__ zero,
                                                           int nzero, const OffsetArgs ka, int32_t* __restrict__ q_off_out) {
  __shared__ uint32_t red[6][256 / WAVE];
  // (the super-cell counters of the counting sort are cleared here, by the way: one launch less in front of every search)
  for (int k = blockIdx.x * 256 + threadIdx.x; k < nzero; k += gridDim.x * 256) zero[k] = 0;
  const int32_t* off = KARG ? ka.v + (nb + 1) : off_dev;           // (the supports' offsets)
  const int32_t* blk_off = KARG ? ka.v + 2 * (nb + 1) : blk_off_dev;
  if (KARG && blockIdx.x == 0)
    for (int k = threadIdx.x; k < 3 * (nb + 1); k += 256) q_off_out[k] = ka.v[k];  // q_off | s_off | blk_off are neighbours
  const int b0 = find_batch(blk_off, nb, (int)blockIdx.x);
  const int p_first = off[b0] + ((int)blockIdx.x - blk_off[b0]) * BBOX_PTS;
  const int p_end = min(off[b0 + 1], p_first + BBOX_PTS);
  const int64_t f0 = (int64_t)p_first * 3;
  const int count = (p_end - p_first) * 3;
  // element f of the flat float stream belongs to axis (f0 + f) % 3; the stride 256 = 1 (mod 3), so a thread's
  // consecutive elements cycle through the axes: slot k of (l3, h3) holds axis (ax0 + k) % 3
  const int ax0 = (int)((f0 + threadIdx.x) % 3);
  const float* src = pts + f0;
  uint32_t l3[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, h3[3] = {0u, 0u, 0u};
  for (int f = threadIdx.x; f < count; f += 6 * 256) {
    uint32_t v[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] = f2ord(src[min(f + k * 256, count - 1)]);  // six independent loads in flight
#pragma unroll
    for (int k = 0; k < 6; ++k)
      if (f + k * 256 < count) {
        l3[k % 3] = min(l3[k % 3], v[k]);
        h3[k % 3] = max(h3[k % 3], v[k]);
      }
  }
  uint32_t lo[3], hi[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int k = a - ax0 < 0 ? a - ax0 + 3 : a - ax0;  // slot that holds axis a
    lo[a] = k == 0 ? l3[0] : (k == 1 ? l3[1] : l3[2]);
    hi[a] = k == 0 ? h3[0] : (k == 1 ? h3[1] : h3[2]);
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] = (uint32_t)wave_min_u32(lo[a]);
    hi[a] = (uint32_t)wave_max_u32(hi[a]);
  }
  const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
  if (lane == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      red[a][w] = lo[a];
      red[3 + a][w] = hi[a];
    }
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    uint32_t v = red[threadIdx.x][0];
#pragma unroll
    for (int i = 1; i < 256 / WAVE; ++i) v = threadIdx.x < 3 ? min(v, red[threadIdx.x][i]) : max(v, red[threadIdx.x][i]);
    partial[(int64_t)blockIdx.x * 6 + threadIdx.x] = v;
  }
}

__global__ void grid_setup_kernel(uint32_t* __restrict__ bbox, const uint32_t* __restrict__ partial,
                                  const int32_t* __restrict__ blk_off,
                                  const int32_t* __restrict__ s_off, int nb, float radius, int xk_max,
                                  BatchGrid* __restrict__ grids, RadiusHdr* __restrict__ hdr,
                                  int32_t* __restrict__ sup_off) {
  // fold the per-block partial boxes: one wave per cloud (looped), lanes over the cloud's blocks
  {
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE, nw = blockDim.x / WAVE;
    for (int b = w; b < nb; b += nw) {
      uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
      for (int k = blk_off[b] + lane; k < blk_off[b + 1]; k += WAVE) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          lo[a] = min(lo[a], partial[(int64_t)k * 6 + a]);
          hi[a] = max(hi[a], partial[(int64_t)k * 6 + 3 + a]);
        }
      }
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        lo[a] = (uint32_t)wave_min_u32(lo[a]);
        hi[a] = (uint32_t)wave_max_u32(hi[a]);
      }
      if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          bbox[b * 6 + a] = lo[a];
          bbox[b * 6 + 3 + a] = hi[a];
        }
      }
    }
    __syncthreads();
  }
  // one thread per cloud (looped), then a serial prefix by thread 0 (nb is small)
  for (int b = threadIdx.x; b < nb; b += blockDim.x) {
    BatchGrid g;
    const int n_b = s_off[b + 1] - s_off[b];
    double cell = fabs((double)radius) * (1.0 + 1.0 / 1024.0);
    if (!(cell > 0.0) || !isfinite(cell)) cell = 1.0;
    g.dim[0] = g.dim[1] = g.dim[2] = 1;
    g.org[0] = g.org[1] = g.org[2] = 0.0;
    if (n_b > 0) {
      double mn[3], mx[3];
      bool finite = true;
      for (int k = 0; k < 3; ++k) {
        mn[k] = (double)ord2f(bbox[b * 6 + k]);
        mx[k] = (double)ord2f(bbox[b * 6 + 3 + k]);
        finite = finite && isfinite(mn[k]) && isfinite(mx[k]);
        g.org[k] = mn[k];
      }
      if (finite) {
        const double cap = (double)max(4096, 4 * n_b);
        bool ok = false;
        for (int it = 0; it < 256; ++it) {
          double e[3], tot = 1.0;
          for (int k = 0; k < 3; ++k) {
            e[k] = floor((mx[k] - mn[k]) / cell) + 1.0;
            tot *= e[k];
          }
          if (tot <= cap) {
            for (int k = 0; k < 3; ++k) g.dim[k] = (int)e[k];
            ok = true;
            break;
          }
          cell *= fmax(cbrt(tot / cap), 1.05);
        }
        if (!ok) cell = INFINITY;  // one cell holds everything (inv_cell = 0): brute force
      } else {
        for (int k = 0; k < 3; ++k) g.org[k] = 0.0;
      }
    }
    g.inv_cell = 1.0 / cell;
    g.inv_cell_x = g.inv_cell;
    g.xk = 1;
    g.sup_base = 0;
    if (n_b > 0 && isfinite(cell) && isfinite(g.inv_cell) && g.inv_cell > 0.0) {
      // refine x only: a support within r of a query is within +-k fine cells of it (|dx| k / cell < k / (1 + 2^-10))
      const double cap = (double)max(4096, 4 * n_b);
      const double ext = (double)ord2f(bbox[b * 6 + 3]) - (double)ord2f(bbox[b * 6]);
      for (int k = xk_max; k > 1; k >>= 1) {
        const double inv_x = (double)k / cell;
        const double ex = floor(ext * inv_x) + 1.0;
        if (isfinite(ex) && ex * (double)g.dim[1] * (double)g.dim[2] <= cap && ex < 2147483647.0) {
          g.xk = k;
          g.inv_cell_x = inv_x;
          g.dim[0] = (int)ex;
          break;
        }
      }
    }
    g.cell_base = 0;
    g.sup_base = 0;
    grids[b] = g;
  }
  // exclusive prefix of the per-cloud cell counts: chunks of blockDim clouds, running carry in LDS
  // (a serial loop over global memory cost ~0.2 us per cloud)
  __shared__ int s_cnt[256], s_sup[256];
  __shared__ int s_carry, s_carry_sup;
  if (threadIdx.x == 0) s_carry = s_carry_sup = 0;
  __syncthreads();
  for (int b0 = 0; b0 < nb; b0 += blockDim.x) {
    const int b = b0 + threadIdx.x;
    const int cells = b < nb ? grids[b].dim[0] * grids[b].dim[1] * grids[b].dim[2] : 0;
    s_cnt[threadIdx.x] = cells;
    s_sup[threadIdx.x] = (cells + SUP_CELLS - 1) >> SUP_SHIFT;
    __syncthreads();
    if (threadIdx.x == 0) {
      int acc = s_carry, acs = s_carry_sup;
      const int live = min((int)blockDim.x, nb - b0);  // (a walk over all 256 slots for 8 clouds was 8 of this launch's 9.6 us)
      for (int k = 0; k < live; ++k) {
        const int c = s_cnt[k], u = s_sup[k];
        s_cnt[k] = acc;
        s_sup[k] = acs;
        acc += c;
        acs += u;
      }
      s_carry = acc;
      s_carry_sup = acs;
    }
    __syncthreads();
    if (b < nb) {
      grids[b].cell_base = s_cnt[threadIdx.x];
      grids[b].sup_base = s_sup[threadIdx.x];
      sup_off[b] = s_sup[threadIdx.x];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    hdr->total_cells = s_carry;
    hdr->total_sup = s_carry_sup;
    hdr->max_count = 0;
    hdr->max_block_hits = 0;
    sup_off[nb] = s_carry_sup;
  }
}

__device__ inline double cell_coord(float x, double org, double inv) {
  return floor(((double)x - org) * inv);
}

__device__ inline int clamped_cell(const BatchGrid& g, float x, float y, float z) {
  int c[3];
  const float p[3] = {x, y, z};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double u = cell_coord(p[k], g.org[k], k == 0 ? g.inv_cell_x : g.inv_cell);
    u = fmin(fmax(u, 0.0), (double)(g.dim[k] - 1));  // NaN -> 0
    c[k] = (int)u;
  }
  return g.cell_base + c[0] + g.dim[0] * (c[1] + g.dim[1] * c[2]);
}

// ---------------------------------------------------------------- binning: two-level counting sort
// (Round 1-2 counted with one returning global atomic per point: device-scope atomics are served behind the per-XCD L2s,
// 1.6 M of them took 64 us, plus a 25 MB clear of the cell table and a three-launch scan over it.)
struct BinSide {
  const float* pts;
  int n;
  const int32_t* off;     // [nb+1] cloud offsets
  int32_t* cell;          // [n] cell of every point (written by the counting pass, read by the scatter pass)
  int2* pairs;            // [n] (point, cell) grouped by super-cell
  int32_t* sup_cnt;       // [nsup+1]
  int32_t* sup_cur;       // [nsup+1]
  int32_t* sup_start;     // [nsup+1]
  float4* sorted;         // [n] {x, y, z, original index} in cell order
  int32_t* cell_start;    // [cells+1] or null (queries need no cell table)
  float* plane_x;         // [n + 8] or null: the same order as coordinate planes (supports only)
  float* plane_y;
  float* plane_z;
};

__global__ void bin_init2_kernel(int32_t* __restrict__ a, int32_t* __restrict__ b, int n) {
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) a[k] = 0, b[k] = 0;
}

// COUNT: cell of every point, LDS histogram over the block's super-cells, one global add per non-empty super-cell.
// SCATTER: the same histogram hands every point its rank inside (block, super-cell); one returning global add per
// non-empty super-cell reserves the block's span; (point, cell) pairs go to their super-cell's range.
template <bool SCATTER>
__global__ __launch_bounds__(256) void coarse_kernel(BinSide A, BinSide B, int blocks_a, int nb,
                                                     const BatchGrid* __restrict__ grids) {
  __shared__ int hist[COARSE_BINS];
  __shared__ int s_info[4];
  const bool second = (int)blockIdx.x >= blocks_a;
  const BinSide& S = second ? B : A;
  const int i0 = ((int)blockIdx.x - (second ? blocks_a : 0)) * COARSE_PTS;
  const int tid = threadIdx.x;
  if (tid == 0) {
    const int last = min(i0 + COARSE_PTS, S.n) - 1;
    const int blo = find_batch(S.off, nb, i0), bhi = find_batch(S.off, nb, last);
    const BatchGrid& gh = grids[bhi];
    s_info[0] = blo;
    s_info[1] = bhi;
    s_info[2] = grids[blo].sup_base;
    s_info[3] = gh.sup_base + ((gh.dim[0] * gh.dim[1] * gh.dim[2] + SUP_CELLS - 1) >> SUP_SHIFT);
  }
  __syncthreads();
  const int blo = s_info[0], bhi = s_info[1], smin = s_info[2], smax = s_info[3];
  const bool in_lds = smax - smin <= COARSE_BINS;  // else: a global atomic per point (clouds with > 2 M cells per block span)
  if (in_lds)
    for (int k = tid; k < smax - smin; k += 256) hist[k] = 0;
  __syncthreads();
  constexpr int PER = COARSE_PTS / 256;
  int sup[PER], rk[PER], cc[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int i = i0 + k * 256 + tid;
    sup[k] = -1;
    rk[k] = 0;
    cc[k] = 0;
    if (i < S.n) {
      int b = blo;
      if (bhi != blo) b = bhi == blo + 1 ? (i >= S.off[bhi] ? bhi : blo) : find_batch(S.off, nb, i);
      const BatchGrid& g = grids[b];
      int c;
      if (SCATTER) {
        c = S.cell[i];
      } else {
        c = clamped_cell(g, S.pts[3 * (int64_t)i], S.pts[3 * (int64_t)i + 1], S.pts[3 * (int64_t)i + 2]);
        S.cell[i] = c;
      }
      cc[k] = c;
      sup[k] = g.sup_base + ((c - g.cell_base) >> SUP_SHIFT);
      if (in_lds) {
        if (SCATTER) rk[k] = atomicAdd(&hist[sup[k] - smin], 1);
        else atomicAdd(&hist[sup[k] - smin], 1);
      } else {
        if (SCATTER) rk[k] = atomicAdd(&S.sup_cur[sup[k]], 1);
        else atomicAdd(&S.sup_cnt[sup[k]], 1);
      }
    }
  }
  __syncthreads();
  if (in_lds) {
    for (int k = tid; k < smax - smin; k += 256) {
      const int cnt = hist[k];
      if (cnt) {
        if (SCATTER) hist[k] = atomicAdd(&S.sup_cur[smin + k], cnt);  // the block's span inside the super-cell
        else atomicAdd(&S.sup_cnt[smin + k], cnt);
      }
    }
  }
  if (!SCATTER) return;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int i = i0 + k * 256 + tid;
    if (sup[k] >= 0) {
      const int dst = S.sup_start[sup[k]] + (in_lds ? hist[sup[k] - smin] : 0) + rk[k];
      S.pairs[dst] = make_int2(i, cc[k]);
    }
  }
}

// exclusive scan of the super-cell counts (one block per side; total_sup is only known on the device)
__global__ __launch_bounds__(1024) void sup_scan_kernel(BinSide A, BinSide B, int first_side, const RadiusHdr* __restrict__ hdr) {
  const BinSide& S = ((int)blockIdx.x + first_side) ? B : A;
  __shared__ int wsum[1024 / WAVE];
  __shared__ int s_carry;
  const int n = hdr->total_sup, tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
  if (tid == 0) s_carry = 0;
  __syncthreads();
  for (int i0 = 0; i0 < n; i0 += 1024) {
    const int i = i0 + tid;
    const int v = i < n ? S.sup_cnt[i] : 0;
    const int inc = wave_incl_scan_add_dpp(v);
    if (lane == WAVE - 1) wsum[w] = inc;
    __syncthreads();
    int base = s_carry, tot = 0;
#pragma unroll
    for (int k = 0; k < 1024 / WAVE; ++k) {
      const int x = wsum[k];
      if (k < w) base += x;
      tot += x;
    }
    if (i < n) S.sup_start[i] = base + inc - v;
    __syncthreads();
    if (tid == 0) s_carry += tot;
    __syncthreads();
  }
  if (tid == 0) S.sup_start[n] = s_carry;
}

// one workgroup per super-cell (grid-stride: the number of super-cells is only known on the device): LDS histogram of its
// <= SUP_CELLS cells, scan -> cell starts, scatter into cell order.  A thread keeps up to FINE_PER of the super-cell's points
// in registers: the (point, cell) pairs are read once and the coordinates are requested before the LDS work starts.
constexpr int FINE_PER = 8;

__global__ __launch_bounds__(256) void fine_kernel(BinSide A, BinSide B, int blocks_a, int nb,
                                                   const BatchGrid* __restrict__ grids, const int32_t* __restrict__ sup_off,
                                                   const RadiusHdr* __restrict__ hdr) {
  __shared__ int hist[SUP_CELLS];
  __shared__ int wsum[256 / WAVE];
  __shared__ float4 stage[256 * FINE_PER];  // the super-cell in cell order: leaves as coalesced copies (records + planes)
  const bool second = (int)blockIdx.x >= blocks_a;
  const BinSide& S = second ? B : A;
  const int stride = second ? (int)gridDim.x - blocks_a : blocks_a;
  const int total_sup = hdr->total_sup;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
  for (int sc = (int)blockIdx.x - (second ? blocks_a : 0); sc < total_sup; sc += stride) {
    const int a = S.sup_start[sc], e = S.sup_start[sc + 1];
    const int b = find_batch(sup_off, nb, sc);
    const BatchGrid& g = grids[b];
    const int ls = sc - g.sup_base;
    const int first = g.cell_base + ls * SUP_CELLS;
    const int ncell = min(SUP_CELLS, g.dim[0] * g.dim[1] * g.dim[2] - ls * SUP_CELLS);
    hist[tid] = 0;
    hist[tid + 256] = 0;
    const bool in_regs = e > a && e - a <= 256 * FINE_PER;
    int2 pr[FINE_PER];
    float cx[FINE_PER], cy[FINE_PER], cz[FINE_PER];
    if (in_regs) {
#pragma unroll
      for (int k = 0; k < FINE_PER; ++k) pr[k] = S.pairs[min(a + k * 256 + tid, e - 1)];
#pragma unroll
      for (int k = 0; k < FINE_PER; ++k) {
        const float* src = S.pts + 3 * (int64_t)pr[k].x;
        cx[k] = src[0];
        cy[k] = src[1];
        cz[k] = src[2];
      }
    }
    __syncthreads();
    if (in_regs) {
#pragma unroll
      for (int k = 0; k < FINE_PER; ++k)
        if (a + k * 256 + tid < e) atomicAdd(&hist[pr[k].y - first], 1);
    } else {
      for (int p = a + tid; p < e; p += 256) atomicAdd(&hist[S.pairs[p].y - first], 1);
    }
    __syncthreads();
    const int v0 = hist[2 * tid], v1 = hist[2 * tid + 1];
    const int inc = wave_incl_scan_add_dpp(v0 + v1);
    if (lane == WAVE - 1) wsum[w] = inc;
    __syncthreads();
    int base = 0;
#pragma unroll
    for (int k = 0; k < 256 / WAVE; ++k)
      if (k < w) base += wsum[k];
    const int ex = base + inc - (v0 + v1);
    hist[2 * tid] = ex;  // becomes the cursor of the cell
    hist[2 * tid + 1] = ex + v0;
    if (S.cell_start) {
      if (2 * tid < ncell) S.cell_start[first + 2 * tid] = a + ex;
      if (2 * tid + 1 < ncell) S.cell_start[first + 2 * tid + 1] = a + ex + v0;
      if (sc == total_sup - 1 && tid == 0) S.cell_start[first + ncell] = e;  // end of the last cell of the last cloud
    }
    __syncthreads();
    // order inside a cell: arrival (the search results do not depend on it)
    if (in_regs) {
#pragma unroll
      for (int k = 0; k < FINE_PER; ++k)
        if (a + k * 256 + tid < e) {
          const int slot = atomicAdd(&hist[pr[k].y - first], 1);
          stage[slot] = make_float4(cx[k], cy[k], cz[k], __int_as_float(pr[k].x));
        }
      __syncthreads();
      // (scattering 16 + 3 x 4 bytes per point straight to global memory took 49 us of the 8 x 200 k binning; staged: 29)
      for (int p = tid; p < e - a; p += 256) {
        const float4 v = stage[p];
        S.sorted[a + p] = v;
        if (S.plane_x) {
          S.plane_x[a + p] = v.x;
          S.plane_y[a + p] = v.y;
          S.plane_z[a + p] = v.z;
        }
      }
    } else {
      for (int p = a + tid; p < e; p += 256) {
        const int2 q = S.pairs[p];
        const int slot = atomicAdd(&hist[q.y - first], 1);
        const float* src = S.pts + 3 * (int64_t)q.x;
        S.sorted[a + slot] = make_float4(src[0], src[1], src[2], __int_as_float(q.x));
        if (S.plane_x) {
          S.plane_x[a + slot] = src[0];
          S.plane_y[a + slot] = src[1];
          S.plane_z[a + slot] = src[2];
        }
      }
    }
    __syncthreads();  // hist is cleared by the next super-cell of this workgroup
  }
}
