// Radius search, count + fill: the two-pass path (gr_radius_search mode 0, and wherever another kernel gives up).
//   count  thread per (cell-ordered query, z-slab): candidates staged in LDS as coordinate planes, tested two at a time with
//          packed fp32 math; per thread a hit count, the nine candidate ranges and a hit bit mask; max over queries -> host
//   fill   gathers only the hits named by the masks into per-query LDS segments, ranks every hit inside its segment by
//          counting (one thread per hit) and stores it at out[query][rank]; pads the rows
#pragma once

// ---------------------------------------------------------------- candidate traversal
// A block owns RQ consecutive cell-ordered queries and runs 3*RQ threads: thread (j, slot) walks
// the three (dy, dz = j-1) bands of query `slot`, so a wave holds 64 neighbouring queries looking
// at the same z-slab.  Cells are numbered x-fastest, hence the union of the block's 27-cell
// neighbourhoods is nine (dy,dz) "bands", each a CONTIGUOUS range of the cell-sorted support array.
// The block stages those ranges in LDS with coalesced float4 loads (falls back to direct global
// reads if they do not fit) and every thread then walks its own candidates out of LDS, four
// independent ds_read_b128 in flight per step.
//   COUNT pass: hits per (query, z-slab) -> q_cnt[3][nq]; per-block max / sum -> blk_stats
//   FILL  pass: phase A appends (dist,index) keys unsorted into per-query LDS segments (the slab
//               sub-counts give every thread a private sub-segment: no atomics);
//               phase B gives each hit one thread, ranks it inside its segment (branch-free
//               counting; segment reads are LDS broadcasts) and stores it straight to its final
//               slot out[query][rank]; padding is written one row per wave.
typedef float f32x2 __attribute__((ext_vector_type(2)));
constexpr int NBAND = 9;
constexpr int NSUB = 3;  // threads per query (one per z-slab)
constexpr int GB = 8;    // hit loads in flight per thread in the FILL gather

template <int RQ>
struct TravLds {
  static constexpr int THREADS = NSUB * RQ;
  static constexpr int STAGE_CAP = 12 * RQ;  // candidates the block can stage
  // ints: offs[RQ+1], orig[RQ], wsum[THREADS/64], sub[3*RQ], band_lo[9], band_hi[9], band_base[10]
  static constexpr int TABLE_MAX = 256;  // clouds whose offsets / grids are cached in LDS (sized per launch)
  static constexpr int N_INTS = (RQ + 1) + RQ + NSUB * RQ + 9 + 9 + 10 + THREADS / WAVE;
  static constexpr size_t TABLE_OFF = (size_t)(N_INTS * 4 + 15) / 16 * 16;
  // the FILL pass only needs offs, orig and wsum (laid out first): its hit segments start right after them
  static constexpr size_t FILL_OFF = (size_t)(((RQ + 1) + RQ + THREADS / WAVE) * 4 + 15) / 16 * 16;
  // COUNT pass: [int tables | q offsets of `tcap` clouds | their grids | candidate planes]
  static __host__ __device__ size_t tables_bytes(int tcap) { return tcap > 0 ? ((size_t)(tcap + 1) * 4 + 15) / 16 * 16 + (size_t)tcap * sizeof(BatchGrid) : 0; }
  static constexpr size_t STAGE_BYTES = (size_t)STAGE_CAP * 12;  // three coordinate planes
  static size_t count_bytes(int tcap) { return TABLE_OFF + tables_bytes(tcap) + STAGE_BYTES; }
  // FILL: slots = hits + at most one pad slot per query, rounded to 16 so every block's key array stays 16-B aligned
  static int64_t slots(int64_t max_block_hits) { return (max_block_hits + RQ + 15) / 16 * 16; }
  static size_t total(int64_t slots) { return FILL_OFF + (size_t)slots * 9; }  // int tables + keys (8 B) + row ids (1 B)
};

template <int RQ, bool FILL, bool HITS_IN_LDS>
__global__ __launch_bounds__(NSUB* RQ) __attribute__((amdgpu_waves_per_eu(8, 8))) void traverse_kernel(
    const float4* __restrict__ sorted_q, int nq, const int32_t* __restrict__ q_off, int nb,
    const BatchGrid* __restrict__ grids, const int32_t* __restrict__ start_s,
    const float4* __restrict__ sorted_s, float r2, int32_t* __restrict__ q_cnt, int2* __restrict__ q_rng,
    unsigned long long* __restrict__ q_mask, int32_t* __restrict__ blk_stats, int width, int row_stride, int64_t pad_value,
    int64_t* __restrict__ out, int max_block_hits, unsigned long long* __restrict__ g_hits, unsigned char* __restrict__ g_rows, int mono) {
  using L = TravLds<RQ>;
  static_assert(RQ % WAVE == 0 && RQ <= 256, "row ids are bytes; waves must not straddle slabs");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int* offs = reinterpret_cast<int*>(smem);
  int* orig = offs + (RQ + 1);
  int* wsum = orig + RQ;
  int* sub = wsum + L::THREADS / WAVE;  // [NSUB][RQ]
  int* band_lo = sub + NSUB * RQ;
  int* band_hi = band_lo + NBAND;
  int* band_base = band_hi + NBAND;
  // COUNT pass only: per-cloud tables cached in LDS so the per-query setup is not a chain of
  // dependent global round trips (query -> cloud id -> grid -> cell starts)
  const int tcap = FILL ? 0 : (nb <= L::TABLE_MAX ? nb : 0);
  int* s_qoff = reinterpret_cast<int*>(smem + L::TABLE_OFF);
  BatchGrid* s_grids = reinterpret_cast<BatchGrid*>(smem + L::TABLE_OFF + ((size_t)(tcap + 1) * 4 + 15) / 16 * 16);
  float4* stage = reinterpret_cast<float4*>(smem + L::TABLE_OFF + L::tables_bytes(tcap));
  // FILL keeps no candidate stage: its hit segments start right after the int tables
  unsigned long long* hits = HITS_IN_LDS ? reinterpret_cast<unsigned long long*>(smem + L::FILL_OFF)
                                         : g_hits + (int64_t)blockIdx.x * max_block_hits;
  unsigned char* rows = HITS_IN_LDS
                            ? reinterpret_cast<unsigned char*>(smem + L::FILL_OFF + (size_t)max_block_hits * 8)
                            : g_rows + (int64_t)blockIdx.x * max_block_hits;

  const int tid = threadIdx.x;
  const int slot = tid % RQ, j = tid / RQ;  // query slot in block, z-slab
  // XCD-aware block order: the dispatcher places block b on XCD b % 8 (speed only, never
  // correctness).  Give each XCD one CONTIGUOUS eighth of the cell-ordered queries so the candidate
  // bands of neighbouring blocks (which overlap ~9x) are served by that XCD's own 4 MiB L2 instead
  // of being re-fetched from Infinity Cache by all eight.
  const int nblk = (nq + RQ - 1) / RQ;
  const int per_xcd = gridDim.x / 8;  // the grid is padded to a multiple of 8 blocks
  const int blk = (blockIdx.x % 8) * per_xcd + blockIdx.x / 8;
  if (blk >= nblk) return;
  const int t = blk * RQ + slot;
  const int lane = tid & (WAVE - 1);
  const bool valid = t < nq;

  if (tid < NBAND) {
    band_lo[tid] = 0x7fffffff;
    band_hi[tid] = 0;
  }
  const bool tables_in_lds = tcap > 0;
  if (tables_in_lds) {
    for (int i = tid; i <= nb; i += L::THREADS) s_qoff[i] = q_off[i];
    const int4* gsrc = reinterpret_cast<const int4*>(grids);
    int4* gdst = reinterpret_cast<int4*>(s_grids);
    for (int i = tid; i < nb * 4; i += L::THREADS) gdst[i] = gsrc[i];
  }
  int my_off = 0;
  float4 qp = make_float4(0.f, 0.f, 0.f, 0.f);
  int p0[3] = {0, 0, 0}, p1[3] = {0, 0, 0};
  unsigned long long fill_bits = 0ull;
  if (FILL) {
    // every slab group redundantly scans the per-query totals (two waves each; no cross-group sync)
    int c[NSUB] = {0, 0, 0};
    if (valid) {
#pragma unroll
      for (int i = 0; i < NSUB; ++i) c[i] = q_cnt[(int64_t)i * nq + t];
      // everything else this thread needs from the COUNT pass is requested NOW, so the block pays one global
      // round trip for (counts, query, ranges, hit mask) instead of two separated by the barrier below
      qp = sorted_q[t];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const int2 r = q_rng[(int64_t)(i * NSUB + j) * nq + t];
        p0[i] = r.x;
        p1[i] = r.y;
      }
      fill_bits = q_mask[(int64_t)j * nq + t];
    }
    const int tot = c[0] + c[1] + c[2];
    const int tot2 = (tot + 1) & ~1;  // segments start on even slots: the rank loop reads two keys per ds_read_b128
    const int inc = wave_incl_scan_add_dpp(tot2);
    if (lane == WAVE - 1) wsum[tid / WAVE] = inc;
    __syncthreads();
    int base = 0;
#pragma unroll
    for (int i = 0; i < RQ / WAVE; ++i)
      if (i < slot / WAVE) base += wsum[j * (RQ / WAVE) + i];
    const int q_start = base + inc - tot2;
    my_off = q_start + (j > 0 ? c[0] : 0) + (j > 1 ? c[1] : 0);
    if (j == 0) {
      offs[slot] = q_start;
      if (slot == RQ - 1) offs[RQ] = q_start + tot2;
      if (tot2 != tot) {  // pad slot: larger than every real key, skipped by the rank phase
        hits[q_start + tot] = ~0ull;
        rows[q_start + tot] = 0xff;
      }
    }
  } else {
    __syncthreads();
  }

  // ---- per-thread candidate ranges (global positions in sorted_s) for bands (dy, dz = j-1):
  //      computed by the COUNT pass and stored; the FILL pass just reloads them (one coalesced trip)
  if (valid) {
    if (FILL) {
      if (j == 0) orig[slot] = __float_as_int(qp.w);
    } else {
      qp = sorted_q[t];
      int b;
      BatchGrid g;
      if (tables_in_lds) {
        b = find_batch(s_qoff, nb, __float_as_int(qp.w));
        g = s_grids[b];
      } else {
        b = find_batch(q_off, nb, __float_as_int(qp.w));
        g = grids[b];
      }
      const double ux = cell_coord(qp.x, g.org[0], g.inv_cell_x), kx = (double)g.xk;
      const double uy = cell_coord(qp.y, g.org[1], g.inv_cell);
      const double cz = cell_coord(qp.z, g.org[2], g.inv_cell) + (double)(j - 1);
      const double tx = (double)(g.dim[0] - 1), ty = (double)(g.dim[1] - 1), tz = (double)(g.dim[2] - 1);
      // the comparisons are written so that NaN coordinates give "no candidates"
      if ((ux + kx >= 0.0) && (ux - kx <= tx) && cz >= 0.0 && cz <= tz) {
        const int lx = (int)fmin(fmax(ux - kx, 0.0), tx);
        const int hx = (int)fmin(fmax(ux + kx, 0.0), tx);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const double cy = uy + (double)(i - 1);
          if (cy >= 0.0 && cy <= ty) {
            const int base = g.cell_base + g.dim[0] * ((int)cy + g.dim[1] * (int)cz);
            p0[i] = start_s[base + lx];
            p1[i] = start_s[base + hx + 1];
          }
        }
      }
#pragma unroll
      for (int i = 0; i < 3; ++i) q_rng[(int64_t)(i * NSUB + j) * nq + t] = make_int2(p0[i], p1[i]);
    }
  } else if (FILL && j == 0) {
    orig[slot] = -1;
  }
  int n = 0;
  if (!FILL) {
    // ---- block-wide extent of every band (waves are slab-uniform: band index = 3*j + i)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const bool has = p1[i] > p0[i];
      int lo, hi;
      if (mono) {
        // self-search: queries are in cell order and every range comes from the query's own cell, so p0 and p1 are
        // non-decreasing along the wave -- the extent is (first valid lane's p0, last valid lane's p1)
        const unsigned long long m = __ballot(has);
        lo = 0x7fffffff;
        hi = 0;
        if (m) {
          lo = __builtin_amdgcn_readlane(p0[i], __builtin_amdgcn_readfirstlane(__ffsll((long long)m) - 1));
          hi = __builtin_amdgcn_readlane(p1[i], __builtin_amdgcn_readfirstlane(63 - __clzll((long long)m)));
        }
      } else {
        lo = wave_min_i32_dpp(has ? p0[i] : 0x7fffffff);
        hi = wave_max_i32_dpp(has ? p1[i] : 0);
      }
      if (lane == 0 && hi > 0) {
        atomicMin(&band_lo[3 * j + i], lo);
        atomicMax(&band_hi[3 * j + i], hi);
      }
    }
    __syncthreads();
    if (tid == 0) {
      int acc = 0;
      for (int k = 0; k < NBAND; ++k) {
        band_base[k] = acc;
        acc += band_hi[k] > band_lo[k] ? band_hi[k] - band_lo[k] : 0;
      }
      band_base[NBAND] = acc;
    }
    __syncthreads();
    const bool staged = band_base[NBAND] <= L::STAGE_CAP;
    // candidates are staged as three coordinate planes (the index is not needed to COUNT), so a thread can
    // pull two neighbours per plane into one 64-bit register pair and test them with packed fp32 math
    float* sx = reinterpret_cast<float*>(stage);
    float* sy = sx + L::STAGE_CAP;
    float* sz = sy + L::STAGE_CAP;
    if (staged) {
      // one flat pass over the union of the nine bands: every thread issues ALL its loads (<= 4) before the
      // first LDS write, so the block pays one global round trip here instead of one per band
      const int total = band_base[NBAND];
      int bl[NBAND], bs[NBAND];
#pragma unroll
      for (int k = 0; k < NBAND; ++k) {
        bl[k] = band_lo[k];
        bs[k] = band_base[k];
      }
      constexpr int PER = L::STAGE_CAP / L::THREADS;
      float4 v[PER];
      // unconditional loads on a clamped index (pad_value = number of supports): behind `if (f < total)` the compiler
      // keeps every load behind the previous one's use -- four memory round trips instead of one
#pragma unroll
      for (int u = 0; u < PER; ++u) {
        const int f = tid + u * L::THREADS;
        unsigned src = (unsigned)bl[0] + (unsigned)f;
#pragma unroll
        for (int k = 1; k < NBAND; ++k) src = f >= bs[k] ? (unsigned)bl[k] + (unsigned)(f - bs[k]) : src;
        src = f < total ? src : 0u;
        v[u] = sorted_s[min(src, (unsigned)((int)pad_value - 1))];
      }
#pragma unroll
      for (int u = 0; u < PER; ++u) {
        const int f = tid + u * L::THREADS;
        if (f < total) {
          sx[f] = v[u].x;
          sy[f] = v[u].y;
          sz[f] = v[u].z;
        }
      }
      __syncthreads();
    }
    // ---- walk every candidate; remember the hits as a bit mask (bit = position in this thread's
    //      enumeration order) so the FILL pass only ever touches the ~16 % that matter
    unsigned long long mask = 0ull;
    int bitpos = 0;
    if (valid && staged) {
      const f32x2 qx = {qp.x, qp.x}, qy = {qp.y, qp.y}, qz = {qp.z, qp.z};
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const int rel = band_base[3 * j + i] - band_lo[3 * j + i];
        int p = p0[i] + rel;
        const int e = p1[i] + rel;
        for (; p + 4 <= e; p += 4) {
          const f32x2 xa = {sx[p], sx[p + 1]}, xb = {sx[p + 2], sx[p + 3]};
          const f32x2 ya = {sy[p], sy[p + 1]}, yb = {sy[p + 2], sy[p + 3]};
          const f32x2 za = {sz[p], sz[p + 1]}, zb = {sz[p + 2], sz[p + 3]};
          // nanoflann.hpp:432-440: result += diff*diff for x, y, z starting from 0 (two lanes per op)
          const f32x2 dxa = qx - xa, dya = qy - ya, dza = qz - za;
          const f32x2 dxb = qx - xb, dyb = qy - yb, dzb = qz - zb;
          const f32x2 da = (dxa * dxa + dya * dya) + dza * dza;
          const f32x2 db = (dxb * dxb + dyb * dyb) + dzb * dzb;
          const unsigned hb = (da.x < r2 ? 1u : 0u) | (da.y < r2 ? 2u : 0u) | (db.x < r2 ? 4u : 0u) | (db.y < r2 ? 8u : 0u);
          if (bitpos < 64) mask |= (unsigned long long)hb << bitpos;
          n += __popc(hb);
          bitpos += 4;
        }
        for (; p < e; ++p) {
          const float dx = qp.x - sx[p], dy = qp.y - sy[p], dz = qp.z - sz[p];
          const float d = (dx * dx + dy * dy) + dz * dz;
          const bool hit = d < r2;
          if (hit && bitpos < 64) mask |= 1ull << bitpos;
          n += hit ? 1 : 0;
          ++bitpos;
        }
      }
    } else if (valid) {
#pragma unroll
      for (int i = 0; i < 3; ++i)
        for (int p = p0[i]; p < p1[i]; ++p) {
          const float4 sp = sorted_s[p];
          const float dx = qp.x - sp.x, dy = qp.y - sp.y, dz = qp.z - sp.z;
          const float d = (dx * dx + dy * dy) + dz * dz;
          const bool hit = d < r2;
          if (hit && bitpos < 64) mask |= 1ull << bitpos;
          n += hit ? 1 : 0;
          ++bitpos;
        }
    }
    if (valid) q_mask[(int64_t)j * nq + t] = mask;
  } else if (valid) {
    // ---- FILL: gather only the hits (bit mask from the COUNT pass), eight loads in flight;
    //      threads with more than 64 candidates re-walk everything
    const int len0 = p1[0] - p0[0], len1 = p1[1] - p0[1], len2 = p1[2] - p0[2];
    auto emit = [&](const float4 sp) {
      const float dx = qp.x - sp.x;
      const float dy = qp.y - sp.y;
      const float dz = qp.z - sp.z;
      const float d = (dx * dx + dy * dy) + dz * dz;
      if (d < r2) {
        // key orders by (distance, index); d >= 0 so its bit pattern is monotone
        hits[my_off + n] = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned int)__float_as_int(sp.w);
        rows[my_off + n] = (unsigned char)slot;
        ++n;
      }
    };
    if (len0 + len1 + len2 <= 64) {
      unsigned long long bits = fill_bits;
      while (bits) {
        int pos[GB];
#pragma unroll
        for (int u = 0; u < GB; ++u) {
          pos[u] = -1;
          if (bits) {
            const int bpos = __ffsll((long long)bits) - 1;
            bits &= bits - 1;
            // enumeration order: band 0, then band 1, then band 2
            pos[u] = bpos < len0 ? p0[0] + bpos : (bpos < len0 + len1 ? p0[1] + (bpos - len0) : p0[2] + (bpos - len0 - len1));
          }
        }
        // unconditional loads (a spent slot re-reads support 0): behind a branch the compiler waits for every load before
        // it issues the next one, and the point of this loop is GB random reads in flight
        float4 sp[GB];
#pragma unroll
        for (int u = 0; u < GB; ++u) sp[u] = sorted_s[max(pos[u], 0)];
#pragma unroll
        for (int u = 0; u < GB; ++u)
          if (pos[u] >= 0) emit(sp[u]);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 3; ++i)
        for (int p = p0[i]; p < p1[i]; ++p) emit(sorted_s[p]);
    }
  }

  if (!FILL) {
    if (valid) q_cnt[(int64_t)j * nq + t] = n;
    sub[tid] = n;
    __syncthreads();
    if (tid < RQ) {
      const int tot = sub[tid] + sub[RQ + tid] + sub[2 * RQ + tid];
      const int mx = wave_max_i32_dpp(tot), sm = wave_sum_i32_dpp(tot);
      if (lane == 0) {
        wsum[tid / WAVE] = mx;
        wsum[RQ / WAVE + tid / WAVE] = sm;
      }
    }
    __syncthreads();
    if (tid == 0) {
      int mx = 0, sm = 0;
#pragma unroll
      for (int i = 0; i < RQ / WAVE; ++i) {
        mx = max(mx, wsum[i]);
        sm += wsum[RQ / WAVE + i];
      }
      blk_stats[2 * blk] = mx;      // reduced by reduce_stats_kernel: no same-address
      blk_stats[2 * blk + 1] = sm;  // global atomics (they cost ~11 ns EACH when contended)
    }
    return;
  }

  __syncthreads();
  // ---- phase B: one thread per hit, rank inside its segment, store to the final slot
  const int total_hits = offs[RQ];
  for (int e = tid; e < total_hits; e += L::THREADS) {
    const int r = rows[e];
    if (r == 0xff) continue;  // pad slot
    const int a = offs[r], len = offs[r + 1] - a;  // both even
    const unsigned long long key = hits[e];
    const ulonglong2* seg = reinterpret_cast<const ulonglong2*>(hits + a);
    int rank = 0;
    int jj = 0;
    for (; jj + 4 <= len / 2; jj += 4) {  // eight keys per step, four independent ds_read_b128 in flight
      ulonglong2 hk[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) hk[u] = seg[jj + u];
#pragma unroll
      for (int u = 0; u < 4; ++u) rank += (hk[u].x < key ? 1 : 0) + (hk[u].y < key ? 1 : 0);
    }
    for (; jj < len / 2; ++jj) {
      const ulonglong2 h = seg[jj];
      rank += (h.x < key ? 1 : 0) + (h.y < key ? 1 : 0);
    }
    if (rank < width) out[(int64_t)orig[r] * row_stride + rank] = (int64_t)(unsigned int)(key & 0xffffffffull);
  }
  // ---- padding: one row per wave iteration, lanes along the row
  const int rows_here = min(RQ, nq - blk * RQ);
  for (int r = tid / 32; r < rows_here; r += L::THREADS / 32) {  // half a wave per row
    int cnt = offs[r + 1] - offs[r];
    if (cnt > 0 && rows[offs[r + 1] - 1] == 0xff) --cnt;  // the segment ends in a pad slot
    int64_t* row = out + (int64_t)orig[r] * row_stride;
    for (int c = min(cnt, width) + (lane & 31); c < row_stride; c += 32) row[c] = pad_value;
  }
}
