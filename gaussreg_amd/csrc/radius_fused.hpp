// Radius search, fused (gr_radius_search mode 1); included after radius_traverse.hpp, whose NBAND / NSUB / f32x2 it shares.
#pragma once
// ---------------------------------------------------------------- single pass for a width known before the launch
// radius_search(..., neighbor_limit) (modules/ops/radius_search.py:7-27) keeps min(max_count, neighbor_limit) columns, so the
// caller can allocate (nq, limit) rows BEFORE anything is counted and one kernel does the whole search:
//   set-up, staging  as in the COUNT pass above
//   tests            hits are remembered in two 32-bit masks per thread (even / odd candidates of its enumeration)
//   scan             hit counts -> per-query segments in the block's key area (LDS)
//   decode           every thread walks its masks, one even and one odd hit per step, and leaves (query slot, staged
//                    position) words in its part of the segment -- no arithmetic in the loop whose trip count diverges
//   keys             one thread per hit (balanced): distance bits and support index from the staged planes
//   ranking          one thread per hit: rank = number of smaller distance words in the segment (32-bit compares, four keys
//                    per ds_read_b128).  The index goes to row[rank] in an LDS row buffer with ds_min: equal distances
//                    collide there, leave a hole behind them, and only such rows are ranked again on (distance, index)
//   rows             whole rows leave as contiguous 16-byte pieces
// Nothing per query goes through global memory in between (the two-pass path writes and re-reads 180 bytes of ranges /
// masks / counts per query) and the host does not sit between two launches.
//   blk_stats[2 blk]     = largest hit count of a query in the block   (max -> the width the reference would return)
//   blk_stats[2 blk + 1] = 1 if a single query had more hits than the block's key area holds (the caller then repeats
//                          the search on the two-pass path)
// A block whose hits do not fit its key area at once works through its queries in groups (direct stores, exact compare).
template <int RQ>
struct FusedLds {
  static constexpr int THREADS = NSUB * RQ;
  static constexpr int STAGE_CAP = 12 * RQ;
  static constexpr int TABLE_MAX = 256;
  // ints: offs[RQ+1], orig[RQ], qtot[RQ], wsum[2 * THREADS/64], sub[3*RQ], band_lo[9], band_hi[9], band_base[10], misc[4],
  //       tie flags[RQ]
  static constexpr int N_INTS = (RQ + 1) + RQ + RQ + 2 * (THREADS / WAVE) + NSUB * RQ + 9 + 9 + 10 + 4 + RQ;
  static constexpr size_t QBUF_OFF = (size_t)(N_INTS * 4 + 15) / 16 * 16;  // float4 per query slot
  static constexpr size_t STAGE_OFF = QBUF_OFF + (size_t)RQ * 16;
  static size_t region_bytes(int width) {  // candidate planes x, y, z, index (+ slack for the 4-wide tail reads); the row
    const size_t st = (size_t)STAGE_CAP * 16 + 16, rb = ((size_t)RQ * width * 4 + 15) / 16 * 16;  // buffer takes their place
    return st > rb ? st : rb;
  }
  static size_t tables_bytes(int tcap) { return tcap > 0 ? ((size_t)(tcap + 1) * 4 + 15) / 16 * 16 + (size_t)tcap * sizeof(BatchGrid) : 0; }
  static size_t hits_bytes(int cap) { return (size_t)(cap + 16) * 9; }  // distance words, (slot, position) / index words, row bytes
  static size_t total(int width, int cap, int tcap) {
    const size_t hits = hits_bytes(cap), tb = tables_bytes(tcap);
    return STAGE_OFF + region_bytes(width) + (hits > tb ? hits : tb);
  }
};

template <int RQ>
__global__ __launch_bounds__(NSUB* RQ) void fused_kernel(
    const float4* __restrict__ sorted_q, int nq, const int32_t* __restrict__ q_off, int nb,
    const BatchGrid* __restrict__ grids, const int32_t* __restrict__ start_s, const float4* __restrict__ sorted_s, int ns_total,
    float r2, int32_t* __restrict__ blk_stats, int width, int64_t pad_value, int64_t* __restrict__ out, int cap,
    int region_bytes, int mono) {
  using L = FusedLds<RQ>;
  static_assert(RQ % WAVE == 0 && RQ <= 256, "row ids are bytes; waves must not straddle slabs");
  constexpr unsigned PADMARK = 0xffffffffu;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int* offs = reinterpret_cast<int*>(smem);
  int* orig = offs + (RQ + 1);
  int* qtot = orig + RQ;
  int* wsum = qtot + RQ;
  int* sub = wsum + 2 * (L::THREADS / WAVE);  // [NSUB][RQ]
  int* band_lo = sub + NSUB * RQ;
  int* band_hi = band_lo + NBAND;
  int* band_base = band_hi + NBAND;
  int* misc = band_base + NBAND + 1;  // [0] group search, [1] number of rows with equal distances
  int* tie_rows = misc + 4;
  float4* qbuf = reinterpret_cast<float4*>(smem + L::QBUF_OFF);
  float* sx = reinterpret_cast<float*>(smem + L::STAGE_OFF);
  float* sy = sx + L::STAGE_CAP;
  float* sz = sy + L::STAGE_CAP;
  int* si = reinterpret_cast<int*>(sz + L::STAGE_CAP);
  unsigned int* rowbuf = reinterpret_cast<unsigned int*>(smem + L::STAGE_OFF);  // takes the planes' place after the keys pass
  char* hreg = smem + L::STAGE_OFF + region_bytes;
  unsigned int* hd = reinterpret_cast<unsigned int*>(hreg);      // distance bits per hit slot
  unsigned int* hm = hd + (cap + 16);                            // (slot << 16 | staged position), then the support index
  unsigned char* hrow = reinterpret_cast<unsigned char*>(hm + (cap + 16));
  const int dummy = cap + 8;  // a slot nobody reads: the target of the decode's "no hit" lanes
  // per-cloud tables for the set-up live where the keys go later
  const int tcap = nb <= L::TABLE_MAX ? nb : 0;
  int* s_qoff = reinterpret_cast<int*>(hreg);
  BatchGrid* s_grids = reinterpret_cast<BatchGrid*>(hreg + ((size_t)(tcap + 1) * 4 + 15) / 16 * 16);

  const int tid = threadIdx.x;
  const int slot = tid % RQ, j = tid / RQ;
  const int nblk = (nq + RQ - 1) / RQ;
  const int per_xcd = gridDim.x / 8;
  const int blk = (blockIdx.x % 8) * per_xcd + blockIdx.x / 8;  // one contiguous eighth of the cell-ordered queries per XCD
  if (blk >= nblk) return;
  const int t = blk * RQ + slot;
  const int lane = tid & (WAVE - 1);
  const bool valid = t < nq;

  if (tid < NBAND) {
    band_lo[tid] = 0x7fffffff;
    band_hi[tid] = 0;
  }
  if (tid == 0) misc[1] = 0;
  if (tid < RQ) tie_rows[tid] = 0;
  const bool tables_in_lds = tcap > 0;
  if (tables_in_lds) {
    for (int i = tid; i <= nb; i += L::THREADS) s_qoff[i] = q_off[i];
    const int4* gsrc = reinterpret_cast<const int4*>(grids);
    int4* gdst = reinterpret_cast<int4*>(s_grids);
    for (int i = tid; i < nb * 4; i += L::THREADS) gdst[i] = gsrc[i];
  }
  float4 qp = make_float4(0.f, 0.f, 0.f, 0.f);
  if (valid) qp = sorted_q[t];
  __syncthreads();
  int p0[3] = {0, 0, 0}, p1[3] = {0, 0, 0};
  if (valid) {
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
    if ((ux + kx >= 0.0) && (ux - kx <= tx) && cz >= 0.0 && cz <= tz) {  // NaN coordinates: no candidates
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
    if (j == 0) {
      orig[slot] = __float_as_int(qp.w);
      qbuf[slot] = qp;
    }
  } else if (j == 0) {
    orig[slot] = -1;
  }
  // ---- block-wide extent of every band (waves are slab-uniform: band index = 3*j + i)
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const bool has = p1[i] > p0[i];
    int lo, hi;
    if (mono) {
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
  if (staged) {
    // wave w copies bands w, w + NWV, ...; lanes run over the band's elements.  (A flat pass over the union of the bands had
    // every element find its band with eight compare / select pairs: ~130 instructions per thread for four elements.)  All
    // loads of a wave are issued before its first LDS write, on clamped indices (no load sits behind a branch).
    constexpr int NWV = L::THREADS / WAVE, KMAX = (NBAND + NWV - 1) / NWV, UNR = 2;
    const int wvi = tid / WAVE;
    float4 v[KMAX][UNR];
    int blo[KMAX], blen[KMAX], bdst[KMAX];
#pragma unroll
    for (int kk = 0; kk < KMAX; ++kk) {
      const int k = wvi + kk * NWV;
      blo[kk] = 0;
      blen[kk] = 0;
      bdst[kk] = 0;
      if (k < NBAND) {
        const int l0 = band_lo[k], h0 = band_hi[k];
        blen[kk] = h0 > l0 ? h0 - l0 : 0;
        blo[kk] = blen[kk] > 0 ? l0 : 0;
        bdst[kk] = band_base[k];
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u)
        v[kk][u] = sorted_s[min(blo[kk] + u * WAVE + lane, ns_total - 1)];
    }
#pragma unroll
    for (int kk = 0; kk < KMAX; ++kk) {
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const int f = u * WAVE + lane;
        if (f < blen[kk]) {
          sx[bdst[kk] + f] = v[kk][u].x;
          sy[bdst[kk] + f] = v[kk][u].y;
          sz[bdst[kk] + f] = v[kk][u].z;
          si[bdst[kk] + f] = __float_as_int(v[kk][u].w);
        }
      }
      for (int f = UNR * WAVE + lane; f < blen[kk]; f += WAVE) {  // a band longer than 128 elements
        const float4 t4 = sorted_s[blo[kk] + f];
        sx[bdst[kk] + f] = t4.x;
        sy[bdst[kk] + f] = t4.y;
        sz[bdst[kk] + f] = t4.z;
        si[bdst[kk] + f] = __float_as_int(t4.w);
      }
    }
    __syncthreads();
  }
  // ---- test every candidate, four per step.  Enumeration slot c = 4 * step + k (k = 0..3; a band's last step is padded);
  //      even slots are remembered in `lo`, odd slots in `hi`: two 32-bit SHIFT REGISTERS -- a hit is the sign bit of
  //      (distance bits - r2 bits) (both are non-negative floats: their bit patterns order like the values, NaN sorts above
  //      everything), shifted in with one v_alignbit; the decode below takes one hit from each side per step
  unsigned lo = 0u, hi = 0u;
  int n = 0;
  int rel[3] = {0, 0, 0};
  if (staged) {
#pragma unroll
    for (int i = 0; i < 3; ++i) rel[i] = band_base[3 * j + i] - band_lo[3 * j + i];
  }
  const int len0 = p1[0] - p0[0], len1 = p1[1] - p0[1], len2 = p1[2] - p0[2];
  const int nit0 = (len0 + 3) >> 2, nit1 = (len1 + 3) >> 2, nit2 = (len2 + 3) >> 2;
  const bool by_mask = staged && (nit0 + nit1 + nit2 <= 16);  // else: counted here, re-walked in the decode
  const unsigned r2b = r2 == r2 ? __float_as_uint(r2) : 0u;      // NaN radius: nothing is a neighbour
  if (valid && by_mask) {
    const f32x2 qx = {qp.x, qp.x}, qy = {qp.y, qp.y}, qz = {qp.z, qp.z};
    auto step4 = [&](int p) {
      const f32x2 xa = {sx[p], sx[p + 1]}, xb = {sx[p + 2], sx[p + 3]};
      const f32x2 ya = {sy[p], sy[p + 1]}, yb = {sy[p + 2], sy[p + 3]};
      const f32x2 za = {sz[p], sz[p + 1]}, zb = {sz[p + 2], sz[p + 3]};
      // nanoflann.hpp:432-440: result += diff*diff for x, y, z starting from 0 (two candidates per op)
      const f32x2 dxa = qx - xa, dya = qy - ya, dza = qz - za;
      const f32x2 dxb = qx - xb, dyb = qy - yb, dzb = qz - zb;
      const f32x2 da = (dxa * dxa + dya * dya) + dza * dza;
      const f32x2 db = (dxb * dxb + dyb * dyb) + dzb * dzb;
      const unsigned t0 = __float_as_uint(da.x) - r2b, t1 = __float_as_uint(da.y) - r2b;
      const unsigned t2 = __float_as_uint(db.x) - r2b, t3 = __float_as_uint(db.y) - r2b;
      lo = __builtin_amdgcn_alignbit(lo, t0, 31);  // (lo << 1) | sign(t0)
      lo = __builtin_amdgcn_alignbit(lo, t2, 31);
      hi = __builtin_amdgcn_alignbit(hi, t1, 31);
      hi = __builtin_amdgcn_alignbit(hi, t3, 31);
    };
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      int p = p0[i] + rel[i];
      const int e = p1[i] + rel[i];
      for (; p + 4 <= e; p += 4) step4(p);
      if (p < e) {  // padded last step: 1..3 candidates left (the reads past the band stay inside the planes)
        const int left = e - p;
        // (same arithmetic; slots past the band shift in a zero)
        {
          const f32x2 xa = {sx[p], sx[p + 1]}, xb = {sx[p + 2], sx[p + 3]};
          const f32x2 ya = {sy[p], sy[p + 1]}, yb = {sy[p + 2], sy[p + 3]};
          const f32x2 za = {sz[p], sz[p + 1]}, zb = {sz[p + 2], sz[p + 3]};
          const f32x2 dxa = qx - xa, dya = qy - ya, dza = qz - za;
          const f32x2 dxb = qx - xb, dyb = qy - yb, dzb = qz - zb;
          const f32x2 da = (dxa * dxa + dya * dya) + dza * dza;
          const f32x2 db = (dxb * dxb + dyb * dyb) + dzb * dzb;
          const unsigned t0 = __float_as_uint(da.x) - r2b;
          const unsigned t1 = left >= 2 ? __float_as_uint(da.y) - r2b : 0u;
          const unsigned t2 = left >= 3 ? __float_as_uint(db.x) - r2b : 0u;
          lo = __builtin_amdgcn_alignbit(lo, t0, 31);
          lo = __builtin_amdgcn_alignbit(lo, t2, 31);
          hi = __builtin_amdgcn_alignbit(hi, t1, 31);
          hi = __builtin_amdgcn_alignbit(hi, 0u, 31);
        }
      }
    }
    n = __popc(lo) + __popc(hi);
  } else if (valid && staged) {  // more than 64 enumeration slots: count now, walk again in the decode
#pragma unroll
    for (int i = 0; i < 3; ++i)
      for (int p = p0[i] + rel[i]; p < p1[i] + rel[i]; ++p) {
        const float dx = qp.x - sx[p], dy = qp.y - sy[p], dz = qp.z - sz[p];
        const float d = (dx * dx + dy * dy) + dz * dz;
        n += d < r2 ? 1 : 0;
      }
  } else if (valid) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
      for (int p = p0[i]; p < p1[i]; ++p) {
        const float4 sp = sorted_s[p];
        const float dx = qp.x - sp.x, dy = qp.y - sp.y, dz = qp.z - sp.z;
        const float d = (dx * dx + dy * dy) + dz * dz;
        n += d < r2 ? 1 : 0;
      }
  }
  sub[tid] = n;
  __syncthreads();
  // ---- block scan of the per-query totals; every slab group does it redundantly (no cross-group sync)
  int c[NSUB];
#pragma unroll
  for (int i = 0; i < NSUB; ++i) c[i] = sub[i * RQ + slot];
  const int tot = c[0] + c[1] + c[2];
  const int tot4 = (tot + 3) & ~3;  // segments start on multiples of four slots: the rank loop reads four keys per ds_read_b128
  const int inc = wave_incl_scan_add_dpp(tot4);
  const int wmx = wave_max_i32_dpp(tot);
  if (lane == WAVE - 1) wsum[tid / WAVE] = inc;
  if (lane == 0) wsum[L::THREADS / WAVE + tid / WAVE] = wmx;
  __syncthreads();
  int base = 0, total4 = 0;
#pragma unroll
  for (int i = 0; i < RQ / WAVE; ++i) {
    const int w = wsum[j * (RQ / WAVE) + i];
    if (i < slot / WAVE) base += w;
    total4 += w;
  }
  const int q_start = base + inc - tot4;
  const int my_off = q_start + (j > 0 ? c[0] : 0) + (j > 1 ? c[1] : 0);
  if (j == 0) {
    offs[slot] = q_start;
    qtot[slot] = tot;
    if (slot == RQ - 1) offs[RQ] = q_start + tot4;
  }
  int blk_flag = 0;
  const bool multi = total4 > cap;
  const bool use_rowbuf = !multi;  // rows leave through an LDS row buffer as contiguous 16-byte pieces
  const int rows_here = min(RQ, nq - blk * RQ);
  if (multi) __syncthreads();  // offs complete
  int glo = 0;
  while (glo < RQ) {
    int ghi = RQ;
    bool skip = false;
    if (multi) {
      if (tid == 0) misc[0] = RQ;
      __syncthreads();
      if (tid >= glo && tid < RQ && offs[tid + 1] - offs[glo] > cap) atomicMin(&misc[0], tid);
      __syncthreads();
      ghi = misc[0];
      if (ghi == glo) {  // one query alone overflows the key area: the caller repeats the call on the two-pass path
        blk_flag = 1;
        skip = true;
        ghi = glo + 1;
      }
    }
    const int gbase = multi ? offs[glo] : 0;
    const bool mine = valid && !skip && slot >= glo && slot < ghi;
    // ---- decode: (query slot, staged position) words of my hits into my part of my query's segment
    if (mine && j == NSUB - 1)
      for (int k = tot; k < tot4; ++k) hm[q_start - gbase + k] = PADMARK;
    if (mine && n > 0) {
      int w = my_off - gbase;
      const unsigned tag = (unsigned)slot << 16;
      if (by_mask) {
        const int c1 = 4 * nit0, c2 = 4 * (nit0 + nit1);
        const int s0 = p0[0] + rel[0], s1 = p0[1] + rel[1] - c1, s2 = p0[2] + rel[2] - c2;
        // the shift registers hold 2 bits per step: the side's first candidate sits in bit 2 S - 1 (S = steps of this thread)
        const int top = 2 * (nit0 + nit1 + nit2) - 1;
        unsigned ml = lo, mh = hi;
        while (ml | mh) {
          const int qa = 31 - __clz((int)ml), qb = 31 - __clz((int)mh);  // -1: none left on that side
          ml &= ~(qa >= 0 ? 1u << qa : 0u);
          mh &= ~(qb >= 0 ? 1u << qb : 0u);
          const int ca = 2 * (top - qa), cb = 2 * (top - qb) + 1;      // enumeration slots
          const int pa = ca + (ca < c1 ? s0 : (ca < c2 ? s1 : s2));
          const int pb = cb + (cb < c1 ? s0 : (cb < c2 ? s1 : s2));
          const int wa = qa >= 0 ? w : dummy;
          w += qa >= 0 ? 1 : 0;
          const int wb = qb >= 0 ? w : dummy;
          w += qb >= 0 ? 1 : 0;
          hm[wa] = tag | (unsigned)pa;
          hm[wb] = tag | (unsigned)pb;
        }
      } else if (staged) {
#pragma unroll
        for (int i = 0; i < 3; ++i)
          for (int p = p0[i] + rel[i]; p < p1[i] + rel[i]; ++p) {
            const float dx = qp.x - sx[p], dy = qp.y - sy[p], dz = qp.z - sz[p];
            const float d = (dx * dx + dy * dy) + dz * dz;
            if (d < r2) hm[w++] = tag | (unsigned)p;
          }
      } else {
#pragma unroll
        for (int i = 0; i < 3; ++i)
          for (int p = p0[i]; p < p1[i]; ++p) {
            const float4 sp = sorted_s[p];
            const float dx = qp.x - sp.x, dy = qp.y - sp.y, dz = qp.z - sp.z;
            const float d = (dx * dx + dy * dy) + dz * dz;
            if (d < r2) {
              hm[w] = (unsigned)p;  // position in the cell-ordered support array
              hrow[w] = (unsigned char)slot;
              ++w;
            }
          }
      }
    }
    __syncthreads();
    // ---- keys: one thread per hit slot -- distance bits and support index (balanced: no lane waits for a longer list)
    const int group_hits = skip ? 0 : offs[ghi] - gbase;
    for (int e = tid; e < group_hits; e += L::THREADS) {
      const unsigned m = hm[e];
      if (m == PADMARK) {  // larger than every real key; skipped by the ranking
        hd[e] = 0xffffffffu;
        hrow[e] = 0xff;
        continue;
      }
      float x, y, z;
      int idx, r;
      if (staged) {
        const int pp = (int)(m & 0xffffu);
        r = (int)(m >> 16);
        x = sx[pp];
        y = sy[pp];
        z = sz[pp];
        idx = si[pp];
        hrow[e] = (unsigned char)r;
      } else {
        const float4 sp = sorted_s[m];
        r = hrow[e];
        x = sp.x;
        y = sp.y;
        z = sp.z;
        idx = __float_as_int(sp.w);
      }
      const float4 qq = qbuf[r];
      const float dx = qq.x - x, dy = qq.y - y, dz = qq.z - z;
      const float d = (dx * dx + dy * dy) + dz * dz;
      hd[e] = __float_as_uint(d);  // d >= 0: the bit pattern is monotone
      hm[e] = (unsigned)idx;
    }
    __syncthreads();
    if (use_rowbuf) {
      // the planes are dead: their place becomes the row buffer, every entry "not written"
      const int quads = (rows_here * width + 3) >> 2;
      for (int i = tid; i < quads; i += L::THREADS) reinterpret_cast<uint4*>(rowbuf)[i] = make_uint4(PADMARK, PADMARK, PADMARK, PADMARK);
      __syncthreads();
    }
    // ---- ranking: one thread per hit
    for (int e = tid; e < group_hits; e += L::THREADS) {
      const int r = hrow[e];
      if (r == 0xff) continue;
      const int a = offs[r] - gbase, quads = (offs[r + 1] - offs[r]) >> 2;
      const unsigned d = hd[e];
      const unsigned idx = hm[e];
      const uint4* seg = reinterpret_cast<const uint4*>(hd + a);
      int rank = 0;
      if (use_rowbuf) {
        int jj = 0;
        for (; jj + 4 <= quads; jj += 4) {
          uint4 k4[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) k4[u] = seg[jj + u];
#pragma unroll
          for (int u = 0; u < 4; ++u)
            rank += (k4[u].x < d ? 1 : 0) + (k4[u].y < d ? 1 : 0) + (k4[u].z < d ? 1 : 0) + (k4[u].w < d ? 1 : 0);
        }
        for (; jj < quads; ++jj) {
          const uint4 k = seg[jj];
          rank += (k.x < d ? 1 : 0) + (k.y < d ? 1 : 0) + (k.z < d ? 1 : 0) + (k.w < d ? 1 : 0);
        }
        // equal distances meet in one entry (the smallest index stays) and leave the next one unwritten
        if (rank < width) atomicMin(&rowbuf[r * width + rank], idx);
      } else {
        // direct stores: exact (distance, index) order in one go
        const uint4* segi = reinterpret_cast<const uint4*>(hm + a);
        for (int jj = 0; jj < quads; ++jj) {
          const uint4 k = seg[jj], ki = segi[jj];
          rank += (k.x < d || (k.x == d && ki.x < idx) ? 1 : 0) + (k.y < d || (k.y == d && ki.y < idx) ? 1 : 0) +
                  (k.z < d || (k.z == d && ki.z < idx) ? 1 : 0) + (k.w < d || (k.w == d && ki.w < idx) ? 1 : 0);
        }
        if (rank < width) out[(int64_t)orig[r] * width + rank] = (int64_t)idx;
      }
    }
    if (use_rowbuf) {
      __syncthreads();
      // whole rows leave as contiguous runs: consecutive lanes, consecutive 16-byte pieces of a row.  An unwritten entry
      // below the row's hit count means two hits of that row have the same distance: the row is noted and redone below
      if ((width & 1) == 0) {
        const int w2 = width >> 1, total_pairs = rows_here * w2;
        const float inv = 1.0f / (float)w2;
        for (int i = tid; i < total_pairs; i += L::THREADS) {
          int r = (int)((float)i * inv);
          r = r * w2 > i ? r - 1 : ((r + 1) * w2 <= i ? r + 1 : r);
          const int cc = (i - r * w2) * 2;
          const int cnt = qtot[r];
          const uint2 v = *reinterpret_cast<const uint2*>(rowbuf + r * width + cc);
          if ((cc < cnt && v.x == PADMARK) || (cc + 1 < cnt && v.y == PADMARK)) {
            tie_rows[r] = 1;
            misc[1] = 1;
          }
          longlong2 o;
          o.x = cc < cnt ? (long long)v.x : (long long)pad_value;
          o.y = cc + 1 < cnt ? (long long)v.y : (long long)pad_value;
          *reinterpret_cast<longlong2*>(out + (int64_t)orig[r] * width + cc) = o;
        }
      } else {
        const int total_el = rows_here * width;
        const float inv = 1.0f / (float)width;
        for (int i = tid; i < total_el; i += L::THREADS) {
          int r = (int)((float)i * inv);
          r = r * width > i ? r - 1 : ((r + 1) * width <= i ? r + 1 : r);
          const int cc = i - r * width;
          const unsigned v = rowbuf[r * width + cc];
          if (cc < qtot[r] && v == PADMARK) {
            tie_rows[r] = 1;
            misc[1] = 1;
          }
          out[(int64_t)orig[r] * width + cc] = cc < qtot[r] ? (long long)v : (long long)pad_value;
        }
      }
      __syncthreads();
      // rows with equal distances (rare): rank their hits again on (distance, index) and overwrite the row's entries
      if (misc[1]) {
        for (int r = 0; r < rows_here; ++r) {
          if (!tie_rows[r]) continue;
          const int a = offs[r], len = qtot[r];
          for (int e = tid; e < len; e += L::THREADS) {
            const unsigned d = hd[a + e], idx = hm[a + e];
            int rank = 0;
            for (int q2 = 0; q2 < len; ++q2) {
              const unsigned dk = hd[a + q2], ik = hm[a + q2];
              rank += (dk < d || (dk == d && ik < idx)) ? 1 : 0;
            }
            if (rank < width) out[(int64_t)orig[r] * width + rank] = (int64_t)idx;
          }
        }
      }
    } else {
      // ---- padding of the group's rows: half a wave per row
      for (int r = glo + tid / 32; r < min(ghi, rows_here); r += L::THREADS / 32) {
        int64_t* row = out + (int64_t)orig[r] * width;
        for (int cc = (skip ? 0 : min(qtot[r], width)) + (lane & 31); cc < width; cc += 32) row[cc] = pad_value;
      }
      if (multi) __syncthreads();  // the next group overwrites the key area
    }
    glo = ghi;
  }
  if (tid == 0) {
    int mx = 0;
#pragma unroll
    for (int i = 0; i < RQ / WAVE; ++i) mx = max(mx, wsum[L::THREADS / WAVE + i]);
    blk_stats[2 * blk] = mx;
    blk_stats[2 * blk + 1] = blk_flag;
  }
}
