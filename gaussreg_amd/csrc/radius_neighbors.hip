// Fixed-radius neighbour search on MI355X: uniform-grid cell binning + per-query 27-cell scan.
//
// Replaces the reference's kd-tree path
//   geotransformer/extensions/cpu/radius_neighbors/radius_neighbors_cpu.cpp:3-91
// with a design that has no tree at all: the result of the reference depends only on
//   (1) fp32 d = ((dx*dx + dy*dy) + dz*dz)      (nanoflann.hpp:432-440)
//   (2) strict d < r*r                          (nanoflann.hpp:249-253)
//   (3) ascending-d order per query             (nanoflann.hpp:1287)
// so any exhaustive candidate enumeration that applies (1)-(3) is result-identical.  This file is
// compiled with -ffp-contract=off so (1) stays three multiplies and two adds.
//
// One translation unit: launchers, dispatch plan and entry points here, the kernels in headers (all launches on `stream`):
//   radius_grid.hpp      bbox, grid_setup, binning: supports (and queries) into cell order; the workspace layout
//   radius_traverse.hpp  count + fill: two passes with the host in between (the width the reference returns)
//   radius_fused.hpp     count + fill in ONE kernel for a width known before the launch (gr_radius_search mode 1)
//   radius_tq.hpp        one thread per query: the default search, and tq_expand_kernel for the bare search
//   radius_sites.hpp     (host only) which of these a (radius, limit) call site gets
// gr_radius_count_cached lets consecutive searches over the same supports and radius skip bbox .. binning for the support
// side (the data pyramid searches every level's supports three times).
#include <algorithm>
#include <atomic>
#include <cstdlib>

#include "common.hpp"
#include "radius_sites.hpp"

namespace gr {
namespace {

#include "radius_grid.hpp"
#include "radius_traverse.hpp"
#include "radius_fused.hpp"
#include "radius_tq.hpp"

// max / max over the per-block (max hits per query, hits per block) pairs -> hdr
// mail (optional): the header also goes to the host's mailbox page, stamped (common.hpp) -- no copy, no stream synchronise
__global__ __launch_bounds__(1024) void reduce_stats_kernel(const int32_t* __restrict__ blk_stats,
                                                            int blocks, RadiusHdr* __restrict__ hdr, int32_t* mail, int stamp,
                                                            int tq) {
  // tq: the second word of a block is (give-up code | wave-finished queries << 8): max of the codes, sum of the counts
  __shared__ int sh[3][1024 / WAVE];
  int mx = 0, ms = 0, sum = 0;
  for (int i = threadIdx.x; i < blocks; i += 1024) {
    mx = max(mx, blk_stats[2 * i]);
    const int v = blk_stats[2 * i + 1];
    ms = max(ms, tq ? (v & 255) : v);
    sum += tq ? (v >> 8) : 0;
  }
#pragma unroll
  for (int d = WAVE / 2; d > 0; d >>= 1) {
    mx = max(mx, __shfl_xor(mx, d, WAVE));
    ms = max(ms, __shfl_xor(ms, d, WAVE));
    sum += __shfl_xor(sum, d, WAVE);
  }
  if ((threadIdx.x & (WAVE - 1)) == 0) {
    sh[0][threadIdx.x / WAVE] = mx;
    sh[1][threadIdx.x / WAVE] = ms;
    sh[2][threadIdx.x / WAVE] = sum;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    mx = 0, ms = 0, sum = 0;
    for (int i = 0; i < 1024 / WAVE; ++i) {
      mx = max(mx, sh[0][i]);
      ms = max(ms, sh[1][i]);
      sum += sh[2][i];
    }
    hdr->max_count = (unsigned)mx;
    hdr->max_block_hits = (unsigned)ms;
    hdr->slow_sum = sum;
    if (mail) {
      mail[0] = mx;
      mail[1] = ms;
      mail[2] = hdr->total_cells;
      mail[3] = hdr->total_sup;
      mail[4] = sum;
      mail_post(mail + 5, stamp);
    }
  }
}

__global__ void pad_fill_kernel(int64_t* __restrict__ out, int64_t n, int64_t v) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = v;
}

// ---------------------------------------------------------------- host side
// What radius_prepare leaves behind for the launchers: the carved workspace with supports and queries in cell order.
struct Prepared {
  RadiusWs w;
  const float4* sorted_q;
  int64_t nq, ns;
  float r2;
  int nb;
  bool same;   // self-search
  bool empty;  // nothing to search: width 0
};

// The one carve of a call, with the size check of every entry point that takes a workspace.
int carve_checked(void* ws, size_t ws_bytes, int64_t nq, int64_t ns, int64_t batch, RadiusWs* w) {
  *w = carve(ws, nq, ns, batch);
  if (ws == nullptr || ws_bytes < w->bytes) {
    set_error("radius workspace too small: need %zu bytes, got %zu", w->bytes, ws_bytes);
    return GR_ERR_WORKSPACE;
  }
  return GR_OK;
}

// h_info[0..3] of every entry point (include/gaussreg_hip.h).  `block_hits`: the count pass's largest hit count of a block,
// -1 = the rows are tiles in the workspace (gr_radius_fill expands them), 0 = the rows are already in `out`.
void write_info(int64_t* h_info, const RadiusHdr& h, int64_t block_hits, bool same) {
  h_info[0] = h.max_count;
  h_info[1] = block_hits;
  h_info[2] = same ? 1 : 0;
  h_info[3] = h.total_cells;
}

// Reduces the per-block statistics into the header and brings the header to the host: through the mailbox page (the
// kernel posts it, the host polls -- no copy in the stream, no stream synchronise), else by a copy into pinned memory and a
// synchronise.  Everything queued on `stream` before is complete when this returns.
inline int reduce_and_read(const RadiusWs& w, int blocks, hipStream_t stream, RadiusHdr* h_out, bool tq = false) {
  volatile int32_t* mail = mailbox();
  if (mail) mail += MAIL_RADIUS;
  const int stamp = mail ? mailbox_next_stamp() : 0;
  if (mail) mailbox_arm(mail + 5);
  hipLaunchKernelGGL(reduce_stats_kernel, dim3(1), dim3(1024), 0, stream, w.blk_stats, blocks, w.hdr,
                     const_cast<int32_t*>(mail), stamp, tq ? 1 : 0);
  GR_LAUNCH_CHECK();
  if (mail) {
    int rc = mailbox_wait(mail + 5, stamp, stream, "radius search");
    if (rc != GR_OK) return rc;
    *h_out = RadiusHdr{(unsigned)mail[0], (unsigned)mail[1], mail[2], mail[3], mail[4]};
    return GR_OK;
  }
  RadiusHdr* h_pinned = static_cast<RadiusHdr*>(pinned_scratch(3, sizeof(RadiusHdr)));
  GR_REQUIRE(h_pinned != nullptr, "pinned read-back buffer could not be allocated");
  GR_HIP(hipMemcpyAsync(h_pinned, w.hdr, sizeof(RadiusHdr), hipMemcpyDeviceToHost, stream));
  GR_HIP(hipStreamSynchronize(stream));
  *h_out = *h_pinned;
  return GR_OK;
}

template <int RQ>
int launch_count(const Prepared& P, hipStream_t stream, RadiusHdr* h_out) {  // h_out: the header, on the host when this returns
  using L = TravLds<RQ>;
  const RadiusWs& w = P.w;
  const int blocks = (int)((P.nq + RQ - 1) / RQ);
  const int grid = (blocks + 7) / 8 * 8;
  KernelTimer timer("radius_count", stream);
  hipLaunchKernelGGL((traverse_kernel<RQ, false, true>), dim3(grid), dim3(L::THREADS), L::count_bytes(P.nb <= L::TABLE_MAX ? P.nb : 0), stream,
                     P.sorted_q, (int)P.nq, w.q_off, P.nb, w.grids, w.start, w.sorted_s, P.r2, w.q_count, w.q_rng, w.q_mask, w.blk_stats,
                     0, 0, P.ns, (int64_t*)nullptr, 0, (unsigned long long*)nullptr, (unsigned char*)nullptr, P.same ? 1 : 0);
  return reduce_and_read(w, blocks, stream, h_out);
}

template <int RQ>
int launch_fill(const RadiusWs& w, const float4* sorted_q, int64_t nq, int64_t ns, int nb, float r2, int64_t width,
                int64_t row_stride, int64_t max_block_hits, int64_t* out, hipStream_t stream) {
  using L = TravLds<RQ>;
  const int blocks = (int)((nq + RQ - 1) / RQ);
  const int grid = (blocks + 7) / 8 * 8;
  const int64_t cap = L::slots(max_block_hits);
  const size_t lds = L::total(cap);
  KernelTimer timer("radius_fill", stream);
  const bool in_lds = lds <= 160 * 1024;  // else (very dense neighbourhoods) hit lists live in a scratch allocation of this call
  auto kern = in_lds ? traverse_kernel<RQ, true, true> : traverse_kernel<RQ, true, false>;
  char* scratch = nullptr;
  const size_t hits_bytes = (size_t)grid * (size_t)cap * 8;
  if (in_lds && lds > 64 * 1024)
    GR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  if (!in_lds) GR_HIP(hipMallocAsync(reinterpret_cast<void**>(&scratch), hits_bytes / 8 * 9 + 256, stream));
  hipLaunchKernelGGL(kern, dim3(grid), dim3(L::THREADS), in_lds ? lds : L::FILL_OFF, stream, sorted_q, (int)nq, w.q_off, nb,
                     w.grids, w.start, w.sorted_s, r2, w.q_count, w.q_rng, w.q_mask, w.blk_stats, (int)width, (int)row_stride, ns,
                     out, (int)cap, reinterpret_cast<unsigned long long*>(scratch),
                     reinterpret_cast<unsigned char*>(in_lds ? nullptr : scratch + hits_bytes), 0);
  if (!in_lds) GR_HIP(hipFreeAsync(scratch, stream));
  GR_LAUNCH_CHECK();
  return GR_OK;
}

constexpr int FUSED_RQ = 64;     // queries per block: 30 KB of LDS, five blocks per CU (0.43 ms per 8 x 200 k; 128 queries: 0.50 ms)
constexpr int FUSED_PER_Q = 28;  // key slots per query in a block's key area

// GR_RADIUS_SINGLE_PASS=1 selects this single-pass kernel.  It is not the default: on 8 x 200 k points it runs as long as
// count + fill together (both are bound by VALU issue: ~3 000 instructions per wave either way)
int launch_fused(const Prepared& P, int64_t width, int64_t* out, hipStream_t stream, RadiusHdr* h_out) {
  constexpr int RQ = FUSED_RQ;
  using L = FusedLds<RQ>;
  const RadiusWs& w = P.w;
  const int blocks = (int)((P.nq + RQ - 1) / RQ);
  const int grid = (blocks + 7) / 8 * 8;
  const int tcap = P.nb <= L::TABLE_MAX ? P.nb : 0;
  // key area: FUSED_PER_Q slots per query, never less than two full rows, within the 160 KB of a CU
  int cap = max(FUSED_PER_Q * RQ, (int)(2 * width + 2));
  cap = (cap + 15) / 16 * 16;
  while (L::total((int)width, cap, tcap) > 160 * 1024 && cap > 64) cap -= 16;
  const size_t region = L::region_bytes((int)width);
  const size_t lds = L::total((int)width, cap, tcap);
  GR_REQUIRE(lds <= 160 * 1024, "radius_search: neighbor_limit %lld does not fit the single-pass kernel", (long long)width);
  auto kern = fused_kernel<RQ>;
  if (lds > 64 * 1024)
    GR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  {
    KernelTimer timer("radius_fused", stream);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(L::THREADS), lds, stream, P.sorted_q, (int)P.nq, w.q_off, P.nb, w.grids, w.start,
                       w.sorted_s, (int)P.ns, P.r2, w.blk_stats, (int)width, P.ns, out, cap, (int)region, P.same ? 1 : 0);
  }
  return reduce_and_read(w, blocks, stream, h_out);
}

inline bool fused_fits(int64_t width) {
  // the row buffer / key area of the largest configuration must fit next to the candidate planes
  return width >= 1 && FusedLds<FUSED_RQ>::total((int)width, (int)((2 * width + 2 + 15) / 16 * 16), 0) <= 160 * 1024;
}

// TQ_STOP=k (developer ablation): tq_kernel returns after its phase k, so results are invalid.  Read once.
int tq_stop() {
  static const int stop = getenv("TQ_STOP") ? atoi(getenv("TQ_STOP")) : 0;
  return stop;
}

// The five instantiations of tq_kernel: <NET, DIRECT (rows of a known width, written by the kernel), PRESEL>.
using TqKernel = decltype(&tq_kernel<32, true, false>);
TqKernel tq_kernel_for(RadiusNet net, bool direct) {
  if (net == RadiusNet::Net32) return direct ? tq_kernel<32, true, false> : tq_kernel<32, false, false>;
  if (!direct) return tq_kernel<64, false, false>;  // (no width to select for: the plain 64-hit network)
  return net == RadiusNet::Net64Presel ? tq_kernel<64, true, true> : tq_kernel<64, true, false>;
}

// One thread per query (radius_tq.hpp).  out != null: rows of `width` columns are written by the kernel; out == null: tiles +
// counts for launch_tq_expand.  h_out->max_block_hits != 0 = a workgroup gave up: the caller repeats the call on count + fill.
int launch_tq(const Prepared& P, RadiusNet net, int64_t width, int64_t* out, hipStream_t stream, RadiusHdr* h_out) {
  const RadiusWs& w = P.w;
  const int blocks = (int)((P.nq + WAVE - 1) / WAVE);
  const int grid = (blocks + 7) / 8 * 8;
  const bool direct = out != nullptr;
  const size_t rows_hi = (size_t)((P.nq + 63) / 64) * 64 * 32;
  {
    KernelTimer timer("radius_tq", stream);
    hipLaunchKernelGGL(tq_kernel_for(net, direct), dim3(grid), dim3(WAVE), 0, stream, P.sorted_q, (int)P.nq, w.q_off, P.nb, w.grids,
                       w.start, w.sorted_s, w.plane_x, w.plane_y, w.plane_z, (int)P.ns, P.r2, w.blk_stats, direct ? (int)width : 0,
                       P.ns, out, direct ? nullptr : w.tiles, direct ? nullptr : w.q_count, direct ? (size_t)0 : rows_hi,
                       P.same ? 1 : 0, direct ? tq_stop() : 0);
  }
  return reduce_and_read(w, blocks, stream, h_out, true);
}

int launch_tq_expand(const RadiusWs& w, int64_t nq, int64_t ns, int64_t width, int64_t* out, hipStream_t stream) {
  KernelTimer timer("radius_expand", stream);
  hipLaunchKernelGGL(tq_expand_kernel, dim3((unsigned)((nq + 63) / 64)), dim3(256), 0, stream, w.tiles, w.q_count,
                     (size_t)((nq + 63) / 64) * 64 * 32, (int)nq, (int)width, ns, out);
  GR_LAUNCH_CHECK();
  return GR_OK;
}

// ---------------------------------------------------------------- radius_prepare: everything up to the first traversal
int check_lengths(const int64_t* h_q_lengths, const int64_t* h_s_lengths, int64_t nq, int64_t ns, int64_t batch) {
  GR_REQUIRE(nq >= 0 && ns >= 0 && batch >= 0, "negative size");
  GR_REQUIRE(nq < (1ll << 31) - 1 && ns < (1ll << 31) - 1 && batch < (1 << 20),
             "radius_neighbors: sizes must fit int32 (nq=%lld ns=%lld)", (long long)nq, (long long)ns);
  int64_t sq = 0, ss = 0;
  for (int64_t b = 0; b < batch; ++b) {
    GR_REQUIRE(h_q_lengths[b] >= 0 && h_s_lengths[b] >= 0, "negative length in batch element %lld", (long long)b);
    sq += h_q_lengths[b];
    ss += h_s_lengths[b];
  }
  GR_REQUIRE(sq == nq && ss == ns, "lengths do not sum to the number of points (q %lld vs %lld, s %lld vs %lld)",
             (long long)sq, (long long)nq, (long long)ss, (long long)ns);
  return GR_OK;
}

// Signature of the support side (cloud pointer, sizes, radius, lengths): lets a caller that searches the same supports
// again (other queries, same radius -- the three searches per level of the data pyramid) skip the binning.  Checked
// against the preparing call's when `reuse`, then left in h_support_sig.
int support_signature(const float* s, const int64_t* h_s_lengths, int64_t ns, int64_t batch, float radius,
                      int64_t* h_support_sig, bool reuse) {
  int64_t sig[4] = {ns, batch, 0, (int64_t)reinterpret_cast<uintptr_t>(s)};
  uint32_t rb;
  memcpy(&rb, &radius, 4);
  uint64_t hsh = 1469598103934665603ull ^ rb;
  for (int64_t b = 0; b < batch; ++b) hsh = (hsh ^ (uint64_t)h_s_lengths[b]) * 1099511628211ull;
  sig[2] = (int64_t)hsh;
  if (reuse) {
    GR_REQUIRE(h_support_sig != nullptr, "reuse_support needs the signature written by the preparing call");
    GR_REQUIRE(memcmp(sig, h_support_sig, sizeof(sig)) == 0,
               "reuse_support: supports / lengths / radius differ from the call that prepared this workspace");
  }
  if (h_support_sig) memcpy(h_support_sig, sig, sizeof(sig));
  return GR_OK;
}

// q offsets | s offsets | bbox block offsets, staged in pinned memory (pinned_scratch: every call ends with a stream
// synchronise, so the previous call's copy has left the buffer) and copied to the device -- unless they ride in the first
// launch's arguments (few clouds, full binning: see OffsetArgs).
int stage_offsets(const RadiusWs& w, const int64_t* h_q_lengths, const int64_t* h_s_lengths, int64_t batch, bool reuse,
                  hipStream_t stream, int32_t** h_offsets) {
  int32_t* const tmp = static_cast<int32_t*>(pinned_scratch(2, sizeof(int32_t) * 3 * (batch + 1)));
  GR_REQUIRE(tmp != nullptr, "pinned staging buffer could not be allocated");
  tmp[0] = tmp[batch + 1] = 0;
  for (int64_t b = 0; b < batch; ++b) {
    tmp[b + 1] = tmp[b] + (int32_t)h_q_lengths[b];
    tmp[batch + 1 + b + 1] = tmp[batch + 1 + b] + (int32_t)h_s_lengths[b];
  }
  if (!reuse) {  // first bounding-box block of every cloud
    int32_t* blk = tmp + 2 * (batch + 1);
    blk[0] = 0;
    for (int64_t b = 0; b < batch; ++b) blk[b + 1] = blk[b] + (int32_t)((h_s_lengths[b] + BBOX_PTS - 1) / BBOX_PTS);
  }
  if (reuse || batch > KARG_CLOUDS)
    GR_HIP(hipMemcpyAsync(w.q_off, tmp, sizeof(int32_t) * (reuse ? 1 : 3) * (batch + 1), hipMemcpyHostToDevice, stream));
  *h_offsets = tmp;
  return GR_OK;
}

// bbox .. cell order: supports and queries (nothing is launched when the grid is reused in a self-search)
int bin_points(const RadiusWs& w, const float* q, const float* s, int64_t nq, int64_t ns, int64_t batch, float radius,
               bool same, bool reuse, const int32_t* h_offsets, hipStream_t stream) {
  const int nb = (int)batch;
  KernelTimer bin_timer("radius_bin", stream);
  const int64_t su = w.nsup + 1;
  BinSide A{s, (int)ns, w.s_off, w.s_cell, w.pairs_s, w.sup_zero, w.sup_zero + 2 * su, w.sup_start, w.sorted_s, w.start,
            w.plane_x, w.plane_y, w.plane_z};
  BinSide B{q, (int)nq, w.q_off, w.q_cell, w.pairs_q, w.sup_zero + su, w.sup_zero + 3 * su, w.sup_start + su, w.sorted_q, nullptr,
            nullptr, nullptr, nullptr};
  if (reuse && same) return GR_OK;
  if (!reuse) {
    // ---- supports (and, in the launches below, the queries): bbox and grid in front of the two-level counting sort
    OffsetArgs ka;
    if (batch <= KARG_CLOUDS) {
      GR_REQUIRE(w.s_off == w.q_off + (batch + 1) && w.blk_off == w.q_off + 2 * (batch + 1), "radius workspace layout");
      memcpy(ka.v, h_offsets, sizeof(int32_t) * 3 * (batch + 1));
    }
    hipLaunchKernelGGL(batch <= KARG_CLOUDS ? bbox_partial_kernel<true> : bbox_partial_kernel<false>,
                       dim3(h_offsets[2 * (batch + 1) + batch]), dim3(256), 0, stream, s, w.s_off, w.blk_off, nb, w.bbox_partial,
                       w.sup_zero, (int)(4 * su), ka, w.q_off);
    // x sub-cells per cell: 2 measured best end to end (count pass 0.166 -> 0.157 ms; 8 gives 0.150 ms but the scan and the
    // scatter over an 8x larger cell table take the difference back)
    constexpr int xk_max = 2;
    hipLaunchKernelGGL(grid_setup_kernel, dim3(1), dim3(256), 0, stream, w.bbox, w.bbox_partial, w.blk_off, w.s_off, nb, radius,
                       xk_max, w.grids, w.hdr, w.sup_off);
  } else {
    // ---- the support grid is in place: only the queries are binned into it
    hipLaunchKernelGGL(bin_init2_kernel, dim3(std::min(256, ((int)su + 255) / 256)), dim3(256), 0, stream, w.sup_zero + su,
                       w.sup_zero + 3 * su, (int)su);
  }
  // blocks of side A (supports) and B (queries) in the shared launches; a side that is in place already has none
  const int blocks_s = reuse ? 0 : (int)((ns + COARSE_PTS - 1) / COARSE_PTS), blocks_q = same ? 0 : (int)((nq + COARSE_PTS - 1) / COARSE_PTS);
  const int fine_blocks = (int)std::min<int64_t>(w.nsup, 4096), sides = reuse || same ? 1 : 2;
  hipLaunchKernelGGL((coarse_kernel<false>), dim3(blocks_s + blocks_q), dim3(256), 0, stream, A, B, blocks_s, nb, w.grids);
  hipLaunchKernelGGL(sup_scan_kernel, dim3(sides), dim3(1024), 0, stream, A, B, reuse ? 1 : 0, w.hdr);
  hipLaunchKernelGGL((coarse_kernel<true>), dim3(blocks_s + blocks_q), dim3(256), 0, stream, A, B, blocks_s, nb, w.grids);
  hipLaunchKernelGGL(fine_kernel, dim3((unsigned)(fine_blocks * sides)), dim3(256), 0, stream, A, B, reuse ? 0 : fine_blocks, nb,
                     w.grids, w.sup_off, w.hdr);
  GR_LAUNCH_CHECK();
  return GR_OK;
}

int radius_prepare(const float* q, const float* s, const int64_t* h_q_lengths, const int64_t* h_s_lengths, int64_t nq,
                   int64_t ns, int64_t batch, float radius, void* ws, size_t ws_bytes, int64_t* h_support_sig,
                   int reuse_support, hipStream_t stream, Prepared* out_p) {
  out_p->empty = true;
  int rc = check_lengths(h_q_lengths, h_s_lengths, nq, ns, batch);
  if (rc != GR_OK || nq == 0 || ns == 0 || batch == 0) return rc;  // an error, or width 0
  RadiusWs w;
  if ((rc = carve_checked(ws, ws_bytes, nq, ns, batch, &w)) != GR_OK) return rc;
  const bool same = (q == s) && (nq == ns) && memcmp(h_q_lengths, h_s_lengths, sizeof(int64_t) * batch) == 0;
  const bool reuse = reuse_support != 0;
  int32_t* h_offsets = nullptr;
  if ((rc = support_signature(s, h_s_lengths, ns, batch, radius, h_support_sig, reuse)) != GR_OK) return rc;
  if ((rc = stage_offsets(w, h_q_lengths, h_s_lengths, batch, reuse, stream, &h_offsets)) != GR_OK) return rc;
  if ((rc = bin_points(w, q, s, nq, ns, batch, radius, same, reuse, h_offsets, stream)) != GR_OK) return rc;
  // (r2: the fp32 product of radius_neighbors_cpu.cpp:12)
  *out_p = Prepared{w, same ? w.sorted_s : w.sorted_q, nq, ns, radius * radius, (int)batch, same, false};
  return GR_OK;
}

// ---------------------------------------------------------------- dispatch
// gr_radius_search_mode: 0 = count, host, fill; 1 = the single-pass kernel (three threads per query); 2 = one thread per
// query (radius_tq.hpp), always tried first (32-hit network); 3 (default) = the kernel the call-site memory picks (32-hit
// network, 64-hit network, 64-hit network behind the pre-selection, or count + fill); 4 = the 64-hit network always tried
// first; 5 = the same behind the pre-selection where the limit allows it, else the plain 64-hit network.
// Initialised from GR_RADIUS_SINGLE_PASS.
std::atomic<int>& search_mode() {
  static std::atomic<int> mode{[] {
    const char* a = getenv("GR_RADIUS_SINGLE_PASS");
    return (a && a[0] >= '0' && a[0] <= '5') ? a[0] - '0' : 3;
  }()};
  return mode;
}

RadiusSites g_sites;

// The kernel one search starts on.  `limit`: the row width of gr_radius_search, -1 for the bare search (no width to select
// for).  CountFill also stands for "no thread-per-query kernel": modes 0 and 1, and supports beyond the kernels' 2^29.
RadiusNet plan_search(int mode, int64_t ns, float radius, int64_t limit) {
  if (ns >= (1ll << 29)) return RadiusNet::CountFill;
  switch (mode) {
    case 2: return RadiusNet::Net32;
    case 3: return g_sites.choose(radius, limit);
    case 4: return RadiusNet::Net64;
    case 5: return tq_presel_ok(limit) ? RadiusNet::Net64Presel : RadiusNet::Net64;
    default: return RadiusNet::CountFill;
  }
}

// The count pass and its h_info; the fill follows in gr_radius_fill or at the end of gr_radius_search.
int count_pass(const Prepared& P, hipStream_t stream, int64_t* h_info, RadiusHdr* h) {
  int rc = launch_count<RT>(P, stream, h);
  if (rc == GR_OK) write_info(h_info, *h, h->max_block_hits, P.same);
  return rc;
}

}  // namespace
}  // namespace gr

using namespace gr;

extern "C" size_t gr_radius_workspace_bytes(int64_t nq, int64_t ns, int64_t batch) {
  if (nq < 0 || ns < 0 || batch < 0) return 0;
  return carve(nullptr, nq, ns, batch).bytes;
}

extern "C" int gr_radius_count(const float* q, const float* s, const int64_t* h_q_lengths, const int64_t* h_s_lengths,
                               int64_t nq, int64_t ns, int64_t batch, float radius, void* ws, size_t ws_bytes, int64_t* h_info,
                               void* stream_) {
  return gr_radius_count_cached(q, s, h_q_lengths, h_s_lengths, nq, ns, batch, radius, ws, ws_bytes, h_info, nullptr, 0,
                                stream_);
}

extern "C" int gr_radius_count_cached(const float* q, const float* s, const int64_t* h_q_lengths, const int64_t* h_s_lengths,
                                      int64_t nq, int64_t ns, int64_t batch, float radius, void* ws, size_t ws_bytes,
                                      int64_t* h_info, int64_t* h_support_sig, int reuse_support, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  GR_REQUIRE(h_info != nullptr, "h_info is null");
  h_info[0] = h_info[1] = h_info[2] = h_info[3] = 0;
  Prepared P;
  int rc = radius_prepare(q, s, h_q_lengths, h_s_lengths, nq, ns, batch, radius, ws, ws_bytes, h_support_sig, reuse_support,
                          stream, &P);
  if (rc != GR_OK || P.empty) return rc;  // an error, or nothing to search: width 0
  RadiusHdr h;
  const int mode = search_mode().load();
  const RadiusNet net = plan_search(mode, ns, radius, -1);
  if (net != RadiusNet::CountFill) {
    // one thread per query: the whole search now (sorted compact rows), gr_radius_fill only widens them
    rc = launch_tq(P, net, 0, nullptr, stream, &h);
    if (rc != GR_OK) return rc;
    const bool done = h.max_block_hits == 0 && h.max_count <= (unsigned)TQ_ROW_CAP;
    // (a finished call most of whose waves needed the exact path is reported too: the next call of the site starts higher)
    if (mode == 3) g_sites.report(radius, -1, net, !done || (int64_t)h.slow_sum * 8 > nq);
    if (done) {
      write_info(h_info, h, -1, P.same);
      return GR_OK;
    }
  }
  return count_pass(P, stream, h_info, &h);
}

extern "C" int gr_radius_fill(const float* q, const float* s, int64_t nq, int64_t ns, int64_t batch,
                              float radius, int64_t width, const int64_t* h_info, int64_t* out,
                              void* ws, size_t ws_bytes, void* stream_) {
  (void)q, (void)s;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  GR_REQUIRE(h_info != nullptr, "h_info is null");
  GR_REQUIRE(width >= 0 && width <= (1 << 30), "bad width %lld", (long long)width);
  if (nq == 0 || width == 0) return GR_OK;
  GR_REQUIRE(out != nullptr, "out is null");
  if (ns == 0 || batch == 0 || h_info[0] == 0) {
    // nothing matched anywhere: a caller that insists on a fixed width gets all-padding rows
    const int64_t n = nq * width;
    hipLaunchKernelGGL(pad_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, out, n, ns);
    GR_LAUNCH_CHECK();
    return GR_OK;
  }
  RadiusWs w;
  int rc = carve_checked(ws, ws_bytes, nq, ns, batch, &w);
  if (rc != GR_OK) return rc;
  if (h_info[1] == -1) return launch_tq_expand(w, nq, ns, width, out, stream);
  return launch_fill<RT>(w, h_info[2] != 0 ? w.sorted_s : w.sorted_q, nq, ns, (int)batch, radius * radius, width, width,
                         h_info[1], out, stream);
}

extern "C" int gr_radius_search_mode(int mode) {
  const int old = search_mode().load();
  if (mode >= 0 && mode <= 5) search_mode().store(mode);
  return old;
}

extern "C" int gr_radius_search(const float* q, const float* s, const int64_t* h_q_lengths, const int64_t* h_s_lengths,
                                int64_t nq, int64_t ns, int64_t batch, float radius, int64_t limit, int64_t* out, void* ws,
                                size_t ws_bytes, int64_t* h_info, int64_t* h_support_sig, int reuse_support, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  GR_REQUIRE(h_info != nullptr, "h_info is null");
  for (int i = 0; i < 6; ++i) h_info[i] = 0;
  GR_REQUIRE(limit >= 1 && limit <= (1 << 20), "radius_search: neighbor_limit must be positive (got %lld)", (long long)limit);
  GR_REQUIRE(out != nullptr || nq == 0, "out is null");
  Prepared P;
  int rc = radius_prepare(q, s, h_q_lengths, h_s_lengths, nq, ns, batch, radius, ws, ws_bytes, h_support_sig, reuse_support,
                          stream, &P);
  if (rc != GR_OK || P.empty) return rc;  // an error, or nothing to search: width 0
  RadiusHdr h;
  const int mode = search_mode().load();
  const RadiusNet net = plan_search(mode, ns, radius, limit);
  const bool tq = net != RadiusNet::CountFill;
  if (tq || (mode == 1 && fused_fits(limit))) {  // one kernel writes the (nq, limit) rows
    rc = tq ? launch_tq(P, net, limit, out, stream, &h) : launch_fused(P, limit, out, stream, &h);
    if (rc != GR_OK) return rc;
    if (tq && mode == 3) g_sites.report(radius, limit, net, h.max_block_hits != 0 || (int64_t)h.slow_sum * 8 > nq);
    write_info(h_info, h, 0, P.same);
    if (h.max_block_hits == 0) {  // no query overflowed its block's key area: `out` is complete
      h_info[4] = 1;
      return GR_OK;
    }
  }
  // count, host, fill: the first min(max_count, limit) columns of the (nq, limit) rows.  (Measured and dropped: launching the
  // fill behind the count with an LDS key area sized from the previous call of the same shape, to take the host out of the
  // middle -- 0.594 vs 0.579 ms per 8 x 200 k points: the host prepares the fill while the count runs; what is left of it
  // sits between calls, not between the kernels.)
  rc = count_pass(P, stream, h_info, &h);
  if (rc != GR_OK || h.max_count == 0) return rc;  // an error, or width 0
  const int64_t width = h.max_count < (uint64_t)limit ? (int64_t)h.max_count : limit;
  return launch_fill<RT>(P.w, P.sorted_q, nq, ns, P.nb, P.r2, width, limit, h.max_block_hits, out, stream);
}
