// The host-side decisions of a rasterizer forward frame, as plain host code (no HIP header; tests/raster_plan_driver.cpp
// drives it on the CPU): which launches count the tile instances, how the counts reach the host, what the scatter has to
// read, how much LDS it gets, and how the count words decode.  rasterizer.hip acts on a plan; it derives none of this itself.
// No heap allocation, no HIP call, no getenv, no lock: a plan is made on the critical path of every one-camera frame.
#pragma once

#include <cstdint>

namespace gr {

constexpr int BIN_T = 256;       // threads per binning workgroup (4 waves)
constexpr int BIN_CHUNK = 2048;  // depth-ordered Gaussians per chunk (count: a workgroup, scatter: a wave)
// many views: resident scatter workgroups per CU that the LDS staging block is sized for (measured at 1 M Gaussians,
// 640 x 480, 32 views: 4 / 5 / 6 / 8 -> 308 / 306 / 278 / 370 us; at 6, 2 % of the chunks take the direct path)
constexpr int SCATTER_WGS = 6;
constexpr int WIDE_T = 1024;  // threads per scatter workgroup for a few views per call
// what tile_scatter_kernel finds in seg_off / chunk_total when it starts (see the kernel)
constexpr int SEG_READ = 0, SEG_SELF_RAW = 1, SEG_SELF_SCAN = 2;
constexpr int SCATTER_ELIST = 1024;  // per wave: instance list of a step with rectangles of 5 .. 8 tiles a side
// stated here, asserted equal in rasterizer.hip (their own headers include HIP)
constexpr int PLAN_TILE = 16, PLAN_WAVE = 64, PLAN_SCAN_SINGLE_ROW = 2048, PLAN_MAX_VIEWS = 64;
constexpr int PLAN_KEY_DEPTH_BITS = 27;

// Which launches leave the chunk bases, the per-view totals and seg_off behind the depth sort:
//   CountScan   tile_count_kernel + seg_scan_kernel<true> (a few views, short chunk rows); the scatter reads seg_off
//   TotalsScan  chunk_total_kernel (unless the bucket launch of the depth sort left the totals) [+ chunk_max_kernel for long
//               rows] + exclusive_scan_i32; the scatter scans the tile counts of its chunk itself (SEG_SELF_SCAN)
//   SelfRaw     nothing: the bucket depth sort left the chunk totals, the scatter scans them, writes seg_off and mails the
//               counts (SEG_SELF_RAW)
enum class CountRoute { CountScan, TotalsScan, SelfRaw };
// How the counts reach the host:
//   Sync   copy on the frame's stream + stream synchronise (every plain frame)
//   Event  copy on a side stream, followed by an event
//   Mail   the counting kernel stores them into host-mapped memory and stamps them; the host polls the stamps
enum class Transport { Sync, Event, Mail };

// The preprocess kernel: Late fetches the SH coefficients only for Gaussians that survive the culling (one view, 16 aligned
// coefficients), Many leaves per-wave key ranges for the bucket depth sort (more than four views), Plain is the kernel as it was.
enum class PreprocessKind { Plain, Late, Many };

struct FramePlan {
  int V, gx, gy, tiles, nchunk;
  bool sh16;           // 16 SH coefficients per Gaussian, 16-byte aligned
  PreprocessKind preprocess;
  bool short_rows;     // a chunk row fits one scan launch, which then leaves totals and maxima as well
  bool deferred, mailbox;
  int key_bits;        // depth-sort key width: PLAN_KEY_DEPTH_BITS, or 32 after a far depth
  bool msd;            // the bucket depth sort (top-digit pass + in-LDS buckets) orders this frame
  bool totals_sorted;  // ... and its bucket launch adds up the chunk totals (many views)
  CountRoute route;
  Transport transport;
  int seg_mode;        // the scatter's SEG_* variant: what `route` left for it
  bool cam_in_args;    // one camera, deferred: the camera rides in the preprocess kernel's arguments and a far depth stores
                       // the frame's stamp -- no upload, no clear.  Only the mailbox compares the far word with a stamp.

  // bucket_sort: the caller wants the bucket depth sort (it is possible for this size and not cooling down)
  static FramePlan make(int64_t P, int V, int W, int H, bool sh16, bool deferred, bool mailbox, bool bucket_sort) {
    FramePlan p;
    p.V = V;
    p.gx = (W + PLAN_TILE - 1) / PLAN_TILE;
    p.gy = (H + PLAN_TILE - 1) / PLAN_TILE;
    p.tiles = p.gx * p.gy;
    p.nchunk = (int)((P + BIN_CHUNK - 1) / BIN_CHUNK);
    p.short_rows = p.nchunk <= PLAN_SCAN_SINGLE_ROW;
    p.deferred = deferred;
    p.mailbox = mailbox;
    p.key_bits = PLAN_KEY_DEPTH_BITS;
    p.msd = bucket_sort;
    p.sh16 = sh16;
    p.preprocess = sh16 && V == 1 ? PreprocessKind::Late : bucket_sort && V > 4 ? PreprocessKind::Many : PreprocessKind::Plain;
    p.cam_in_args = sh16 && V == 1 && deferred && mailbox && p.short_rows;
    p.route_from_sort();
    return p;
  }
  // the same frame ordered again after a bucket of the depth sort overflowed: three passes
  FramePlan without_buckets() const {
    FramePlan p = *this;
    p.msd = false;
    p.route_from_sort();
    return p;
  }
  // ... and after a depth past the compact keys: three passes over all 32 depth bits
  FramePlan with_full_keys() const {
    FramePlan p = without_buckets();
    p.key_bits = 32;
    return p;
  }

 private:
  void route_from_sort() {
    const bool few = short_rows && V <= 4;
    totals_sorted = msd && V > 4;
    route = few ? (msd && deferred && mailbox ? CountRoute::SelfRaw : CountRoute::CountScan) : CountRoute::TotalsScan;
    transport = !deferred ? Transport::Sync : few && mailbox ? Transport::Mail : Transport::Event;
    seg_mode = route == CountRoute::SelfRaw ? SEG_SELF_RAW : route == CountRoute::TotalsScan ? SEG_SELF_SCAN : SEG_READ;
  }
};

// The scatter's workgroup size and LDS: per-wave 16-bit tile cursors + a staging block that holds a whole chunk's instances
// (chunks that do not fit write straight to global memory) + per wave the instance list of a step with rectangles of 5 .. 8
// tiles a side, when it still fits.
struct ScatterPlan {
  int threads;      // a few views: WIDE_T, as long as the sixteen cursor rows leave room for the staging block
  int64_t cur_bytes;
  int stage_max;    // staging entries the LDS budget allows
  int stage_cap;    // ... and those asked for: the hint rounded up to 64, at most stage_max
  int elist_cap;
  int64_t lds;

  // stage_hint: the largest chunk total (this frame's; a speculative launch has last frame's, 0 = unknown)
  static ScatterPlan make(int tiles, int V, int64_t stage_hint, bool speculative) {
    ScatterPlan s;
    const bool wide = V <= 4 && (int64_t)(WIDE_T / PLAN_WAVE) * tiles * 4 <= 100 * 1024;
    s.threads = wide ? WIDE_T : BIN_T;
    const int waves = s.threads / PLAN_WAVE;
    // (the 256-thread scatter counts in a difference grid that IS the wave's cursor row: no LDS beyond the cursors)
    s.cur_bytes = (int64_t)waves * ((tiles + 1) & ~1) * 2;
    // many views: sized for SCATTER_WGS resident workgroups per CU (the chunks above that take the direct path), not for the
    // largest chunk -- the scatter is latency-bound and wants the waves
    int64_t budget = wide ? 156 * 1024 : 160 * 1024 / SCATTER_WGS - 512;
    if (budget < s.cur_bytes + 8 * 1024) budget = 78 * 1024;  // (huge images: two workgroups)
    const int64_t cap_max = (budget - s.cur_bytes) / 2;
    s.stage_max = (int)(cap_max > 0 ? cap_max : 0);
    int64_t want = stage_hint > 0 ? stage_hint : 0;
    // the hint is last frame's figure; a chunk that outgrows it writes straight to memory (a 25 % margin here cost a
    // resident workgroup per CU: + 16 % scatter time)
    if (speculative) want = want > 0 ? want + 64 : cap_max;
    const int64_t asked = (want + 63) / 64 * 64;
    s.stage_cap = (int)(asked < s.stage_max ? asked : s.stage_max);
    const int64_t base = s.cur_bytes + ((int64_t)s.stage_cap * 2 + 3) / 4 * 4;
    // (only for images whose rectangles are that large: at 640 x 480 the 16 KB would cost a resident workgroup per CU)
    s.elist_cap = tiles >= 4096 && base + (int64_t)waves * SCATTER_ELIST * 4 <= 156 * 1024 ? SCATTER_ELIST : 0;
    s.lds = base + (int64_t)waves * s.elist_cap * 4;
    return s;
  }
};

// The count words of a frame, as the counting kernels leave them:
//   copied (Sync, Event)  [V] totals, [V] per-view chunk maxima (short rows), [1] far word, [1] chunk maximum (long rows)
//   mailed (Mail)         [V] totals, [V] per-view chunk maxima, [1] far word, [V] stamps (short rows only)
// and the far word:
//   Sync   bit 0: a depth overflowed the compact keys; bit 1: a bucket of the depth sort overflowed
//   Event  the word was cleared in front of the frame: positive = far depth, negative = bucket overflow (the order is not
//          valid either way: the frame is redone)
//   Mail   nobody clears the word: it counts only when it equals this frame's stamp (far depth) or its negative (bucket
//          overflow); anything else is another frame's
struct Counts {
  int32_t totals[PLAN_MAX_VIEWS];
  int32_t chunk_max;
  bool far_depth;        // the frame has to be ordered again
  bool bucket_overflow;  // ... because a bucket overflowed
};
inline Counts decode_counts(const volatile int32_t* words, int V, bool short_rows, Transport transport, int far_seq) {
  Counts c;
  for (int v = 0; v < V; ++v) c.totals[v] = words[v];
  if (short_rows) {
    c.chunk_max = words[V];
    for (int v = 1; v < V; ++v) {
      const int32_t m = words[V + v];
      if (m > c.chunk_max) c.chunk_max = m;
    }
  } else {
    c.chunk_max = words[2 * V + 1];
  }
  const int32_t far = words[2 * V];
  switch (transport) {
    case Transport::Sync:
      c.far_depth = (far & 1) != 0;
      c.bucket_overflow = (far & 2) != 0;
      break;
    case Transport::Event:
      c.far_depth = far != 0;
      c.bucket_overflow = far < 0;
      break;
    case Transport::Mail:
      c.far_depth = far == far_seq || far == -far_seq;
      c.bucket_overflow = far == -far_seq;
      break;
  }
  return c;
}
// offset of view v's stamp among the mailed words
inline int mail_stamp_word(int V, int v) { return 2 * V + 1 + v; }

}  // namespace gr
