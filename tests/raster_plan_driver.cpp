// Stand-alone driver of the rasterizer's frame plan (gaussreg_amd/csrc/raster_plan.hpp), built and run by
// tests/test_raster_frame_plan.py with the host compiler.  Commands on stdin, one per line, one line of numbers out for each:
//   plan <P> <V> <W> <H> <sh16> <deferred> <mailbox> <bucket_sort>
//        -> gx gy tiles nchunk short_rows preprocess cam_in_args, then for the plan, its without_buckets() and its
//           with_full_keys(): route transport seg_mode msd totals_sorted key_bits
//   scatter <tiles> <V> <stage_hint> <speculative>   -> threads cur_bytes stage_max stage_cap elist_cap lds
//   decode <V> <short_rows> <transport> <far_seq> <nwords> <word> ...   -> chunk_max far_depth bucket_overflow totals ...
// Enumerations are printed as their integer values (CountRoute: 0 CountScan, 1 TotalsScan, 2 SelfRaw; Transport: 0 Sync,
// 1 Event, 2 Mail; PreprocessKind: 0 Plain, 1 Late, 2 Many).
#include <cstdio>
#include <cstring>

#include "raster_plan.hpp"

static void print_route(const gr::FramePlan& p) {
  printf(" %d %d %d %d %d %d", (int)p.route, (int)p.transport, p.seg_mode, (int)p.msd, (int)p.totals_sorted, p.key_bits);
}

int main() {
  char cmd[16];
  while (scanf("%15s", cmd) == 1) {
    if (strcmp(cmd, "plan") == 0) {
      long long P;
      int V, W, H, sh16, deferred, mailbox, bucket;
      if (scanf("%lld %d %d %d %d %d %d %d", &P, &V, &W, &H, &sh16, &deferred, &mailbox, &bucket) != 8) return 2;
      const gr::FramePlan p = gr::FramePlan::make(P, V, W, H, sh16 != 0, deferred != 0, mailbox != 0, bucket != 0);
      printf("%d %d %d %d %d %d %d", p.gx, p.gy, p.tiles, p.nchunk, (int)p.short_rows, (int)p.preprocess, (int)p.cam_in_args);
      print_route(p);
      print_route(p.without_buckets());
      print_route(p.with_full_keys());
      printf("\n");
    } else if (strcmp(cmd, "scatter") == 0) {
      int tiles, V, spec;
      long long hint;
      if (scanf("%d %d %lld %d", &tiles, &V, &hint, &spec) != 4) return 2;
      const gr::ScatterPlan s = gr::ScatterPlan::make(tiles, V, hint, spec != 0);
      printf("%d %lld %d %d %d %lld\n", s.threads, (long long)s.cur_bytes, s.stage_max, s.stage_cap, s.elist_cap, (long long)s.lds);
    } else if (strcmp(cmd, "decode") == 0) {
      int V, short_rows, transport, far_seq, n;
      if (scanf("%d %d %d %d %d", &V, &short_rows, &transport, &far_seq, &n) != 5) return 2;
      if (V < 1 || V > gr::PLAN_MAX_VIEWS || n < 2 * V + 1 + (short_rows ? 0 : 1) || n > 4 * gr::PLAN_MAX_VIEWS) return 2;
      int32_t* words = new int32_t[n];  // exactly n words: a read past the layout is the sanitizer's to catch
      for (int i = 0; i < n; ++i)
        if (scanf("%d", &words[i]) != 1) return 2;
      const gr::Counts c = gr::decode_counts(words, V, short_rows != 0, (gr::Transport)transport, far_seq);
      printf("%d %d %d", c.chunk_max, (int)c.far_depth, (int)c.bucket_overflow);
      for (int v = 0; v < V; ++v) printf(" %d", c.totals[v]);
      printf("\n");
      delete[] words;
    } else {
      return 2;
    }
  }
  return 0;
}
