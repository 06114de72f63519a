// Radius search: which kernel a call site gets.  Plain host code, no HIP header (tests/radius_sites_driver.cpp).
// The thread-per-query kernel sorts up to NET hits per query in registers (NET = 32: the big levels of the data pyramid,
// 4 - 14 hits on average; NET = 64: its middle levels, ~30); where most queries of a wave have more, the kernel gives up
// after its tests and the call is repeated on count + fill.  A caller repeats the same (radius, limit) call site over and
// over (13 per pair in the pyramid), so a give-up is remembered per (radius bits, limit): the site moves up TQ_LEVELS --
// 32 -> 64 -> 64 behind the pre-selection (rows of a known width <= TQ_PRESEL_MAX: the coarsest levels, where a query has
// ~150 hits and keeps 49; other limits skip this level) -> count + fill -- and steps back down every TQ_RETRY_AFTER calls.
#pragma once
#include <cstdint>
#include <cstring>
#include <mutex>

namespace gr {

// the kernel of one search: count + fill, or tq_kernel's 32-hit network / 64-hit network / 64-hit network behind the pre-selection
enum class RadiusNet { CountFill, Net32, Net64, Net64Presel };
constexpr RadiusNet TQ_LEVELS[4] = {RadiusNet::Net32, RadiusNet::Net64, RadiusNet::Net64Presel, RadiusNet::CountFill};
constexpr int TQ_MEMO = 64, TQ_RETRY_AFTER = 256;
constexpr int64_t TQ_PRESEL_MAX = 56;  // the selection needs a bin boundary between `width` and 64 hits

inline bool tq_presel_ok(int64_t limit) { return limit >= 1 && limit <= TQ_PRESEL_MAX; }

class RadiusSites {
 public:
  // the kernel for this call of the site; an unknown site starts on the 32-hit network
  RadiusNet choose(float radius, int64_t limit) {
    std::lock_guard<std::mutex> lk(mu_);
    Site* e = find(bits(radius), limit);
    if (!e) return TQ_LEVELS[0];
    if (e->level > 0 && ++e->calls > TQ_RETRY_AFTER) {
      e->level = step(e->level, -1, limit);
      e->calls = 0;
    }
    return TQ_LEVELS[e->level];
  }
  // `net` gave up (or finished with more than an eighth of the queries beyond the network): the site starts one level
  // above `net` next time.  A site that never gave up takes no slot; a full table hands out its slots round-robin.
  void report(float radius, int64_t limit, RadiusNet net, bool gave_up) {
    if (!gave_up) return;
    std::lock_guard<std::mutex> lk(mu_);
    Site* e = find(bits(radius), limit);
    for (Site& c : sites_)
      if (!e && !c.used) e = &c;
    if (!e) e = &sites_[next_++ % TQ_MEMO];
    int level = 0;
    while (TQ_LEVELS[level] != net) ++level;
    *e = Site{bits(radius), limit, step(level, +1, limit), 0, true};
  }

 private:
  struct Site {
    uint32_t rbits;
    int64_t limit;
    int level;  // index into TQ_LEVELS
    int calls;  // calls at this level since it last changed
    bool used;
  };
  static uint32_t bits(float radius) {
    uint32_t rb;
    return memcpy(&rb, &radius, 4), rb;
  }
  // one level up (the last one stays) or down (from a level > 0), past the pre-selection where the limit rules it out
  static int step(int level, int dir, int64_t limit) {
    level = level + dir > 3 ? 3 : level + dir;
    if (TQ_LEVELS[level] == RadiusNet::Net64Presel && !tq_presel_ok(limit)) level += dir;
    return level;
  }
  Site* find(uint32_t rb, int64_t limit) {
    for (Site& e : sites_)
      if (e.used && e.rbits == rb && e.limit == limit) return &e;
    return nullptr;
  }
  Site sites_[TQ_MEMO] = {};
  unsigned next_ = 0;
  std::mutex mu_;
};

}  // namespace gr
