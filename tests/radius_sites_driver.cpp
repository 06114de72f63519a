// Stand-alone driver of the radius search's call-site memory (gaussreg_amd/csrc/radius_sites.hpp), built and run by
// tests/test_radius_call_sites.py with the host compiler.  Commands on stdin, one per line, radius as its fp32 bits:
//   choose <radius bits> <limit>                      -> prints the kernel the site gets
//   report <radius bits> <limit> <kernel> <gave_up>   -> prints nothing
// Kernels are written 32, 64, presel, count_fill.
#include <cstdio>
#include <cstring>

#include "radius_sites.hpp"

static const char* const NAMES[4] = {"count_fill", "32", "64", "presel"};  // indexed by RadiusNet

int main() {
  gr::RadiusSites sites;
  char cmd[16], name[16];
  unsigned bits;
  long long limit;
  int gave_up;
  while (scanf("%15s %u %lld", cmd, &bits, &limit) == 3) {
    float radius;
    memcpy(&radius, &bits, 4);
    if (strcmp(cmd, "choose") == 0) {
      puts(NAMES[(int)sites.choose(radius, limit)]);
    } else if (strcmp(cmd, "report") == 0 && scanf("%15s %d", name, &gave_up) == 2) {
      int net = 0;
      while (net < 4 && strcmp(NAMES[net], name) != 0) ++net;
      if (net == 4) return 2;
      sites.report(radius, limit, (gr::RadiusNet)net, gave_up != 0);
    } else {
      return 2;
    }
  }
  return 0;
}
