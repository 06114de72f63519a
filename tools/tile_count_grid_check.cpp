// Host copy of the arithmetic of tile_scatter_kernel's phase A (256-thread instances, csrc/rasterizer.hip): corner adds
// into a difference grid of signed 16-bit cells packed two to a 32-bit word, the two prefix passes (word form for an even
// number of tile columns, halfword form for an odd one) and the counts phase B then reads as unsigned halfwords --
// against a brute-force count over random rectangles.  Stand-alone, meant to run under the host sanitizers:
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/tile_count_grid_check.cpp -o check && ./check
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

namespace {
constexpr int CW = 512;  // rectangles per wave

struct Rect {
  int x0, y0, w, h;
};

// what a wave leaves in its cursor row: [row / 2] words = [row] halfword counts, row = tiles rounded up to even
std::vector<uint32_t> grid_counts(const std::vector<Rect>& rects, int gx, int gy) {
  const int tiles = gx * gy, row = (tiles + 1) & ~1;
  std::vector<uint32_t> myw(row / 2, 0u);
  auto corner = [&](int tile, uint32_t one) { myw.at(tile >> 1) += one << ((tile & 1) * 16); };
  for (const Rect& r : rects) {
    if (r.w * r.h == 0) continue;
    const int t00 = r.y0 * gx + r.x0, t10 = t00 + r.h * gx;
    const bool in_x = r.x0 + r.w < gx, in_y = r.y0 + r.h < gy;
    corner(t00, 1u);
    if (in_x) corner(t00 + r.w, ~0u);
    if (in_y) corner(t10, ~0u);
    if (in_x && in_y) corner(t10 + r.w, 1u);
  }
  if ((gx & 1) == 0) {
    const int nw = gx >> 1;
    for (int k = 0; k < nw; ++k) {  // lanes = word columns
      uint32_t run = 0u;
      for (int y = 0; y < gy; ++y) myw.at(y * nw + k) = run += myw.at(y * nw + k);
    }
    for (int y = 0; y < gy; ++y) {  // lanes = rows
      uint32_t front = 0u;
      for (int k = 0; k < nw; ++k) {
        uint32_t n = myw.at(y * nw + k);
        n += (n << 16) + front;
        front = (n >> 16) * 0x10001u;
        myw.at(y * nw + k) = n;
      }
    }
  } else {
    for (uint32_t& n : myw) n += (n & 0x8000u) << 1;
    std::vector<int16_t> g16(row);
    std::memcpy(g16.data(), myw.data(), row * sizeof(int16_t));  // (little-endian, as on the device)
    for (int x = 0; x < gx; ++x) {
      int run = 0;
      for (int y = 0; y < gy; ++y) g16.at(y * gx + x) = (int16_t)(run += g16.at(y * gx + x));
    }
    for (int y = 0; y < gy; ++y) {
      int run = 0;
      for (int x = 0; x < gx; ++x) g16.at(y * gx + x) = (int16_t)(run += g16.at(y * gx + x));
    }
    std::memcpy(myw.data(), g16.data(), row * sizeof(int16_t));
  }
  return myw;
}

int check(const std::vector<Rect>& rects, int gx, int gy, const char* what) {
  const int tiles = gx * gy;
  std::vector<int> want(tiles, 0);
  for (const Rect& r : rects)
    for (int y = r.y0; y < r.y0 + r.h; ++y)
      for (int x = r.x0; x < r.x0 + r.w; ++x) ++want.at(y * gx + x);
  const std::vector<uint32_t> got = grid_counts(rects, gx, gy);
  for (int t = 0; t < tiles; ++t) {
    const int g = (int)((got.at(t >> 1) >> ((t & 1) * 16)) & 0xffffu);  // cur16[tile]
    if (g != want[t]) {
      std::printf("MISMATCH %s: grid %d x %d, tile %d: %d, brute force %d\n", what, gx, gy, t, g, want[t]);
      return 1;
    }
  }
  if ((tiles & 1) && (got.back() >> 16) != 0u) {
    std::printf("MISMATCH %s: grid %d x %d, pad halfword not zero\n", what, gx, gy);
    return 1;
  }
  return 0;
}
}  // namespace

int main() {
  std::mt19937 rng(14);
  auto uni = [&](int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(rng); };
  int bad = 0, cases = 0;
  const int shapes[][2] = {{1, 1}, {2, 3}, {3, 2}, {1, 7}, {7, 1}, {40, 30}, {41, 31}, {120, 68}, {63, 38}, {255, 255}, {254, 3}};
  for (const auto& s : shapes) {
    const int gx = s[0], gy = s[1];
    for (int mode = 0; mode < 6; ++mode) {
      std::vector<Rect> rects;
      for (int i = 0; i < CW; ++i) {
        Rect r{0, 0, 0, 0};
        switch (mode) {
          case 0:  // small rectangles anywhere, some empty
            r.x0 = uni(0, gx - 1), r.y0 = uni(0, gy - 1);
            r.w = std::min(uni(0, 4), gx - r.x0), r.h = std::min(uni(0, 4), gy - r.y0);
            break;
          case 1:  // any rectangle
            r.x0 = uni(0, gx - 1), r.y0 = uni(0, gy - 1);
            r.w = uni(1, gx - r.x0), r.h = uni(1, gy - r.y0);
            break;
          case 2:  // all of the image, 512 deep
            r = {0, 0, gx, gy};
            break;
          case 3:  // ends on the right and bottom edge
            r.x0 = uni(0, gx - 1), r.y0 = uni(0, gy - 1);
            r.w = gx - r.x0, r.h = gy - r.y0;
            break;
          case 4:  // one tile, 512 deep: its right and lower neighbours go to -512 on the way
            r = {gx / 2, gy / 2, 1, 1};
            break;
          default:  // alternating columns of +512 / -512 in the difference grid
            r.x0 = 2 * uni(0, (gx - 1) / 2), r.y0 = 0;
            r.w = 1, r.h = gy;
            break;
        }
        rects.push_back(r);
      }
      char what[32];
      std::snprintf(what, sizeof what, "mode %d", mode);
      bad += check(rects, gx, gy, what);
      ++cases;
    }
  }
  std::printf("%d cases, %d mismatches\n", cases, bad);
  return bad != 0;
}
