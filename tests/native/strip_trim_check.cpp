// Host check of the trimmed window of the strip kernels (mcmc_gpu_amd/csrc/strip_step.h: the make_window overload that takes the
// static rectangle of StaticFields -- the bounding box of the update mask grown by one cell).  The helpers are __host__ __device__,
// so this program runs the code the kernels run; it calls no HIP runtime function.  tests/native/strip_geometry_check.cpp checks the
// untrimmed chain; this one runs make_window(.., rectangle) -> config -> lane_setup -> write_masks / cell_written for all 8 x 64
// (wave, lane) pairs with the INTERIOR value the trimmed window reports:
//   window       the trimmed window is the grid-clipped window (restated from the oracle's window_bounds) intersected with the
//                rectangle; mr0 / mc0 move on by the rows / columns cut at the top / left; interior is that of the trimmed window;
//                no common cell: wh = ww = 0, n = 0, no lane valid, rows = -2 in every lane, nothing written
//   whole grid   a rectangle that is the grid gives the six-argument make_window field for field
//   ownership    the cells row_own && kFColOwn, addressed cell0 + jj * W in uint32 as the kernels do, hit every cell of the trimmed
//                window exactly once and no other cell
//   indices      fidx and tidx of an own cell are the ones the UNTRIMMED window gives that grid cell: it keeps its place in the
//                bh x bw proposal field and in the (bh + 2) x (bw + 2) tile
//   tile writes  cell_written for jj = 0 .. n + 1 at tidx + jj * (bw + 2): inside the tile; every write puts the bed of the grid cell
//                that belongs at that tile cell (one value per tile cell, whoever writes it); cells of the trimmed window exactly
//                once; the non-corner cells of its ring that exist in the grid at least once (several row strips write the same
//                halo-column cell, as in the untrimmed window); ring cells outside the grid and every other tile cell never
//   depth        n <= kNR, and never more than the untrimmed window's n
// Sweep (block sizes and centres thinned so that the program runs in seconds): the grids, block ranges and masks of
// tests/test_gpu_strip_trim.py and the headline 256 x 256 problem, centres over the whole grid (windows clipped and unclipped), and
// per grid the rectangles: the whole grid, the case's own, one touching each grid edge, one row high, one column wide, a single
// cell, and empty.  It prints what it saw and fails if a kind of window was not seen.
// With sanitizers, as the stand-alone program it is:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I mcmc_gpu_amd/csrc \
//         -o strip_trim_check_san tests/native/strip_trim_check.cpp && ./strip_trim_check_san
#include "strip_step.h"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

using namespace gsm::strip;

static long g_fail = 0;
#define CHECK(cond, ...)                                                       \
  do {                                                                         \
    if (!(cond)) {                                                             \
      if (g_fail < 20) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } \
      ++g_fail;                                                                \
    }                                                                          \
  } while (0)

struct Rect { int r0, r1, c0, c1; };
struct Tally { long windows, same, empty, top, bottom, left, right, regrouped, shallower, interior, clipped, grid_clipped; int deepest; };
static Tally g_t = {};

static std::vector<uint8_t> g_cnt, g_tcnt;
static std::vector<uint32_t> g_touched;
static std::vector<int> g_ttouched;

template <bool INTERIOR>
static void tile_writes(const Lane& L, int n, int W, int ts, int tile_len, const Window& g0) {
  const WriteMasks wm = write_masks(L);
  for (int jj = 0; jj <= n + 1; ++jj) {
    if (!cell_written<INTERIOR>(L, wm, jj)) continue;
    const long ti = (long)L.tidx + (long)jj * ts;
    CHECK(ti >= 0 && ti < tile_len, "tile index %ld of %d", ti, tile_len);
    if (ti < 0 || ti >= tile_len) continue;
    // the grid cell whose bed the lane writes is the one that belongs at this tile cell (block cell (y, x) at (y + 1, x + 1))
    const uint32_t idx = L.cell0 + (uint32_t)(jj * W);
    const int r = (int)(idx / (uint32_t)W), c = (int)(idx % (uint32_t)W);
    const int ty = (int)(ti / ts), tx = (int)(ti % ts);
    CHECK(r == g0.r0 - g0.mr0 + ty - 1 && c == g0.c0 - g0.mc0 + tx - 1, "tile cell (%d, %d) written with the bed of (%d, %d)", ty, tx, r, c);
    if (g_tcnt[ti]++ == 0) g_ttouched.push_back((int)ti);
  }
}

static void check_window(int H, int W, int row, int col, int bh, int bw, const Rect& q) {
  // the oracle's window_bounds (oracle/mcmc_oracle.py, MCMC.py:1266-1276), bh and bw even; then the intersection, restated
  const int ur0 = std::max(0, row - bh / 2), ur1 = std::min(H, row + bh / 2);
  const int uc0 = std::max(0, col - bw / 2), uc1 = std::min(W, col + bw / 2);
  const int umr0 = std::max(bh - ur1, 0), umc0 = std::max(bw - uc1, 0);
  int r0 = std::max(ur0, q.r0), r1 = std::min(ur1, q.r1), c0 = std::max(uc0, q.c0), c1 = std::min(uc1, q.c1);
  const bool empty = r1 <= r0 || c1 <= c0;
  if (empty) { r1 = r0 = ur0; c1 = c0 = uc0; }
  const int wh = r1 - r0, ww = c1 - c0;

  const Window g0 = make_window(H, W, row, col, bh, bw);
  const Window g = make_window(H, W, row, col, bh, bw, q.r0, q.r1, q.c0, q.c1);
  CHECK(g.wh == wh && g.ww == ww && g.bw == bw, "size %d x %d, expected %d x %d (H %d W %d row %d col %d bh %d bw %d)", g.wh, g.ww, wh, ww, H, W, row, col, bh, bw);
  if (!empty) {
    CHECK(g.r0 == r0 && g.c0 == c0 && g.mr0 == umr0 + r0 - ur0 && g.mc0 == umc0 + c0 - uc0, "origin (H %d W %d row %d col %d bh %d bw %d)", H, W, row, col, bh, bw);
    CHECK(g.interior == (r0 > 0 && r1 < H && c0 > 0 && c1 < W), "interior (H %d W %d row %d col %d bh %d bw %d)", H, W, row, col, bh, bw);
  }
  if (q.r0 <= 0 && q.r1 >= H && q.c0 <= 0 && q.c1 >= W)
    CHECK(g.r0 == g0.r0 && g.c0 == g0.c0 && g.wh == g0.wh && g.ww == g0.ww && g.mr0 == g0.mr0 && g.mc0 == g0.mc0 && g.bw == g0.bw && g.interior == g0.interior,
          "whole-grid rectangle differs from the six-argument window (H %d W %d row %d col %d bh %d bw %d)", H, W, row, col, bh, bw);
  const Cfg c = config(g.wh, g.ww), cu = config(g0.wh, g0.ww);
  CHECK(c.n <= kNR && c.n <= cu.n, "n %d (untrimmed %d) at wh %d ww %d", c.n, cu.n, wh, ww);
  if (c.n > kNR) return;

  const uint32_t cells = (uint32_t)(H * W);
  const int ts = bw + 2, tile_len = (bh + 2) * (bw + 2);
  if (g_cnt.size() < cells) g_cnt.assign(cells, 0);
  if ((int)g_tcnt.size() < tile_len) g_tcnt.assign(tile_len, 0);
  g_touched.clear();
  g_ttouched.clear();

  for (int wave = 0; wave < kSW; ++wave) {
    for (int lane = 0; lane < 64; ++lane) {
      const Lane L = lane_setup(lane, wave, c, g, H, W);
      if (empty) CHECK(L.rows == -2 && !has(L, kFValid) && !has(L, kFColIn) && !has(L, kFColOwn), "empty window: wave %d lane %d has work", wave, lane);
      if (has(L, kFColOwn)) {
        for (int jj = 1; jj <= kNR; ++jj) {
          if (!row_own(L, jj)) continue;
          const uint32_t idx = L.cell0 + (uint32_t)(jj * W);
          CHECK(idx < cells, "own cell %u of %u (wave %d lane %d jj %d)", idx, cells, wave, lane, jj);
          if (idx >= cells) continue;
          const int r = (int)(idx / (uint32_t)W), cc = (int)(idx % (uint32_t)W);
          CHECK(r >= r0 && r < r1 && cc >= c0 && cc < c1, "own cell (%d, %d) outside the trimmed window [%d, %d) x [%d, %d)", r, cc, r0, r1, c0, c1);
          CHECK(L.fidx + jj * bw == (umr0 + r - ur0) * bw + umc0 + cc - uc0, "fidx of (%d, %d)", r, cc);
          CHECK(L.tidx + jj * ts == (umr0 + r - ur0 + 1) * ts + umc0 + cc - uc0 + 1, "tidx of (%d, %d)", r, cc);
          if (g_cnt[idx]++ == 0) g_touched.push_back(idx);
          CHECK(g_cnt[idx] == 1, "cell (%d, %d) owned %d times", r, cc, (int)g_cnt[idx]);
        }
      }
      if (g.interior) tile_writes<true>(L, c.n, W, ts, tile_len, g0);
      else tile_writes<false>(L, c.n, W, ts, tile_len, g0);
    }
  }
  CHECK((long)g_touched.size() == (long)wh * ww, "%zu of %d window cells owned (H %d W %d row %d col %d bh %d bw %d, rectangle [%d, %d) x [%d, %d))",
        g_touched.size(), wh * ww, H, W, row, col, bh, bw, q.r0, q.r1, q.c0, q.c1);
  for (uint32_t idx : g_touched) g_cnt[idx] = 0;

  for (int ty = 0; ty < bh + 2; ++ty) {
    for (int tx = 0; tx < bw + 2; ++tx) {
      const int k = g_tcnt[ty * ts + tx];
      const int r = ur0 - umr0 + ty - 1, cc = uc0 - umc0 + tx - 1;          // the grid cell of the tile cell
      const int wy = r - r0, wx = cc - c0;                                  // ... in coordinates of the trimmed window
      const bool in_window = wy >= 0 && wy < wh && wx >= 0 && wx < ww;
      const bool in_ring = !empty && !in_window && wy >= -1 && wy <= wh && wx >= -1 && wx <= ww;
      const bool corner = (wy == -1 || wy == wh) && (wx == -1 || wx == ww);
      const bool in_grid = r >= 0 && r < H && cc >= 0 && cc < W;
      if (in_window) CHECK(k == 1, "window cell (%d, %d) written %d times (H %d W %d row %d col %d bh %d bw %d)", r, cc, k, H, W, row, col, bh, bw);
      else if (in_ring && !in_grid) CHECK(k == 0, "ring cell (%d, %d) outside the grid written", r, cc);
      else if (in_ring && !corner) CHECK(k >= 1, "ring cell (%d, %d) not written (H %d W %d row %d col %d bh %d bw %d)", r, cc, H, W, row, col, bh, bw);
      else if (!in_ring) CHECK(k == 0, "tile cell (%d, %d) outside window and ring written", ty, tx);
    }
  }
  for (int ti : g_ttouched) g_tcnt[ti] = 0;

  ++g_t.windows;
  const bool grid_clipped = g0.wh < bh || g0.ww < bw;
  g_t.grid_clipped += grid_clipped;
  if (empty) { ++g_t.empty; return; }
  if (wh == g0.wh && ww == g0.ww) { ++g_t.same; return; }
  g_t.top += r0 > ur0; g_t.bottom += r1 < ur1; g_t.left += c0 > uc0; g_t.right += c1 < uc1;
  if (c.g != cu.g || c.sr != cu.sr) ++g_t.regrouped;
  else if (c.n < cu.n) ++g_t.shallower;
  g_t.interior += g.interior; g_t.clipped += !g.interior;
  g_t.deepest = std::max(g_t.deepest, c.n);
}

// rows / columns 0, 1, n - 2, n - 1 and every stride-th one from 2
static std::vector<int> positions(int n, int stride) {
  std::set<int> s;
  for (int v : {0, 1, n - 2, n - 1}) if (v >= 0 && v < n) s.insert(v);
  for (int v = 2; v < n; v += stride) s.insert(v);
  return std::vector<int>(s.begin(), s.end());
}

// mask rows [mr0, mr1] x columns [mc0, mc1] (inclusive, as the tests state them) -> the rectangle gsm_set_static stores
static Rect grown(int H, int W, int mr0, int mr1, int mc0, int mc1) {
  return Rect{std::max(mr0 - 1, 0), std::min(mr1 + 2, H), std::max(mc0 - 1, 0), std::min(mc1 + 2, W)};
}

static void check_table(const char* name, int H, int W, int bw0, int bw1, int bws, int bh0, int bh1, int bhs, int rstride, int cstride, const Rect& own) {
  CHECK(table_ok(bh1, bw1), "%s: table_ok(%d, %d)", name, bh1, bw1);
  const Rect rects[] = {
      {0, H, 0, W},                                                  // the whole grid: nothing trimmed
      own,
      {0, H / 2, W / 4, 3 * W / 4}, {H / 2, H, W / 4, 3 * W / 4},    // touching the top / bottom grid edge
      {H / 4, 3 * H / 4, 0, W / 2}, {H / 4, 3 * H / 4, W / 2, W},    // touching the left / right grid edge
      {H / 2, H / 2 + 1, 0, W}, {0, H, W / 3, W / 3 + 1},            // one row high, one column wide
      {H / 2, H / 2 + 1, W / 2, W / 2 + 1}, {0, 1, 0, 1},            // a single cell: inside, at the corner
      {0, 0, 0, 0},                                                  // empty mask
  };
  const std::vector<int> rows = positions(H, rstride), cols = positions(W, cstride);
  const long before = g_t.windows;
  for (const Rect& q : rects)
    for (int bh = bh0; bh <= bh1; bh += bhs)
      for (int bw = bw0; bw <= bw1; bw += bws)
        for (int row : rows)
          for (int col : cols) check_window(H, W, row, col, bh, bw, q);
  printf("%-10s grid %3d x %3d, bw %3d-%3d, bh %2d-%2d, own rectangle [%d, %d) x [%d, %d): %ld windows\n", name, H, W, bw0, bw1, bh0, bh1, own.r0, own.r1,
         own.c0, own.c1, g_t.windows - before);
}

int main() {
  // the cases of tests/test_gpu_strip_trim.py: grid, widths, heights, the rectangle of the case's update mask
  check_table("regroup", 96, 100, 72, 90, 2, 50, 80, 10, 13, 14, grown(96, 100, 20, 75, 22, 77));
  check_table("deeper", 104, 72, 40, 62, 2, 64, 94, 10, 14, 11, grown(104, 72, 16, 87, 10, 61));
  check_table("l_shape", 96, 80, 64, 70, 2, 50, 80, 10, 13, 11, grown(96, 80, 18, 70, 0, 52));
  check_table("empty", 64, 64, 8, 16, 4, 8, 16, 4, 5, 5, grown(64, 64, 24, 39, 24, 39));
  check_table("tiny_8x10", 8, 10, 2, 4, 2, 2, 4, 2, 1, 1, grown(8, 10, 3, 4, 4, 6));
  // the headline problem: 256 x 256, blocks 50-80, update region H/8 .. 7H/8
  check_table("headline", 256, 256, 50, 80, 6, 50, 80, 10, 23, 29, grown(256, 256, 32, 223, 32, 223));

  printf("%ld windows: %ld untrimmed, %ld empty, trimmed at the top / bottom / left / right %ld / %ld / %ld / %ld; of the trimmed, %ld change the\n"
         "decomposition, %ld keep it with a smaller n, %ld interior, %ld at a grid border, deepest n %d; %ld windows clipped at the grid\n",
         g_t.windows, g_t.same, g_t.empty, g_t.top, g_t.bottom, g_t.left, g_t.right, g_t.regrouped, g_t.shallower, g_t.interior, g_t.clipped, g_t.deepest,
         g_t.grid_clipped);
  if (!g_t.same || !g_t.empty || !g_t.top || !g_t.bottom || !g_t.left || !g_t.right || !g_t.regrouped || !g_t.shallower || !g_t.interior || !g_t.clipped ||
      !g_t.grid_clipped || g_t.grid_clipped == g_t.windows) {
    printf("FAIL: a kind of window was not seen\n");
    return 1;
  }
  if (g_fail) { printf("%ld checks failed\n", g_fail); return 1; }
  printf("strip trim ok\n");
  return 0;
}
