// Host check of the integer geometry of the strip kernels (mcmc_gpu_amd/csrc/strip_step.h): which lane of the 512-thread
// workgroup owns which cell of a step's window, which tile cells phase A writes, and the divisions without a divide.
// The helpers are __host__ __device__, so this program runs the code the kernels run; it calls no HIP runtime function.
//
// Per window, all 8 x 64 (wave, lane) pairs go through lane_setup with config(wh, ww) and the INTERIOR value make_window
// reports:
//   ownership    the cells row_own && kFColOwn, addressed cell0 + jj * W in uint32 as the kernels do, lie in [0, H * W), hit
//                every cell of the window exactly once and no other cell; fidx and tidx of an own cell are those of the
//                oracle's window_bounds (mr0, mc0: restated below, not taken from make_window)
//   tile writes  cell_written for jj = 0 .. n + 1 at tidx + jj * (bw + 2): inside the (bh + 2)(bw + 2) tile; window cells
//                exactly once; the non-corner cells of the halo ring that exist in the grid at least once (several row
//                strips write the same halo-column cell with the same bed value); ring cells outside the grid and every
//                other tile cell never (the four corners of the ring, which nobody reads, may be written when in the grid)
//   divisions    rows_per_strip == ceil, small_div == t / d, config == the table of decompositions restated below,
//                table_ok == "n <= kNR for every width up to bw, bw <= 496"
// It prints, per decomposition and INTERIOR value, how many windows it checked and the deepest n, and fails if a count is 0.
//
// The geometry every step kernel shares (mcmc_gpu_amd/csrc/step_common.h), on every window above plus all centres of a 12 x 12
// and a 9 x 14 grid with blocks 4 x 4, 6 x 10 and 12 x 12 (clipped on each edge, on two at once, as large as the grid):
//   window       clip_window (r0, r1, c0, c1, mr0, mc0, wh, ww), interior and halo_tile equal the oracle's window_bounds and the
//                halo slice of MCMC.py:1293-1297, restated below; dr, dc place the window inside the tile
//   tile width   halo_tile_width(W, col, bw) == the tile's tw
//   overlap      halo_touches(second, first) == "some cell of the second step's halo tile is a cell of the first step's window",
//                by brute force over all ordered pairs of windows of the two small grids
#include "strip_step.h"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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

// the decompositions, restated: upper window width, log2(lanes per strip), column groups, row strips
struct RefRow { int ww_max, cs, g, sr; };
static const RefRow kRef[6] = {{62, 6, 1, 8}, {70, 4, 5, 6}, {90, 5, 3, 5}, {124, 6, 2, 4}, {248, 6, 4, 2}, {496, 6, 8, 1}};
static int ref_index(int ww) { int i = 0; while (ww > kRef[i].ww_max) ++i; return i; }

struct Tally { long windows[6][2]; int deepest[6]; };
static Tally g_tally = {};

template <bool INTERIOR>
static void tile_writes(const Lane& L, int n, int ts, int tile_len, std::vector<uint8_t>& tcnt, std::vector<int>& ttouched) {
  const WriteMasks wm = write_masks(L);
  for (int jj = 0; jj <= n + 1; ++jj) {
    if (!cell_written<INTERIOR>(L, wm, jj)) continue;
    const long ti = (long)L.tidx + (long)jj * ts;
    CHECK(ti >= 0 && ti < tile_len, "tile index %ld of %d", ti, tile_len);
    if (ti < 0 || ti >= tile_len) continue;
    if (tcnt[ti]++ == 0) ttouched.push_back((int)ti);
  }
}

static std::vector<uint8_t> g_cnt, g_tcnt;
static std::vector<uint32_t> g_touched;
static std::vector<int> g_ttouched;

// the shared window and halo tile against the oracle's window_bounds (oracle/mcmc_oracle.py, MCMC.py:1266-1276; bh and bw
// even) and the halo slice max(0, r0 - 1) : min(H, r1 + 1) of MCMC.py:1293-1297, restated here
static gsm::step::Window check_step_window(int H, int W, int row, int col, int bh, int bw) {
  namespace st = gsm::step;
  const st::Window w = st::clip_window(H, W, row, col, bh, bw);
  const st::HaloTile t = st::halo_tile(H, W, w);
  const int r0 = std::max(0, row - bh / 2), r1 = std::min(H, row + bh / 2);
  const int c0 = std::max(0, col - bw / 2), c1 = std::min(W, col + bw / 2);
  const int mr0 = std::max(bh - r1, 0), mc0 = std::max(bw - c1, 0);
  CHECK(w.r0 == r0 && w.r1 == r1 && w.c0 == c0 && w.c1 == c1 && w.mr0 == mr0 && w.mc0 == mc0 && w.wh == r1 - r0 && w.ww == c1 - c0,
        "clip_window H %d W %d row %d col %d bh %d bw %d", H, W, row, col, bh, bw);
  CHECK(st::interior(H, W, w) == (r0 > 0 && r1 < H && c0 > 0 && c1 < W), "interior H %d W %d row %d col %d bh %d bw %d", H, W, row, col, bh, bw);
  const int hr0 = std::max(0, r0 - 1), hr1 = std::min(H, r1 + 1), hc0 = std::max(0, c0 - 1), hc1 = std::min(W, c1 + 1);
  CHECK(t.hr0 == hr0 && t.hr1 == hr1 && t.hc0 == hc0 && t.hc1 == hc1 && t.tw == hc1 - hc0 && t.ncell == (hr1 - hr0) * (hc1 - hc0) &&
            t.dr == r0 - hr0 && t.dc == c0 - hc0,
        "halo_tile H %d W %d row %d col %d bh %d bw %d", H, W, row, col, bh, bw);
  CHECK(st::halo_tile_width(W, col, bw) == t.tw, "halo_tile_width(%d, %d, %d) = %d, tile %d", W, col, bw, st::halo_tile_width(W, col, bw), t.tw);
  // the window's cells inside the tile and inside the field, as the kernels address them
  CHECK(st::in_window(w, t, t.dr, t.dc) && st::in_window(w, t, t.dr + w.wh - 1, t.dc + w.ww - 1) && !st::in_window(w, t, t.dr - 1, t.dc) &&
            !st::in_window(w, t, t.dr, t.dc - 1) && !st::in_window(w, t, t.dr + w.wh, t.dc) && !st::in_window(w, t, t.dr, t.dc + w.ww),
        "in_window H %d W %d row %d col %d bh %d bw %d", H, W, row, col, bh, bw);
  CHECK(st::field_index(w, t, t.dr, t.dc, bw) == mr0 * bw + mc0, "field_index H %d W %d row %d col %d bh %d bw %d", H, W, row, col, bh, bw);
  return w;
}

// every centre of a small grid with three block shapes; the overlap predicate over all ordered pairs of these windows
static void check_small_grid(int H, int W) {
  namespace st = gsm::step;
  const int shapes[3][2] = {{4, 4}, {6, 10}, {12, 12}};
  std::vector<st::Window> ws;
  for (const auto& sh : shapes)
    for (int row = 0; row < H; ++row)
      for (int col = 0; col < W; ++col) ws.push_back(check_step_window(H, W, row, col, sh[0], sh[1]));
  long touching = 0;
  for (const st::Window& first : ws) {
    for (const st::Window& second : ws) {
      const st::HaloTile t = st::halo_tile(H, W, second);
      bool brute = false;
      for (int r = t.hr0; r < t.hr1 && !brute; ++r)
        for (int c = t.hc0; c < t.hc1 && !brute; ++c) brute = r >= first.r0 && r < first.r1 && c >= first.c0 && c < first.c1;
      touching += brute;
      CHECK(st::halo_touches(second, first) == brute, "halo_touches: second [%d, %d) x [%d, %d), first [%d, %d) x [%d, %d) on %d x %d", second.r0,
            second.r1, second.c0, second.c1, first.r0, first.r1, first.c0, first.c1, H, W);
    }
    CHECK(!st::halo_touches(first, st::Window{}) || (first.r0 == 0 && first.c0 == 0), "an empty window touches [%d, %d) x [%d, %d)", first.r0, first.r1,
          first.c0, first.c1);
  }
  CHECK(touching > 0 && touching < (long)ws.size() * (long)ws.size(), "overlap pairs on %d x %d: %ld", H, W, touching);
  printf("shared     grid %3d x %3d: %zu windows, %zu ordered pairs, %ld touching\n", H, W, ws.size(), ws.size() * ws.size(), touching);
}

static void check_window(int H, int W, int row, int col, int bh, int bw) {
  check_step_window(H, W, row, col, bh, bw);
  const Window g = make_window(H, W, row, col, bh, bw);
  // the oracle's window_bounds (oracle/mcmc_oracle.py, MCMC.py:1266-1276), bh and bw even
  const int r0 = std::max(0, row - bh / 2), r1 = std::min(H, row + bh / 2);
  const int c0 = std::max(0, col - bw / 2), c1 = std::min(W, col + bw / 2);
  const int mr0 = std::max(bh - r1, 0), mc0 = std::max(bw - c1, 0);
  const int wh = r1 - r0, ww = c1 - c0;
  CHECK(g.r0 == r0 && g.c0 == c0 && g.wh == wh && g.ww == ww && g.mr0 == mr0 && g.mc0 == mc0 && g.bw == bw,
        "make_window H %d W %d row %d col %d bh %d bw %d", H, W, row, col, bh, bw);
  const bool interior = r0 > 0 && r1 < H && c0 > 0 && c1 < W;
  CHECK(g.interior == interior, "interior H %d W %d row %d col %d bh %d bw %d", H, W, row, col, bh, bw);
  const Cfg c = config(g.wh, g.ww);
  const int ri = ref_index(ww);
  CHECK(c.n <= kNR, "n %d at wh %d ww %d", c.n, wh, ww);
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
      if (has(L, kFColOwn)) {
        for (int jj = 1; jj <= kNR; ++jj) {
          if (!row_own(L, jj)) continue;
          const uint32_t idx = L.cell0 + (uint32_t)(jj * W);
          CHECK(idx < cells, "own cell %u of %u (wave %d lane %d jj %d)", idx, cells, wave, lane, jj);
          if (idx >= cells) continue;
          const int r = (int)(idx / (uint32_t)W), cc = (int)(idx % (uint32_t)W);
          CHECK(r >= r0 && r < r1 && cc >= c0 && cc < c1, "own cell (%d, %d) outside window [%d, %d) x [%d, %d)", r, cc, r0, r1, c0, c1);
          CHECK(L.fidx + jj * bw == (mr0 + r - r0) * bw + mc0 + cc - c0, "fidx of (%d, %d)", r, cc);
          CHECK(L.tidx + jj * ts == (mr0 + r - r0 + 1) * ts + mc0 + cc - c0 + 1, "tidx of (%d, %d)", r, cc);
          if (g_cnt[idx]++ == 0) g_touched.push_back(idx);
          CHECK(g_cnt[idx] == 1, "cell (%d, %d) owned %d times", r, cc, (int)g_cnt[idx]);
        }
      }
      if (g.interior) tile_writes<true>(L, c.n, ts, tile_len, g_tcnt, g_ttouched);
      else tile_writes<false>(L, c.n, ts, tile_len, g_tcnt, g_ttouched);
    }
  }
  // distinct cells, all inside the window, as many as the window has: a partition
  CHECK((long)g_touched.size() == (long)wh * ww, "%zu of %d window cells owned (H %d W %d row %d col %d bh %d bw %d)", g_touched.size(), wh * ww, H, W,
        row, col, bh, bw);
  for (uint32_t idx : g_touched) g_cnt[idx] = 0;

  long written = 0;
  for (int ty = 0; ty < bh + 2; ++ty) {
    for (int tx = 0; tx < bw + 2; ++tx) {
      const int k = g_tcnt[ty * ts + tx];
      written += k != 0;
      const int wy = ty - 1 - mr0, wx = tx - 1 - mc0;          // window coordinates of the tile cell
      const int r = r0 + wy, cc = c0 + wx;
      const bool in_window = wy >= 0 && wy < wh && wx >= 0 && wx < ww;
      const bool in_ring = !in_window && wy >= -1 && wy <= wh && wx >= -1 && wx <= ww;
      const bool corner = (wy == -1 || wy == wh) && (wx == -1 || wx == ww);
      const bool in_grid = r >= 0 && r < H && cc >= 0 && cc < W;
      if (in_window) CHECK(k == 1, "window cell (%d, %d) written %d times (H %d W %d row %d col %d bh %d bw %d)", r, cc, k, H, W, row, col, bh, bw);
      else if (in_ring && !in_grid) CHECK(k == 0, "ring cell (%d, %d) outside the grid written", r, cc);
      else if (in_ring && !corner) CHECK(k >= 1, "ring cell (%d, %d) not written (H %d W %d row %d col %d bh %d bw %d)", r, cc, H, W, row, col, bh, bw);
      else if (!in_ring) CHECK(k == 0, "tile cell (%d, %d) outside window and ring written", ty, tx);
    }
  }
  CHECK(written == (long)g_ttouched.size(), "tile bookkeeping");
  for (int ti : g_ttouched) g_tcnt[ti] = 0;

  ++g_tally.windows[ri][g.interior ? 1 : 0];
  if (c.n > g_tally.deepest[ri]) g_tally.deepest[ri] = c.n;
}

// rows / columns 0, 1, n - 2, n - 1 and every stride-th one from 2
static std::vector<int> positions(int n, int stride) {
  std::set<int> s;
  for (int v : {0, 1, n - 2, n - 1}) if (v >= 0 && v < n) s.insert(v);
  for (int v = 2; v < n; v += stride) s.insert(v);
  return std::vector<int>(s.begin(), s.end());
}

static void check_table(const char* name, int H, int W, int bw0, int bw1, int bh0, int bh1, int rstride, int cstride) {
  CHECK(table_ok(bh1, bw1), "%s: table_ok(%d, %d)", name, bh1, bw1);
  const std::vector<int> rows = positions(H, rstride), cols = positions(W, cstride);
  long n = 0;
  for (int bh = bh0; bh <= bh1; bh += 2)
    for (int bw = bw0; bw <= bw1; bw += 2)
      for (int row : rows)
        for (int col : cols) { check_window(H, W, row, col, bh, bw); ++n; }
  printf("%-10s grid %3d x %3d, bw %3d-%3d, bh %2d-%2d: %ld windows\n", name, H, W, bw0, bw1, bh0, bh1, n);
}

static void check_divisions() {
  const int srs[6] = {8, 6, 5, 4, 2, 1};
  for (int sr : srs)
    for (int wh = 1; wh <= 8191; ++wh) CHECK(rows_per_strip(wh, sr) == (wh + sr - 1) / sr, "rows_per_strip(%d, %d) = %d", wh, sr, rows_per_strip(wh, sr));
  for (int t = 0; t < 64; ++t)
    for (int d = 1; d <= 8; ++d) CHECK(small_div(t, d) == t / d, "small_div(%d, %d) = %d", t, d, small_div(t, d));
  for (int ww = 1; ww <= 496; ++ww) {
    const RefRow& e = kRef[ref_index(ww)];
    CHECK(8 * (64 >> e.cs) >= e.g * e.sr, "more strips than the workgroup has at ww %d", ww);
    CHECK(e.g * ((1 << e.cs) - 2) >= ww, "column groups do not span ww %d", ww);
    for (int wh = 1; wh <= 8191; ++wh) {
      const Cfg c = config(wh, ww);
      CHECK(c.cs == e.cs && c.g == e.g && c.sr == e.sr && c.n == (wh + e.sr - 1) / e.sr, "config(%d, %d) = (%d, %d, %d, %d)", wh, ww, c.cs, c.g, c.sr, c.n);
    }
  }
  for (int bh = 1; bh <= 160; ++bh) {
    bool ok = true;                                            // n <= kNR for every width up to bw, by the restated table
    for (int bw = 1; bw <= 520; ++bw) {
      if (bw <= 496) ok = ok && (bh + kRef[ref_index(bw)].sr - 1) / kRef[ref_index(bw)].sr <= kNR;
      CHECK(table_ok(bh, bw) == (ok && bw <= 496), "table_ok(%d, %d) = %d", bh, bw, (int)table_ok(bh, bw));
    }
  }
}

int main() {
  check_divisions();
  // the tables of tests/strip_oracle_cases.py, every even width and height
  check_table("strip_g1", 104, 72, 40, 62, 64, 94, 5, 7);
  check_table("strip_l16", 96, 80, 64, 70, 50, 80, 5, 7);
  check_table("strip_l32", 96, 100, 72, 90, 50, 80, 5, 7);
  check_table("strip_g2", 60, 136, 92, 124, 18, 48, 5, 7);
  check_table("strip_g4", 44, 140, 126, 128, 8, 32, 3, 3);
  // the grids of tests/test_gpu_parity.py with their block sizes
  check_table("parity_64", 64, 64, 8, 16, 8, 16, 2, 2);
  check_table("tiny_8x10", 8, 10, 2, 4, 2, 4, 1, 1);
  check_small_grid(12, 12);
  check_small_grid(9, 14);

  bool empty = false;
  for (int i = 0; i < 5; ++i) {                                // the sixth (g = 8) is out of reach: block widths stop at 128
    printf("decomposition g %d x sr %d (%2d lanes): %8ld clipped windows, %7ld interior, deepest n %2d\n", kRef[i].g, kRef[i].sr, 1 << kRef[i].cs,
           g_tally.windows[i][0], g_tally.windows[i][1], g_tally.deepest[i]);
    empty = empty || g_tally.windows[i][0] == 0 || g_tally.windows[i][1] == 0;
  }
  if (empty) { printf("FAIL: a decomposition was not seen with both INTERIOR values\n"); return 1; }
  if (g_fail) { printf("%ld checks failed\n", g_fail); return 1; }
  printf("strip geometry ok\n");
  return 0;
}
