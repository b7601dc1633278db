// Host check of mcmc_gpu_amd/csrc/sort_device.h (tests/test_qt_fit_host.py compiles and runs it with g++; no GPU, no HIP runtime):
//   1. key_of_bits on every special value: unsigned key order == the order of the doubles, -0 below +0, every NaN (either sign, quiet
//      or signalling, any payload) on the one key above +inf's, and bits_of_key gives the bits back;
//   2. merge_path over every pair of run lengths 0 .. 9 on runs with ties: at every output position the cut is the stable merge's (A's
//      key first among equals), and the cuts at consecutive positions tile both runs exactly once;
//   3. merge_chunk / sort_tiles / sort_passes at sizes round every tile boundary: the chunks of every pass tile the field exactly once,
//      and the passes played on the host -- a tile sort by the bitonic network as the kernel walks it (bitonic_low, compare_exchange,
//      lds_slot; thread by thread, stage by stage), then every chunk merged from its two merge_path cuts, thread by thread -- sort it;
//   4. lower_bound against a linear scan.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "sort_device.h"

using namespace gsm::sortdev;

static int failures = 0;
#define CHECK(cond, ...)                                     \
  do {                                                       \
    if (!(cond)) {                                           \
      if (++failures <= 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                        \
  } while (0)

static uint64_t bits(double x) { uint64_t b; std::memcpy(&b, &x, 8); return b; }
static double dbl(uint64_t b) { double x; std::memcpy(&x, &b, 8); return x; }

static void check_keys() {
  const double inf = std::numeric_limits<double>::infinity(), mx = std::numeric_limits<double>::max(), mn = std::numeric_limits<double>::min(),
               sub = std::numeric_limits<double>::denorm_min();
  // strictly ascending as doubles, except that -0 == +0 compare equal and must still be ordered -0 first
  const double asc[] = {-inf, -mx, -1e300, -2.0, -1.0 - 2.220446049250313e-16, -1.0, -0.5, -mn, -mn / 2, -2 * sub, -sub, -0.0, 0.0,
                        sub, 2 * sub, mn / 2, mn, 0.5, 1.0, 1.0 + 2.220446049250313e-16, 2.0, 1e300, mx, inf};
  const int n = (int)(sizeof(asc) / sizeof(asc[0]));
  for (int i = 0; i < n; ++i) {
    const uint64_t k = key_of_bits(bits(asc[i]));
    CHECK(bits_of_key(k) == bits(asc[i]), "round trip of %g", asc[i]);
    CHECK(k != kKeyNaN, "%g takes NaN's key", asc[i]);
    if (i) CHECK(key_of_bits(bits(asc[i - 1])) < k, "keys of %g and %g out of order", asc[i - 1], asc[i]);
  }
  CHECK(key_of_bits(bits(-inf)) == kKeyNegInf && key_of_bits(bits(inf)) == kKeyPosInf, "the keys of the infinities");
  const uint64_t nans[] = {0x7FF8000000000000ull, 0xFFF8000000000000ull, 0x7FF0000000000001ull, 0xFFF0000000000001ull, 0x7FFFFFFFFFFFFFFFull,
                           0xFFFFFFFFFFFFFFFFull, 0x7FF4000000000000ull, bits(std::nan("")), bits(-std::nan(""))};
  for (uint64_t b : nans) {
    CHECK(std::isnan(dbl(b)), "test value %llx is not a NaN", (unsigned long long)b);
    CHECK(key_of_bits(b) == kKeyNaN, "NaN %llx not on NaN's key", (unsigned long long)b);
  }
  CHECK(kKeyNaN > kKeyPosInf, "NaN must sort after +inf");
  CHECK(std::isnan(dbl(bits_of_key(kKeyNaN))), "NaN's key must give a NaN");
  // order against random doubles of every exponent
  std::mt19937_64 g(11);
  for (int t = 0; t < 200000; ++t) {
    const uint64_t a = g(), b = g();
    const double x = dbl(a), y = dbl(b);
    if (std::isnan(x) || std::isnan(y)) continue;
    const uint64_t ka = key_of_bits(a), kb = key_of_bits(b);
    if (x < y) CHECK(ka < kb, "order of %a %a", x, y);
    if (x > y) CHECK(ka > kb, "order of %a %a", x, y);
    CHECK(bits_of_key(ka) == a, "round trip of %a", x);
  }
}

// the stable merge (A first among equals) of two runs tagged by origin
static void check_merge_path() {
  for (int na = 0; na <= 9; ++na)
    for (int nb = 0; nb <= 9; ++nb)
      for (int variant = 0; variant < 6; ++variant) {
        std::vector<uint64_t> A(na), B(nb);
        std::mt19937 g(100 * na + 10 * nb + variant);
        // variant 0: all equal; 1: A below B; 2: B below A; 3..5: few distinct values (many ties)
        for (auto& v : A) v = variant == 0 ? 5 : variant == 1 ? g() % 3 : variant == 2 ? 10 + g() % 3 : g() % (variant - 1);
        for (auto& v : B) v = variant == 0 ? 5 : variant == 1 ? 10 + g() % 3 : variant == 2 ? g() % 3 : g() % (variant - 1);
        std::sort(A.begin(), A.end()); std::sort(B.begin(), B.end());
        // reference: how many keys of A are among the first d outputs of the stable merge
        std::vector<int> from_a(na + nb + 1, 0);
        std::vector<uint64_t> merged;
        { int i = 0, j = 0;
          for (int d = 0; d < na + nb; ++d) {
            const bool ta = j >= nb || (i < na && A[i] <= B[j]);
            merged.push_back(ta ? A[i] : B[j]);
            ta ? ++i : ++j;
            from_a[d + 1] = i;
          } }
        auto ga = [&](int64_t i) { return A[(size_t)i]; };
        auto gb = [&](int64_t i) { return B[(size_t)i]; };
        std::vector<int> hit_a(na, 0), hit_b(nb, 0);
        int64_t prev = 0;
        for (int d = 0; d <= na + nb; ++d) {
          const int64_t a = merge_path(ga, na, gb, nb, d);
          CHECK(a == from_a[d], "merge_path(na=%d, nb=%d, variant %d, d=%d) = %lld, stable merge takes %d", na, nb, variant, d, (long long)a, from_a[d]);
          CHECK(a >= 0 && a <= na && d - a >= 0 && d - a <= nb, "cut outside the runs");
          if (d) {
            CHECK(a >= prev && (d - a) >= (d - 1 - prev), "cuts not monotone");
            for (int64_t i = prev; i < a; ++i) ++hit_a[(size_t)i];
            for (int64_t j = d - 1 - prev; j < d - a; ++j) ++hit_b[(size_t)j];
          }
          prev = a;
        }
        for (int v : hit_a) CHECK(v == 1, "a key of A covered %d times", v);
        for (int v : hit_b) CHECK(v == 1, "a key of B covered %d times", v);
      }
}

// the tile sort as qt_tile_sort_kernel walks it, on one tile of keys in `lds` (indexed through lds_slot)
static void host_tile_sort(std::vector<uint64_t>& lds) {
  auto reg_stages = [&](int tid, int k) {
    const int base = tid * kSortRun, slot = lds_slot(base);
    for (int j = kSortRun / 2; j >= 1; j >>= 1)
      if (j < k)
        for (int p = 0; p < kSortRun / 2; ++p) {
          const int i = bitonic_low(p, j);
          compare_exchange(lds[slot + i], lds[slot + (i | j)], ((base + i) & k) == 0);
        }
  };
  for (int k = 2; k <= kSortRun; k <<= 1)
    for (int tid = 0; tid < kSortThreads; ++tid) reg_stages(tid, k);
  for (int k = 2 * kSortRun; k <= kSortTile; k <<= 1) {
    for (int j = k >> 1; j >= kSortRun; j >>= 1)
      for (int tid = 0; tid < kSortThreads; ++tid)
        for (int e = 0; e < kSortRun / 2; ++e) {
          const int i = bitonic_low(tid + e * kSortThreads, j), l = i | j;
          compare_exchange(lds[lds_slot(i)], lds[lds_slot(l)], (i & k) == 0);
        }
    for (int tid = 0; tid < kSortThreads; ++tid) reg_stages(tid, k);
  }
}

static void host_sort(std::vector<uint64_t>& keys) {
  const int64_t cells = (int64_t)keys.size(), tiles = sort_tiles(cells);
  std::vector<uint64_t> other(keys.size());
  for (int64_t t = 0; t < tiles; ++t) {
    std::vector<uint64_t> lds(kSortLdsSlots, 0);
    const int64_t base = t * kSortTile;
    const int cnt = (int)std::min<int64_t>(kSortTile, cells - base);
    for (int i = 0; i < kSortTile; ++i) lds[lds_slot(i)] = i < cnt ? keys[(size_t)(base + i)] : kKeyNaN;
    host_tile_sort(lds);
    for (int i = 0; i < cnt; ++i) keys[(size_t)(base + i)] = lds[lds_slot(i)];
  }
  const int passes = sort_passes(cells);
  CHECK((tiles <= 1 && passes == 0) || ((int64_t(1) << passes) >= tiles && (int64_t(1) << (passes - 1)) < tiles), "sort_passes(%lld) = %d", (long long)cells, passes);
  std::vector<uint64_t>* in = &keys; std::vector<uint64_t>* out = &other;
  for (int p = 0; p < passes; ++p) {
    std::vector<int> written(keys.size(), 0);
    for (int64_t c = 0; c < tiles; ++c) {
      const MergeChunk m = merge_chunk(cells, p, c);
      CHECK(m.a_beg >= 0 && m.na >= 1 && m.nb >= 0 && m.a_beg + m.na + m.nb <= cells && m.d0 >= 0 && m.d0 < m.d1 && m.d1 <= m.na + m.nb &&
            m.d1 - m.d0 <= kSortTile && m.a_beg + m.d0 == c * kSortTile, "chunk %lld of pass %d at %lld cells", (long long)c, p, (long long)cells);
      const uint64_t* A = in->data() + m.a_beg; const uint64_t* B = A + m.na;
      uint64_t* dst = out->data() + m.a_beg + m.d0;
      const int total = (int)(m.d1 - m.d0);
      for (int i = 0; i < total; ++i) ++written[(size_t)(m.a_beg + m.d0 + i)];
      if (m.nb == 0) { for (int i = 0; i < total; ++i) dst[i] = A[m.d0 + i]; continue; }
      auto ga = [A](int64_t i) { return A[i]; };
      auto gb = [B](int64_t i) { return B[i]; };
      const int64_t a0 = merge_path(ga, m.na, gb, m.nb, m.d0), a1 = merge_path(ga, m.na, gb, m.nb, m.d1), b0 = m.d0 - a0;
      const int la = (int)(a1 - a0), lb = total - la;
      std::vector<uint64_t> lds(kSortLdsSlots, 0), o(kSortLdsSlots, 0);
      for (int i = 0; i < total; ++i) lds[lds_slot(i)] = i < la ? A[a0 + i] : B[b0 + (i - la)];
      auto la_at = [&](int64_t i) { return lds[(size_t)lds_slot((int)i)]; };
      auto lb_at = [&](int64_t i) { return lds[(size_t)lds_slot(la + (int)i)]; };
      for (int tid = 0; tid < kSortThreads; ++tid) {
        const int diag = std::min(tid * kSortRun, total);
        int ia = (int)merge_path(la_at, la, lb_at, lb, diag), ib = diag - ia;
        for (int s = 0; s < kSortRun && diag + s < total; ++s) {
          const bool ta = ib >= lb || (ia < la && la_at(ia) <= lb_at(ib));
          o[(size_t)lds_slot(tid * kSortRun + s)] = ta ? la_at(ia) : lb_at(ib);
          ta ? ++ia : ++ib;
        }
      }
      for (int i = 0; i < total; ++i) dst[i] = o[(size_t)lds_slot(i)];
    }
    for (size_t i = 0; i < written.size(); ++i) CHECK(written[i] == 1, "pass %d at %lld cells: key %zu written %d times", p, (long long)cells, i, written[i]);
    std::swap(in, out);
  }
  if (in != &keys) keys = *in;
}

static void check_sort() {
  const int T = kSortTile;
  const int sizes[] = {1, 2, 3, 17, 255, 256, 257, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 3 * T, 4 * T + 1, 5 * T + 7, 8 * T - 1, 100 * 130};
  int which = 0;
  for (int n : sizes) {
    std::mt19937_64 g(n);
    std::vector<uint64_t> keys((size_t)n);
    for (auto& k : keys) {
      switch (which % 4) {
        case 0: k = key_of_bits(g()); break;                                   // any bits, NaNs among them
        case 1: k = key_of_bits(bits((double)(int)(g() % 7) - 3.0)); break;    // seven values, zero among them: ties
        case 2: k = key_of_bits(bits((g() % 5 == 0) ? std::nan("") : (double)(g() % 1000) * 0.1)); break;
        default: k = g() % 3; break;
      }
    }
    ++which;
    std::vector<uint64_t> want = keys;
    std::sort(want.begin(), want.end());
    host_sort(keys);
    CHECK(keys == want, "host play of the sort at %d keys", n);
    for (uint64_t probe : {uint64_t(0), uint64_t(1), want[want.size() / 2], kKeyPosInf, kKeyNaN}) {
      int64_t lin = 0;
      while (lin < n && want[(size_t)lin] < probe) ++lin;
      CHECK(lower_bound(want.data(), (int64_t)n, probe) == lin, "lower_bound at %d keys", n);
    }
  }
  CHECK(sort_tiles(1) == 1 && sort_tiles(T) == 1 && sort_tiles(T + 1) == 2 && sort_passes(T) == 0 && sort_passes(T + 1) == 1 &&
        sort_passes(2 * T + 1) == 2 && sort_passes(int64_t(1) << 24) == 24 - 12, "tile and pass counts");
  for (int i = 0; i < kSortTile; ++i) CHECK(lds_slot(i) < kSortLdsSlots && (i == 0 || lds_slot(i) > lds_slot(i - 1)), "lds_slot(%d)", i);
}

int main() {
  check_keys();
  check_merge_path();
  check_sort();
  if (failures) { std::printf("%d failures\n", failures); return 1; }
  std::printf("sort device ok\n");
  return 0;
}
