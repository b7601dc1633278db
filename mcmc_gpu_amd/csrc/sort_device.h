// Segmented sort of fp64 fields on the device (qt_fit_kernel.hip, gsm.h: gsm_qt_fit): what does not depend on the machine -- the
// order-preserving key of a double, the merge-path partition search, and the tile / pass / chunk geometry of the sort.  The file
// compiles for the host too: tests/native/sort_device_check.cpp runs every function here lane by lane with g++.
//
// The sort: a workgroup sorts a tile of kSortTile keys in LDS (bitonic network), then ceil(log2(tiles)) merge passes double the length
// of the sorted runs of every field.  A pass merges the runs pairwise; its output is cut into chunks of kSortTile keys, one workgroup
// each, and the workgroup finds the part of either run that lands in its chunk by a merge-path search (Odeh, Green, Mwassi, Birk:
// Merge Path -- Parallel Merging Made Simple, 2012).  Keys only: equal keys are indistinguishable, so the sorted sequence is unique
// and depends on neither the network, the geometry nor the batch.
#pragma once
#include <cstdint>
#if !defined(__HIPCC__)
#define GSM_SORT_FN inline
#else
#define GSM_SORT_FN __host__ __device__ __forceinline__
#endif

namespace gsm {
namespace sortdev {

constexpr int kSortTile = 4096;          // keys per tile and per merge chunk: a power of two
constexpr int kSortThreads = 256;        // threads of a workgroup
constexpr int kSortRun = kSortTile / kSortThreads;      // consecutive keys a thread owns (register stages, sequential merge): 16
constexpr int kSortRunLog = 4;
static_assert((kSortTile & (kSortTile - 1)) == 0 && kSortTile <= 16384 && (1 << kSortRunLog) == kSortRun, "tile geometry");

// ---- keys: unsigned order == the order of the doubles, -inf < .. < -0 < +0 < .. < +inf < every NaN.  Every NaN (either sign, any
// payload) takes the one key kKeyNaN, which is above +inf's; no other double maps to it.
constexpr uint64_t kKeyNaN = ~uint64_t(0);
constexpr uint64_t kKeyNegInf = 0x000FFFFFFFFFFFFFull;      // the smallest key a double takes
constexpr uint64_t kKeyPosInf = 0xFFF0000000000000ull;      // the largest key of a value that is not NaN
GSM_SORT_FN uint64_t key_of_bits(uint64_t b) {
  if ((b & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull) return kKeyNaN;
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
// the bits of the double a key came from; kKeyNaN gives a quiet NaN
GSM_SORT_FN uint64_t bits_of_key(uint64_t k) {
  if (k == kKeyNaN) return 0x7FF8000000000000ull;
  return (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
}

// ---- merge path.  Two ascending runs A[0, na) and B[0, nb) merge into one of na + nb keys, A's key first among equal keys.  For an
// output position d in [0, na + nb] this returns a, the number of keys of A among the first d outputs (d - a come from B):
// the smallest a in [max(0, d - nb), min(d, na)] with a == min(d, na) or A(a) > B(d - 1 - a); A and B are callables that return
// the key at an index (a run in global memory, or in LDS behind lds_slot).  Monotone in d, so consecutive positions
// d0 <= d1 cut both runs into pieces [a0, a1) and [d0 - a0, d1 - a1) that tile them exactly once.
template <class GetA, class GetB>
GSM_SORT_FN int64_t merge_path(GetA A, int64_t na, GetB B, int64_t nb, int64_t d) {
  int64_t lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (A(mid) <= B(d - 1 - mid)) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the first index of the ascending run s[0, n) whose key is >= k (n if none)
template <class Key>
GSM_SORT_FN int64_t lower_bound(const Key* s, int64_t n, Key k) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (s[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// ---- geometry of a field of `cells` keys
GSM_SORT_FN int64_t sort_tiles(int64_t cells) { return (cells + kSortTile - 1) / kSortTile; }      // tiles == chunks of every pass
GSM_SORT_FN int sort_passes(int64_t cells) {                                                       // ceil(log2(tiles))
  int p = 0;
  for (int64_t t = sort_tiles(cells); (int64_t(1) << p) < t; ++p) {}
  return p;
}
// Chunk c of merge pass p (runs of kSortTile << p keys in, twice that out): the two runs it draws from, as offsets into the field,
// and the output positions [d0, d1) of their merge that it writes at field offset a_beg + d0.  nb == 0: a run without a partner, copied.
struct MergeChunk { int64_t a_beg, na, nb, d0, d1; };
GSM_SORT_FN MergeChunk merge_chunk(int64_t cells, int pass, int64_t c) {
  const int64_t L = int64_t(kSortTile) << pass, o0 = c * kSortTile;
  MergeChunk m;
  m.a_beg = o0 / (2 * L) * (2 * L);
  const int64_t a_end = m.a_beg + L < cells ? m.a_beg + L : cells, b_end = m.a_beg + 2 * L < cells ? m.a_beg + 2 * L : cells;
  m.na = a_end - m.a_beg; m.nb = b_end - a_end;
  m.d0 = o0 - m.a_beg;
  m.d1 = m.d0 + kSortTile < m.na + m.nb ? m.d0 + kSortTile : m.na + m.nb;
  return m;
}

// LDS index of key i of a tile: one slot of padding after every kSortRun keys, so that the lanes of a wavefront, each at its own
// run of kSortRun consecutive keys, fall on distinct banks (a stride of 17 eight-byte slots), and consecutive keys stay consecutive.
GSM_SORT_FN int lds_slot(int i) { return i + (i >> kSortRunLog); }
constexpr int kSortLdsSlots = kSortTile + kSortThreads;

// one compare-exchange of the bitonic network: ascending pair when `up`
template <class Key>
GSM_SORT_FN void compare_exchange(Key& a, Key& b, bool up) {
  const bool sw = up ? (a > b) : (a < b);
  const Key x = sw ? b : a, y = sw ? a : b;
  a = x; b = y;
}
// the low index of pair p of a stage with partner distance j (a power of two); the partner is that index | j
GSM_SORT_FN int bitonic_low(int p, int j) { return ((p & ~(j - 1)) << 1) | (p & (j - 1)); }

}  // namespace sortdev
}  // namespace gsm
