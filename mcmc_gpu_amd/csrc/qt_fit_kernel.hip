// Fit of the normal-score transformers of a stack of fields on gfx950 (gsm.h: gsm_qt_fit): per field the table quantiles_ of
// scikit-learn's QuantileTransformer(n_quantiles, subsample=None).fit on one feature -- a sort of the field and nq interpolated order
// statistics of its values that are not NaN.
//
// Replaces, for a stack of beds:
//   nst_trans = QuantileTransformer(n_quantiles=1000, output_distribution="normal", subsample=None, random_state=rng_seed).fit(data)
//   (smallScaleChain_multiprocessing.py:493-494; sklearn/preprocessing/_data.py QuantileTransformer._dense_fit:
//   np.nanpercentile(col, references * 100) then np.maximum.accumulate; numpy/lib/_function_base_impl.py _quantile, _lerp)
//
// Three steps, every field on its own (sort_device.h has the keys, the partition search and the geometry):
//   1. qt_tile_sort_kernel    a workgroup reads a tile of 4096 doubles, maps them to order-preserving 64-bit keys (NaN last) and sorts
//                             them in LDS by a bitonic network; the input is only read
//   2. qt_merge_kernel        ceil(log2(tiles)) passes between the handle's two key buffers; a workgroup writes 4096 consecutive keys
//                             of the merge of two runs, cut out by two merge-path searches
//   3. qt_quantile_kernel     a workgroup per field: the number m of keys below NaN's and the counts of +-inf by binary search in the
//                             sorted keys, then t[k] and its running maximum for k < nq
// Keys carry no payload, so the sorted keys are the unique ascending arrangement of the field's values: nothing of the result depends
// on the tiling, the batch, the launch geometry or the lane.  No atomics.
#include "gsm_internal.h"
#include "sort_device.h"

namespace gsm {

using namespace sortdev;

// the stages with partner distance below kSortRun of the merge step k, on the kSortRun consecutive keys [base, base + kSortRun) a thread holds
__device__ __forceinline__ void qt_register_stages(uint64_t (&v)[kSortRun], int base, int k) {
#pragma unroll
  for (int j = kSortRun / 2; j >= 1; j >>= 1) {
    if (j < k) {
#pragma unroll
      for (int p = 0; p < kSortRun / 2; ++p) {
        const int i = bitonic_low(p, j);
        compare_exchange(v[i], v[i | j], ((base + i) & k) == 0);
      }
    }
  }
}

// ---- step 1.  Thread t owns keys 16 t .. 16 t + 15 of the tile in the stages whose partner distance is below 16 (registers); the
// other stages run on LDS, thread t at pairs t, t + 256, ..: consecutive lanes at consecutive keys.  LDS index through lds_slot
// (a pad slot after every 16 keys): a thread's own 16 keys are read and written at a lane stride of 17 slots, conflict-free.
// A ragged last tile is filled up with kKeyNaN, the largest key, and only the field's own cells are written back.
__global__ __launch_bounds__(kSortThreads) void qt_tile_sort_kernel(const double* __restrict__ x, uint64_t* __restrict__ keys, int64_t cells,
                                                                    int64_t tiles) {
  __shared__ uint64_t lds[kSortLdsSlots];
  const int tid = threadIdx.x;
  const int64_t field = blockIdx.x / tiles, base = (int64_t)(blockIdx.x % tiles) * kSortTile;
  const int cnt = (int)(cells - base < kSortTile ? cells - base : kSortTile);
  const uint64_t* xb = reinterpret_cast<const uint64_t*>(x) + field * cells + base;
#pragma unroll
  for (int e = 0; e < kSortRun; ++e) {
    const int i = tid + e * kSortThreads;
    lds[lds_slot(i)] = i < cnt ? key_of_bits(xb[i]) : kKeyNaN;
  }
  __syncthreads();
  uint64_t v[kSortRun];
  const int own = tid * kSortRun, own_slot = lds_slot(own);
#pragma unroll
  for (int r = 0; r < kSortRun; ++r) v[r] = lds[own_slot + r];
#pragma unroll
  for (int k = 2; k <= kSortRun; k <<= 1) qt_register_stages(v, own, k);
  for (int k = 2 * kSortRun; k <= kSortTile; k <<= 1) {
#pragma unroll
    for (int r = 0; r < kSortRun; ++r) lds[own_slot + r] = v[r];
    __syncthreads();
    for (int j = k >> 1; j >= kSortRun; j >>= 1) {
#pragma unroll
      for (int e = 0; e < kSortRun / 2; ++e) {
        const int i = bitonic_low(tid + e * kSortThreads, j), l = i | j;
        uint64_t a = lds[lds_slot(i)], b = lds[lds_slot(l)];
        compare_exchange(a, b, (i & k) == 0);
        lds[lds_slot(i)] = a; lds[lds_slot(l)] = b;
      }
      __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < kSortRun; ++r) v[r] = lds[own_slot + r];
    qt_register_stages(v, own, k);
  }
#pragma unroll
  for (int r = 0; r < kSortRun; ++r) lds[own_slot + r] = v[r];          // a thread's own slots: nobody else reads them before the barrier
  __syncthreads();
  uint64_t* kb = keys + field * cells + base;
#pragma unroll
  for (int e = 0; e < kSortRun; ++e) {
    const int i = tid + e * kSortThreads;
    if (i < cnt) kb[i] = lds[lds_slot(i)];
  }
}

// ---- step 2, one pass.  Chunk c of a field (sort_device.h: merge_chunk) is the output positions [d0, d1) of the merge of runs A
// and B.  Two threads search the runs in global memory for the cuts at d0 and d1; the pieces [a0, a1) of A and [b0, b1) of B, d1 - d0
// keys together, go to LDS; thread t cuts them again at output 16 t (a search in LDS) and merges its 16 outputs in registers, A's
// key first among equals; the outputs return through LDS so that the global writes are coalesced.  A run without a partner is copied.
__global__ __launch_bounds__(kSortThreads) void qt_merge_kernel(const uint64_t* __restrict__ in, uint64_t* __restrict__ out, int64_t cells,
                                                                int64_t tiles, int pass) {
  __shared__ uint64_t lds[kSortLdsSlots];
  __shared__ int64_t cut[2];
  const int tid = threadIdx.x;
  const int64_t field = blockIdx.x / tiles;
  const MergeChunk m = merge_chunk(cells, pass, (int64_t)(blockIdx.x % tiles));
  const uint64_t* A = in + field * cells + m.a_beg;
  const uint64_t* B = A + m.na;
  uint64_t* dst = out + field * cells + m.a_beg + m.d0;
  const int total = (int)(m.d1 - m.d0);
  if (m.nb == 0) {
    for (int i = tid; i < total; i += kSortThreads) dst[i] = A[m.d0 + i];
    return;
  }
  auto ga = [A](int64_t i) { return A[i]; };
  auto gb = [B](int64_t i) { return B[i]; };
  if (tid == 0) cut[0] = merge_path(ga, m.na, gb, m.nb, m.d0);
  if (tid == 64) cut[1] = merge_path(ga, m.na, gb, m.nb, m.d1);
  __syncthreads();
  const int64_t a0 = cut[0], b0 = m.d0 - a0;
  const int la = (int)(cut[1] - a0), lb = total - la;
  for (int i = tid; i < total; i += kSortThreads) lds[lds_slot(i)] = i < la ? A[a0 + i] : B[b0 + (i - la)];
  __syncthreads();
  const uint64_t* l = lds;
  auto la_at = [l](int64_t i) { return l[lds_slot((int)i)]; };
  auto lb_at = [l, la](int64_t i) { return l[lds_slot(la + (int)i)]; };
  const int diag = tid * kSortRun < total ? tid * kSortRun : total;
  int ia = (int)merge_path(la_at, la, lb_at, lb, diag), ib = diag - ia;
  uint64_t ka = ia < la ? la_at(ia) : kKeyNaN, kb = ib < lb ? lb_at(ib) : kKeyNaN;
  uint64_t o[kSortRun];
#pragma unroll
  for (int s = 0; s < kSortRun; ++s) {                  // outputs past `total` repeat a key and are not written
    const bool take_a = ib >= lb || (ia < la && ka <= kb);
    o[s] = take_a ? ka : kb;
    if (take_a) { ++ia; ka = ia < la ? la_at(ia) : kKeyNaN; }
    else { ++ib; kb = ib < lb ? lb_at(ib) : kKeyNaN; }
  }
  __syncthreads();                                      // the inputs have been read: their LDS takes the outputs
  const int own_slot = lds_slot(tid * kSortRun);
#pragma unroll
  for (int s = 0; s < kSortRun; ++s) lds[own_slot + s] = o[s];
  __syncthreads();
  for (int i = tid; i < total; i += kSortThreads) dst[i] = lds[lds_slot(i)];
}

// the sorted values of every field from its sorted keys: the values that are not NaN ascending, then NaN up to `cells`
__global__ __launch_bounds__(256) void qt_values_kernel(const uint64_t* __restrict__ keys, double* __restrict__ sorted, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < total) reinterpret_cast<uint64_t*>(sorted)[i] = bits_of_key(keys[i]);
}

// np.maximum of two doubles: NaN from either side stays
__device__ __forceinline__ double qt_np_maximum(double a, double b) { return (a >= b || a != a) ? a : b; }

// ---- step 3.  With s the field's sorted values that are not NaN, m of them:
//   v = (m - 1) * q[k];  lo = floor(v);  g = v - lo;  hi = min(lo + 1, m - 1);  a = s[lo];  b = s[hi];  d = b - a
//   t[k] = g >= 0.5 ? b - d * (1 - g) : a + d * g;      quantiles[k] = np.maximum.accumulate(t)[k]
// every operation rounded on its own (the library is built with -ffp-contract=off).  The running maximum is a scan over k: chunks
// of 256 entries, a Hillis-Steele scan in LDS within a chunk, the carry from chunk to chunk; -inf is a left identity of np.maximum.
// m == 0: a row of NaN.
__global__ __launch_bounds__(256) void qt_quantile_kernel(const uint64_t* __restrict__ keys, int64_t cells, const double* __restrict__ q, int nq,
                                                          double* __restrict__ quantiles, int64_t* __restrict__ n_valid,
                                                          int64_t* __restrict__ n_inf) {
  __shared__ double scan[2][256];
  const int tid = threadIdx.x;
  const int64_t field = blockIdx.x;
  const uint64_t* s = keys + field * cells;
  const int64_t m = lower_bound(s, cells, kKeyNaN);
  if (tid == 0) {
    n_valid[field] = m;
    n_inf[field] = lower_bound(s, m, kKeyNegInf + 1) + (m - lower_bound(s, m, kKeyPosInf));
  }
  double* qr = quantiles + field * (int64_t)nq;
  if (m == 0) {
    for (int k = tid; k < nq; k += 256) qr[k] = __longlong_as_double(0x7FF8000000000000ll);
    return;
  }
  double carry = -HUGE_VAL;
  for (int k0 = 0; k0 < nq; k0 += 256) {
    const int k = k0 + tid;
    double t = -HUGE_VAL;
    if (k < nq) {
      const double v = (double)(m - 1) * q[k];
      const double fl = floor(v), g = v - fl;
      const int64_t lo = (int64_t)fl, hi = lo + 1 < m - 1 ? lo + 1 : m - 1;
      const double a = __longlong_as_double((long long)bits_of_key(s[lo])), b = __longlong_as_double((long long)bits_of_key(s[hi]));
      const double d = b - a;
      t = g >= 0.5 ? b - d * (1.0 - g) : a + d * g;
    }
    int cur = 0;
    scan[0][tid] = t;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
      const double mine = scan[cur][tid];
      scan[cur ^ 1][tid] = tid >= off ? qt_np_maximum(scan[cur][tid - off], mine) : mine;
      cur ^= 1;
      __syncthreads();
    }
    const double incl = qt_np_maximum(carry, scan[cur][tid]);
    if (k < nq) qr[k] = incl;
    carry = qt_np_maximum(carry, scan[cur][255 < nq - 1 - k0 ? 255 : nq - 1 - k0]);
    __syncthreads();                                    // scan[] is written again by the next chunk
  }
}

hipError_t launch_qt_fit(const double* x, int n, int64_t cells, const double* q, int nq, uint64_t* keys0, uint64_t* keys1, double* quantiles,
                         int64_t* n_valid, int64_t* n_inf, double* sorted, hipStream_t st) {
  const int64_t tiles = sort_tiles(cells), blocks = (int64_t)n * tiles, total = (int64_t)n * cells;
  if (blocks > INT32_MAX || (total + 255) / 256 > INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(qt_tile_sort_kernel, dim3((unsigned)blocks), dim3(kSortThreads), 0, st, x, keys0, cells, tiles);
  uint64_t* buf[2] = {keys0, keys1};
  const int passes = sort_passes(cells);
  for (int p = 0; p < passes; ++p)
    hipLaunchKernelGGL(qt_merge_kernel, dim3((unsigned)blocks), dim3(kSortThreads), 0, st, buf[p & 1], buf[(p & 1) ^ 1], cells, tiles, p);
  const uint64_t* fin = buf[passes & 1];
  hipLaunchKernelGGL(qt_quantile_kernel, dim3((unsigned)n), dim3(256), 0, st, fin, cells, q, nq, quantiles, n_valid, n_inf);
  if (sorted) hipLaunchKernelGGL(qt_values_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, fin, sorted, total);
  return hipGetLastError();
}

}  // namespace gsm
