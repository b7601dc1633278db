// Posterior accumulator: running moments of every chain's bed over a thinned set of iterations, and their reduction over
// chains (include/gsm.h, gsm_posterior_*).  The reference keeps whole-bed caches on the host instead (bed_cache and
// sample_values of chain_crf.run, MCMC.py:1174-1198, :1362-1366).
//
// All kernels here are streams without reuse: no LDS, no atomics, 16 bytes per lane and load where the layout allows it,
// consecutive lanes on consecutive addresses, every load of a loop trip issued before the first use.  Sums over chains are
// taken in index order; where the chain axis is split over workgroups to fill the machine, each part writes its own slab
// and a second kernel adds the slabs in part order, so results do not depend on scheduling.
#include "posterior_device.h"

namespace gsm {
namespace {

constexpr int kPostUnroll = 2;     // 16-byte groups per lane and loop trip of the per-chain accumulate
constexpr int kPostChains = 4;     // chains whose loads are in flight together in the pooled form

// ---- per-chain form --------------------------------------------------------------------------------------------------
// d = bed - ref; s1 += d; s2 += d * d over the flat [n_chains * H * W] arrays.  kFirst: ref = bed is written instead of
// read and the accumulators are set to d = bed - bed (0, or NaN where the bed is not finite) and d * d.
template <typename T, int V, bool kFirst>
__global__ __launch_bounds__(kPostBlock) void post_accumulate_kernel(const T* __restrict__ beds, T* __restrict__ ref,
                                                                     double* __restrict__ s1, double* __restrict__ s2, int64_t n) {
  using PT = Pack<T, V>;
  using PD = Pack<double, 2>;
  constexpr int kD = V / 2;                       // 16-byte packs of doubles per group
  const int64_t n_groups = n / V;
  const int64_t trip = (int64_t)kPostBlock * kPostUnroll;
  for (int64_t base = (int64_t)blockIdx.x * trip; base < n_groups; base += (int64_t)gridDim.x * trip) {
    PT b[kPostUnroll], r[kPostUnroll];
    PD a1[kPostUnroll][kD], a2[kPostUnroll][kD];
    bool live[kPostUnroll];
#pragma unroll
    for (int u = 0; u < kPostUnroll; ++u) {
      const int64_t gidx = base + (int64_t)u * kPostBlock + threadIdx.x;
      live[u] = gidx < n_groups;
      if (live[u]) {
        b[u] = *reinterpret_cast<const PT*>(beds + gidx * V);
        if (!kFirst) {
          r[u] = *reinterpret_cast<const PT*>(ref + gidx * V);
#pragma unroll
          for (int k = 0; k < kD; ++k) {
            a1[u][k] = *reinterpret_cast<const PD*>(s1 + gidx * V + 2 * k);
            a2[u][k] = *reinterpret_cast<const PD*>(s2 + gidx * V + 2 * k);
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kPostUnroll; ++u) {
      if (!live[u]) continue;
      const int64_t gidx = base + (int64_t)u * kPostBlock + threadIdx.x;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const double x = (double)b[u].v[k];
        const double d = x - (kFirst ? x : (double)r[u].v[k]);
        if (kFirst) {
          a1[u][k / 2].v[k % 2] = d;
          a2[u][k / 2].v[k % 2] = d * d;
        } else {
          a1[u][k / 2].v[k % 2] += d;
          a2[u][k / 2].v[k % 2] += d * d;
        }
      }
      if (kFirst) *reinterpret_cast<PT*>(ref + gidx * V) = b[u];
#pragma unroll
      for (int k = 0; k < kD; ++k) {
        *reinterpret_cast<PD*>(s1 + gidx * V + 2 * k) = a1[u][k];
        *reinterpret_cast<PD*>(s2 + gidx * V + 2 * k) = a2[u][k];
      }
    }
  }
  // tail: the n % V elements after the last whole group (an odd cell count)
  const int64_t t = n_groups * V + threadIdx.x;
  if (blockIdx.x == 0 && t < n) {
    const double x = (double)beds[t];
    const double d = x - (kFirst ? x : (double)ref[t]);
    if (kFirst) { ref[t] = beds[t]; s1[t] = d; s2[t] = d * d; }
    else { s1[t] += d; s2[t] += d * d; }
  }
}

// ---- pooled form -----------------------------------------------------------------------------------------------------
// part p of blockIdx.y sums d = bed_c - g and d * d over its chains [p * cpp, (p + 1) * cpp) in index order, V cells per lane,
// into slab[(p * 2 + f) * plane + cell], f = 0 (sum d), 1 (sum d * d).  plane % V == 0.
template <typename T, int V>
__global__ __launch_bounds__(kPostBlock) void post_pooled_kernel(const T* __restrict__ beds, const double* __restrict__ g,
                                                                 double* __restrict__ slab, int64_t plane, int n_chains, int cpp) {
  using PT = Pack<T, V>;
  const int64_t cell = ((int64_t)blockIdx.x * kPostBlock + threadIdx.x) * V;
  if (cell >= plane) return;
  const auto [c0, c1] = chain_range(cpp, n_chains);
  double gv[V], a1[V], a2[V];
#pragma unroll
  for (int k = 0; k < V; ++k) { gv[k] = g[cell + k]; a1[k] = 0.0; a2[k] = 0.0; }
  int c = c0;
  for (; c + kPostChains <= c1; c += kPostChains) {
    PT b[kPostChains];
#pragma unroll
    for (int j = 0; j < kPostChains; ++j) b[j] = *reinterpret_cast<const PT*>(beds + (int64_t)(c + j) * plane + cell);
#pragma unroll
    for (int j = 0; j < kPostChains; ++j)
#pragma unroll
      for (int k = 0; k < V; ++k) { const double d = (double)b[j].v[k] - gv[k]; a1[k] += d; a2[k] += d * d; }
  }
  for (; c < c1; ++c) {
    const PT b = *reinterpret_cast<const PT*>(beds + (int64_t)c * plane + cell);
#pragma unroll
    for (int k = 0; k < V; ++k) { const double d = (double)b.v[k] - gv[k]; a1[k] += d; a2[k] += d * d; }
  }
  double* o1 = slab + ((int64_t)blockIdx.y * 2 + 0) * plane + cell;
  double* o2 = slab + ((int64_t)blockIdx.y * 2 + 1) * plane + cell;
#pragma unroll
  for (int k = 0; k < V; ++k) { o1[k] = a1[k]; o2[k] = a2[k]; }
}

// ---- reduction over this handle's sequences --------------------------------------------------------------------------
// part p sums, over its chains in index order and each chain's n_seq sequences in order, a = (ref_c - g) + s1 / N,
// a * a and v = (s2 - s1 * s1 / N) / (N - 1) into slab[(p * 3 + f) * plane + cell]; sequence k of chain c has its sums at
// k * seq_stride + c * plane; the first n_closed sequences of a chain hold (a_m, v_m) already (post_close_kernel).  One cell per lane.
template <typename T>
__global__ __launch_bounds__(kPostBlock) void post_partials_kernel(const T* __restrict__ ref, const double* __restrict__ g,
                                                                   const double* __restrict__ s1, const double* __restrict__ s2,
                                                                   double* __restrict__ slab, int64_t plane, int n_chains, int n_seq,
                                                                   int64_t seq_stride, int n_closed, double N, int cpp) {
  const int64_t cell = (int64_t)blockIdx.x * kPostBlock + threadIdx.x;
  if (cell >= plane) return;
  const auto [c0, c1] = chain_range(cpp, n_chains);
  const double gv = g[cell], nm1 = N - 1.0;
  double p0 = 0.0, p1 = 0.0, p2 = 0.0;
#pragma unroll 2
  for (int c = c0; c < c1; ++c) {
    const double r = (double)ref[(int64_t)c * plane + cell] - gv;
    for (int k = 0; k < n_seq; ++k) {
      const int64_t i = (int64_t)k * seq_stride + (int64_t)c * plane + cell;
      const double x1 = s1[i], x2 = s2[i];
      const double a = k < n_closed ? x1 : r + x1 / N;
      const double v = k < n_closed ? x2 : (x2 - x1 * x1 / N) / nm1;
      p0 += a; p1 += a * a; p2 += v;
    }
  }
  slab[((int64_t)blockIdx.y * 3 + 0) * plane + cell] = p0;
  slab[((int64_t)blockIdx.y * 3 + 1) * plane + cell] = p1;
  slab[((int64_t)blockIdx.y * 3 + 2) * plane + cell] = p2;
}

// A finished sequence's sums become its mean minus g and its variance, in place: s1 = (ref_c - g) + s1 / N, s2 = (s2 - s1^2 / N) /
// (N - 1).  After it `ref` is free to take the next sequence's first snapshot, so that EVERY sequence is shifted by a value of
// its own and a sequence that never changes has variance 0 exactly.  blockIdx.y = chain.
template <typename T>
__global__ __launch_bounds__(kPostBlock) void post_close_kernel(const T* __restrict__ ref, const double* __restrict__ g,
                                                                double* __restrict__ s1, double* __restrict__ s2, int64_t plane, double N) {
  const int64_t cell = (int64_t)blockIdx.x * kPostBlock + threadIdx.x;
  if (cell >= plane) return;
  const int64_t i = (int64_t)blockIdx.y * plane + cell;
  const double x1 = s1[i], x2 = s2[i];
  s1[i] = ((double)ref[i] - g[cell]) + x1 / N;
  s2[i] = (x2 - x1 * x1 / N) / (N - 1.0);
}

// out.f[i][cell] (+)= sum over parts, in part order, of slab[(p * n_fields + i) * plane + cell]
__global__ __launch_bounds__(kPostBlock) void post_combine_kernel(const double* __restrict__ slab, int parts, int n_fields, int64_t plane,
                                                                  PostOut out, int add) {
  for (int64_t cell = (int64_t)blockIdx.x * kPostBlock + threadIdx.x; cell < plane; cell += (int64_t)gridDim.x * kPostBlock)
    for (int f = 0; f < n_fields; ++f) {
      double s = 0.0;
      for (int p = 0; p < parts; ++p) s += slab[((int64_t)p * n_fields + f) * plane + cell];
      out.f[f][cell] = add ? out.f[f][cell] + s : s;
    }
}

// out[c * n_samples + p] = bed of chain c at cells[p] (NaN for a cell index outside the grid)
template <typename T>
__global__ __launch_bounds__(kPostBlock) void post_sample_kernel(const T* __restrict__ beds, const int32_t* __restrict__ cells, int n_samples,
                                                                 int n_chains, int64_t plane, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kPostBlock + threadIdx.x;
  if (i >= (int64_t)n_chains * n_samples) return;
  const int c = (int)(i / n_samples), p = (int)(i % n_samples);
  const int32_t cell = cells[p];
  out[i] = (cell >= 0 && cell < plane) ? (double)beds[(int64_t)c * plane + cell] : __builtin_nan("");
}

}  // namespace

hipError_t launch_posterior_combine(const double* slab, int parts, int n_fields, int64_t plane, const PostOut& out, int add, int n_cu,
                                    hipStream_t st) {
  hipLaunchKernelGGL(post_combine_kernel, dim3(grid_for(plane, kPostBlock, n_cu)), dim3(kPostBlock), 0, st, slab, parts, n_fields, plane, out, add);
  return hipGetLastError();
}

hipError_t launch_posterior_accumulate(const void* beds, void* ref, double* s1, double* s2, int64_t n, int f32_state, int first, int n_cu,
                                       hipStream_t st) {
  dispatch_state(f32_state, [&](auto tag) {
    using T = typename decltype(tag)::T;
    constexpr int V = decltype(tag)::V;
    const dim3 grid(grid_for(n / V, kPostBlock * kPostUnroll, n_cu));
    if (first) hipLaunchKernelGGL((post_accumulate_kernel<T, V, true>), grid, dim3(kPostBlock), 0, st, (const T*)beds, (T*)ref, s1, s2, n);
    else hipLaunchKernelGGL((post_accumulate_kernel<T, V, false>), grid, dim3(kPostBlock), 0, st, (const T*)beds, (T*)ref, s1, s2, n);
  });
  return hipGetLastError();
}

hipError_t launch_posterior_pooled(const void* beds, const double* g, double* s1, double* s2, double* slab, int64_t plane, int n_chains,
                                   int parts, int f32_state, int n_cu, hipStream_t st) {
  const int vec = posterior_vec(plane, f32_state);
  const dim3 grid((unsigned)posterior_cell_blocks(plane, vec), (unsigned)parts);
  dispatch_state_vec(f32_state, vec, [&](auto tag) {
    using T = typename decltype(tag)::T;
    hipLaunchKernelGGL((post_pooled_kernel<T, decltype(tag)::V>), grid, dim3(kPostBlock), 0, st, (const T*)beds, g, slab, plane, n_chains,
                       chains_per_part(n_chains, parts));
  });
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_posterior_combine(slab, parts, 2, plane, PostOut{{s1, s2}}, 1, n_cu, st);
}

hipError_t launch_posterior_partials(const void* ref, const double* g, const double* s1, const double* s2, double* slab, double* partials,
                                     int64_t plane, int n_chains, int n_seq, int64_t seq_stride, int n_closed, int n_per_seq, int parts, int f32_state,
                                     int n_cu, hipStream_t st) {
  const dim3 grid((unsigned)posterior_cell_blocks(plane, 1), (unsigned)parts);
  dispatch_state(f32_state, [&](auto tag) {
    using T = typename decltype(tag)::T;
    hipLaunchKernelGGL((post_partials_kernel<T>), grid, dim3(kPostBlock), 0, st, (const T*)ref, g, s1, s2, slab, plane, n_chains, n_seq, seq_stride,
                       n_closed, (double)n_per_seq, chains_per_part(n_chains, parts));
  });
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_posterior_combine(slab, parts, 3, plane, PostOut{{partials, partials + plane, partials + 2 * plane}}, 0, n_cu, st);
}

hipError_t launch_posterior_close(const void* ref, const double* g, double* s1, double* s2, int64_t plane, int n_chains, int n_per_seq,
                                  int f32_state, hipStream_t st) {
  const dim3 grid((unsigned)posterior_cell_blocks(plane, 1), (unsigned)n_chains);
  dispatch_state(f32_state, [&](auto tag) {
    using T = typename decltype(tag)::T;
    hipLaunchKernelGGL((post_close_kernel<T>), grid, dim3(kPostBlock), 0, st, (const T*)ref, g, s1, s2, plane, (double)n_per_seq);
  });
  return hipGetLastError();
}

hipError_t launch_posterior_sample(const void* beds, const int32_t* cells, int n_samples, int n_chains, int64_t plane, int f32_state,
                                   double* out, hipStream_t st) {
  const dim3 grid((unsigned)(((int64_t)n_chains * n_samples + kPostBlock - 1) / kPostBlock));
  dispatch_state(f32_state, [&](auto tag) {
    using T = typename decltype(tag)::T;
    hipLaunchKernelGGL((post_sample_kernel<T>), grid, dim3(kPostBlock), 0, st, (const T*)beds, cells, n_samples, n_chains, plane, out);
  });
  return hipGetLastError();
}

}  // namespace gsm
