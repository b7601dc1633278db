// The handle behind include/gsm.h, the owners of its device resources and the helpers shared by the gsm_api*.hip translation units.
#pragma once
#include "gsm_internal.h"
#include <utility>

namespace gsm {

// Owners: move-only, never throw, wrap the HIP calls and nothing else.  Every hipMalloc / hipFree / event / stream call of the host layer is
// in this block; a member or a local of one of these types is released on every path, the handle's by `delete` in gsm_destroy.

// Device array of T: a pointer and its capacity in elements.
template <class T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
  DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p_, o.p_); std::swap(cap_, o.cap_); return *this; }
  ~DevBuf() { reset(); }
  void reset() { if (p_) hipFree(p_); p_ = nullptr; cap_ = 0; }
  T* get() const { return p_; }
  // grow-only; a buffer that is too small is freed first, and a failed allocation leaves the buffer empty
  hipError_t ensure(size_t n) {
    if (p_ && cap_ >= n) return hipSuccess;
    reset();
    hipError_t e = hipMalloc(&p_, n * sizeof(T));
    if (e != hipSuccess) p_ = nullptr; else cap_ = n;
    return e;
  }
  // a fresh allocation of exactly n elements, filled from src (host or device) on st
  hipError_t assign(const T* src, size_t n, hipStream_t st) {
    reset();
    hipError_t e = ensure(n);
    return e != hipSuccess ? e : hipMemcpyAsync(p_, src, n * sizeof(T), hipMemcpyDefault, st);
  }
 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
};

// An event or a stream, created with `flags` on first use.  A std::vector<Event> holds the timing events of a call.
template <class H, hipError_t (*Create)(H*, unsigned), hipError_t (*Destroy)(H)>
class Owned {
 public:
  Owned() = default;
  Owned(Owned&& o) noexcept : v_(std::exchange(o.v_, nullptr)) {}
  ~Owned() { if (v_) Destroy(v_); }
  hipError_t ensure(unsigned flags) { return v_ ? hipSuccess : Create(&v_, flags); }
  H get() const { return v_; }
 private:
  H v_ = nullptr;
};
using Event = Owned<hipEvent_t, hipEventCreateWithFlags, hipEventDestroy>;
using Stream = Owned<hipStream_t, hipStreamCreateWithFlags, hipStreamDestroy>;

}  // namespace gsm

struct gsm_context {
  int H = 0, W = 0, n_chains = 0, device = 0, f32_state = 0;
  std::string err;
  bool have_static = false, have_blocks = false, have_centres = false;
  // owned device copies; S and B are the views of them that the kernels take
  gsm::DevBuf<double> d_static[6];  // surf velx vely dhdt smb weight
  gsm::DevBuf<uint8_t> d_upd, d_mc;
  gsm::DevBuf<double2> d_svx, d_svy, d_ds;
  gsm::DevBuf<double2> d_sABC;     // sA | sB | sC in one allocation (one buffer descriptor): S.sB and S.sC point into it
  gsm::StaticFields S{};
  gsm::DevBuf<int32_t> d_bh, d_bw;
  gsm::DevBuf<int64_t> d_mask_off;
  gsm::DevBuf<double> d_masks;
  gsm::DevBuf<double> d_mask1d;    // [n_sizes][kMask1D]: the masks as a function of the distance to the block border, if they are one
  gsm::DevBuf<double> d_tables;
  gsm::DevBuf<int32_t> d_fy_off, d_g_off;
  gsm::DevBuf<double> d_tab1d; gsm::DevBuf<int32_t> d_t1_off;   // 1-D twiddle tables of the strip kernel's DFT stages
  int lds_sx = 0, lds_st = 0, lds_x_half = 0, lds_tt = 0, prop_tiles = 0, prop_tiles1 = 0;
  int tables_len = 0, tab_max = 0;
  gsm::DevBuf<double> d_k2;        // per-size k^2 tables of the spectral amplitude (depend on rf.resolution)
  gsm::DevBuf<double> d_mathtab;   // log / sincos table of the coefficient phase (math_tables.h)
  // gsm_sgs_loss partial sums: a sum and a bad-cell count per (chain, part), a ticket per chain
  struct SgsParts { gsm::DevBuf<double> sum; gsm::DevBuf<int32_t> bad, ticket; size_t cap = 0; } sgs_parts;
  // gsm_sgs_blocks scratch: visiting ranks + one record per (chain, cell slot), see SgsArgs
  static constexpr int kSgsDepth = 8;                                            // sets of record scratch of an overlapped batch (iteration j uses set j mod depth)
  gsm::DevBuf<char> d_sgs_rec[kSgsDepth];                                        // capacity in bytes; sgs_rec_cells: the (chain, cell slot) records a set holds
  size_t sgs_rec_cells[kSgsDepth] = {};
  gsm::DevBuf<double> d_sgs_next_acc;                                            // T(proposed) of every chain (sgs_loss_tail_kernel<true>)
  gsm::Stream sgs_side, sgs_side2; gsm::Event sgs_ev[kSgsDepth + 2];             // gsm_sgs_iterate's second stream (records of later iterations beside the current one)
  int sgs_ktype = 0; const double* sgs_gmean = nullptr;        // gsm_sgs_set_kriging (the caller's array)
  gsm::DevBuf<int32_t> d_sgs_group; int sgs_n_groups = 0;      // gsm_sgs_set_groups: the group of every chain; 0 groups: none set
  const int32_t* sgs_group() const { return sgs_n_groups ? d_sgs_group.get() : nullptr; }
  gsm::DevBuf<uint64_t> d_pcg_tab;   // gsm_draw_pcg64: LCG jump table (kPcgJumpWords) + ziggurat tables (768 words)
  gsm::DevBuf<int32_t> d_k2_off;
  double k2_resolution = 0.0;
  gsm::DevBuf<gsm::PropScalars> d_scalars[2];
  // Cholesky generator
  int n_classes = 0;
  gsm::DevBuf<const double*> d_factors;
  struct CholScratch { gsm::DevBuf<int> ints; gsm::DevBuf<int64_t> zoff; gsm::DevBuf<int> per_rec; gsm::DevBuf<double> scale, zbuf;
                       size_t recs = 0; int groups = 0; } chol[2];
  gsm::BlockTable B{};
  int tile_cap = 0;
  gsm::DevBuf<int32_t> d_centres;
  int n_centres = 0;
  gsm::DevBuf<int32_t> d_err;
  int n_cu = 0;                                               // compute units of the device (grid sizing of the posterior kernels)
  gsm::DevBuf<double> d_post_slab;                            // gsm_posterior_*: per-part sums before they are combined in part order
  gsm::DevBuf<double> d_vario_sum; gsm::DevBuf<int64_t> d_vario_count;   // gsm_variogram_map: per-part sums and counts before they are combined in part order
  gsm::DevBuf<double> d_trend_tmp;                            // gsm_gaussian_filter: the axis-0 pass of every field (grow-only)
  gsm::DevBuf<uint64_t> d_sort_keys[2];                       // gsm_qt_fit: the sort's two key buffers, n * cells keys each (grow-only)
  gsm::DevBuf<double> d_qt_fit_q;                             // gsm_qt_fit: the caller's q on the device (grow-only)
  // philox-mode scratch (two buffers)
  struct Scratch {
    gsm::DevBuf<int32_t> size_idx, centre;
    gsm::DevBuf<double> u, fields;
    size_t recs = 0;
  } scr[2];
  int64_t field_stride = 0;
  gsm::Stream aux;
  gsm::Event ev_prop[2], ev_step[2];
  // timing
  bool timing = false;
  int last_fused = 0;     // 1 when the last gsm_run_philox call went through the fused chain kernel
  // gsm_set_option (include/gsm.h: GSM_OPT_*), read at every call
  int use_fused = 1;      // GSM_OPT_FUSED
  int use_strip = 1;      // GSM_OPT_STRIP: 0 = never the strip kernels on this handle (strip_for)
  int use_split2 = 1;     // GSM_OPT_SPLIT2: effective on strip handles only (make_propose)
  int fused_segment = 4096;   // GSM_OPT_FUSED_SEGMENT: steps per launch of the fused chain kernel
  double t_step_ms = 0, t_prop_ms = 0;
  int n_step_launch = 0, n_prop_launch = 0;
};

namespace gsm {

int fail(gsm_handle h, int code, const std::string& msg);     // records msg (per thread when h is NULL) and returns code
#define HIPCHK(h, expr)                                                                       \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess)                                                                     \
      return fail(h, GSM_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));           \
  } while (0)

// First statement of every entry point that takes a handle, gsm_gaussian_filter excepted: the stencils, searches and tiles behind them
// assume a grid of at least 3 x 3 cells.  gsm_create takes smaller grids for the filter alone (an axis of one or two cells is a
// case of scipy's reflection), and everything else refuses such a handle here.
#define GSM_GRID_HANDLE(h)                                                                                                   \
  do {                                                                                                                       \
    if (!(h)) return GSM_E_ARG;                                                                                              \
    if ((h)->H < 3 || (h)->W < 3)                                                                                            \
      return gsm::fail(h, GSM_E_ARG, std::string(__func__) + ": the handle's grid has a side below 3 cells (gsm_gaussian_filter only)"); \
  } while (0)

// helpers of more than one translation unit (defined in gsm_api.hip unless noted)
int strip_for(gsm_handle h);                                             // 1 when this handle's static fields and block table go to the strip kernels
int read_and_clear_flag(gsm_handle h, hipStream_t st, int32_t* flag);   // the device error flag once st has drained; cleared when it was set
hipError_t ensure_mathtab(DevBuf<double>& d);                            // the table of math_tables.h (Box-Muller of both generators), uploaded once per buffer
std::pair<double, double> qt_clip();                                     // the score limits of scikit-learn's QuantileTransformer
int ensure_pcg_tables(gsm_handle h);                                     // gsm_api_chain.hip

}  // namespace gsm
