// C ABI of libgsm_hip.so (see include/gsm.h for the contract and the reference interfaces replaced): handle lifetime, the handle's tables, loss / residual,
// covariance / Cholesky, the quantile transform, min-dist, debug entries.  The rest: gsm_api_chain.hip, gsm_api_sgs.hip, gsm_api_posterior.hip.
#include "gsm_context.h"
#include "math_tables.h"
#include "normal_score.h"
#include <math.h>
#include <string.h>
#include <algorithm>

using namespace gsm;

static thread_local std::string g_create_err;

int gsm::fail(gsm_handle h, int code, const std::string& msg) {
  if (h) h->err = msg; else g_create_err = msg;
  return code;
}

extern "C" const char* gsm_last_error(gsm_handle h) { return h ? h->err.c_str() : g_create_err.c_str(); }

extern "C" int gsm_create(gsm_handle* out, int32_t H, int32_t W, int32_t n_chains, int32_t dtype, int32_t device) {
  if (!out) return fail(nullptr, GSM_E_ARG, "gsm_create: out is NULL");
  *out = nullptr;
  if (H < 1 || W < 1 || n_chains < 1) return fail(nullptr, GSM_E_ARG, "gsm_create: need H,W >= 1 and n_chains >= 1");
  if ((int64_t)H * W > (1LL << 30)) return fail(nullptr, GSM_E_ARG, "gsm_create: grid too large");
  if (dtype != 0 && dtype != 1) return fail(nullptr, GSM_E_UNSUPPORTED, "gsm_create: dtype must be 0 (fp64 state) or 1 (fp32 state)");
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev < 1)
    return fail(nullptr, GSM_E_HIP, std::string("gsm_create: no HIP device: ") + hipGetErrorString(e));
  if (device < 0 || device >= ndev) return fail(nullptr, GSM_E_ARG, "gsm_create: device index out of range");
  e = hipSetDevice(device);
  if (e != hipSuccess) return fail(nullptr, GSM_E_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
  gsm_context* c = new gsm_context();
  c->H = H; c->W = W; c->n_chains = n_chains; c->device = device; c->f32_state = dtype;
  e = c->d_err.ensure(1);
  if (e == hipSuccess) e = hipMemset(c->d_err.get(), 0, sizeof(int32_t));
  if (e != hipSuccess) { delete c; return fail(nullptr, GSM_E_HIP, std::string("hipMalloc: ") + hipGetErrorString(e)); }
  *out = c;
  return GSM_OK;
}

extern "C" int gsm_destroy(gsm_handle h) {
  if (!h) return GSM_OK;
  hipSetDevice(h->device);
  delete h;          // every device resource of the handle is a member that owns it (gsm_context.h)
  return GSM_OK;
}

extern "C" int gsm_set_option(gsm_handle h, int32_t which, int32_t value) {
  if (!h) return GSM_E_ARG;
  int* const opt = which == GSM_OPT_FUSED ? &h->use_fused : which == GSM_OPT_STRIP ? &h->use_strip : which == GSM_OPT_SPLIT2 ? &h->use_split2 :
                   which == GSM_OPT_FUSED_SEGMENT ? &h->fused_segment : nullptr;
  if (!opt) return fail(h, GSM_E_ARG, "gsm_set_option: unknown option " + std::to_string(which));
  if (which == GSM_OPT_FUSED_SEGMENT ? value < 1 : (value != 0 && value != 1))
    return fail(h, GSM_E_ARG, "gsm_set_option: value " + std::to_string(value) + " out of range for option " + std::to_string(which));
  *opt = value;
  return GSM_OK;
}

extern "C" int gsm_set_static(gsm_handle h, const double* surf, const double* velx, const double* vely,
                              const double* dhdt, const double* smb, const double* crf_weight,
                              const uint8_t* update_mask, const uint8_t* mc_mask, double resolution,
                              double sigma_mc, void* stream) {
  GSM_GRID_HANDLE(h);
  if (!surf || !velx || !vely || !dhdt || !smb || !update_mask || !mc_mask)
    return fail(h, GSM_E_ARG, "gsm_set_static: NULL field");
  if (!(resolution > 0.0) || !(sigma_mc > 0.0)) return fail(h, GSM_E_ARG, "gsm_set_static: resolution and sigma_mc must be > 0");
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(h, hipSetDevice(h->device));
  const size_t n = (size_t)h->H * h->W;
  const double* src[6] = {surf, velx, vely, dhdt, smb, crf_weight};
  for (int i = 0; i < 6; ++i) {
    if (!src[i]) { h->d_static[i].reset(); continue; }
    HIPCHK(h, h->d_static[i].assign(src[i], n, st));
  }
  HIPCHK(h, h->d_upd.assign(update_mask, n, st));
  HIPCHK(h, h->d_mc.assign(mc_mask, n, st));
  StaticFields& S = h->S;
  S.surf = h->d_static[0].get(); S.velx = h->d_static[1].get(); S.vely = h->d_static[2].get();
  S.dhdt = h->d_static[3].get(); S.smb = h->d_static[4].get(); S.weight = h->d_static[5].get();
  S.upd = h->d_upd.get(); S.mc = h->d_mc.get();
  S.H = h->H; S.W = h->W;
  {
    // The rectangle the strip kernels cut every window down to (StaticFields::tr0 ..): bounding box of the set cells, grown by the
    // stencil's reach and clipped to the grid.  One pass over a host copy of the mask (the caller's array may live on the device);
    // gsm_set_static is the only place a handle's update mask is set.
    std::vector<uint8_t> um(n);
    HIPCHK(h, hipMemcpyAsync(um.data(), update_mask, n, hipMemcpyDefault, st));
    HIPCHK(h, hipStreamSynchronize(st));
    int r_lo = h->H, r_hi = -1, c_lo = h->W, c_hi = -1;
    for (int r = 0; r < h->H; ++r) {
      const uint8_t* m = um.data() + (size_t)r * h->W;
      for (int c = 0; c < h->W; ++c)
        if (m[c]) { r_lo = std::min(r_lo, r); r_hi = r; c_lo = std::min(c_lo, c); c_hi = std::max(c_hi, c); }
    }
    if (r_hi < 0) S.tr0 = S.tr1 = S.tc0 = S.tc1 = 0;
    else {
      S.tr0 = std::max(r_lo - 1, 0); S.tr1 = std::min(r_hi + 2, h->H);
      S.tc0 = std::max(c_lo - 1, 0); S.tc1 = std::min(c_hi + 2, h->W);
    }
  }
  S.res = resolution;
  S.two_res = 2.0 * resolution;
  S.rcp_res = 1.0 / S.res;
  S.rcp_two_res = 1.0 / S.two_res;
  S.two_sigma2 = 2 * (sigma_mc * sigma_mc);
  S.rcp_two_sigma2 = 1.0 / S.two_sigma2;
  // exact_div() needs a correctly rounded reciprocal of a divisor whose significand is not all ones and
  // quotients far from the exponent limits; anything else takes the IEEE division path.
  {
    auto divisor_ok = [](double d) {
      uint64_t bits;
      memcpy(&bits, &d, sizeof(bits));
      const bool all_ones = (bits & 0xFFFFFFFFFFFFFull) == 0xFFFFFFFFFFFFFull;
      return !all_ones && d > 1e-100 && d < 1e100;
    };
    S.fast_div = (divisor_ok(S.res) && divisor_ok(S.two_sigma2)) ? 1 : 0;
  }
  HIPCHK(h, h->d_svx.ensure(n));          // allocated by the first call: n is the handle's
  HIPCHK(h, h->d_svy.ensure(n));
  HIPCHK(h, h->d_ds.ensure(n));
  HIPCHK(h, h->d_sABC.ensure(3 * n));      // sA | sB | sC in one allocation (one buffer descriptor)
  double2 *sA = h->d_sABC.get(), *sB = sA + n, *sC = sA + 2 * n;
  HIPCHK(h, launch_pack_static(S, h->d_svx.get(), h->d_svy.get(), h->d_ds.get(), st));
  HIPCHK(h, launch_pack_flux_static(S, sA, sB, sC, st));
  S.svx = h->d_svx.get(); S.svy = h->d_svy.get(); S.ds = h->d_ds.get();
  S.sA = sA; S.sB = sB; S.sC = sC;
  HIPCHK(h, hipStreamSynchronize(st));
  h->have_static = true;
  return GSM_OK;
}

extern "C" int gsm_set_blocks(gsm_handle h, int32_t n_sizes, const int32_t* bh, const int32_t* bw,
                              const double* edge_masks_packed, const int64_t* mask_offsets, void* stream) {
  GSM_GRID_HANDLE(h);
  if (n_sizes < 1 || !bh || !bw) return fail(h, GSM_E_ARG, "gsm_set_blocks: empty block table");
  if (n_sizes > 64) return fail(h, GSM_E_UNSUPPORTED, "gsm_set_blocks: at most 64 block sizes");
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(h, hipSetDevice(h->device));
  int max_bh = 0, max_bw = 0, cap = 0;
  int64_t mask_total = 0;
  for (int i = 0; i < n_sizes; ++i) {
    // proposal_device.h has no code for odd lengths (both DFT stages split by the parity of k): this test is the only gate
    if (bh[i] < 2 || bw[i] < 2 || (bh[i] & 1) || (bw[i] & 1))
      return fail(h, GSM_E_ARG, "gsm_set_blocks: block sizes must be even and >= 2 (RandField.get_block_sizes makes them even)");
    if (bh[i] > h->H || bw[i] > h->W)
      return fail(h, GSM_E_ARG, "gsm_set_blocks: block larger than the grid (the reference's slices mismatch there)");
    max_bh = std::max(max_bh, bh[i]);
    max_bw = std::max(max_bw, bw[i]);
    cap = std::max(cap, (bh[i] + 2) * (bw[i] + 2));
    if (mask_offsets) mask_total = std::max<int64_t>(mask_total, mask_offsets[i] + (int64_t)bh[i] * bw[i]);
  }
  if (step_lds_bytes(cap) > 160 * 1024)
    return fail(h, GSM_E_UNSUPPORTED, "gsm_set_blocks: (bh+2)*(bw+2) window does not fit the 160 KiB LDS tile");
  // the factors of gsm_set_factors and the Cholesky generator's scratch belong to the table that is replaced from here on:
  // one pointer per (size, class) of THAT table, buffers sized by its largest block.  gsm_set_factors is due again.
  h->d_factors.reset();
  h->n_classes = 0;
  for (auto& c : h->chol) c = gsm_context::CholScratch();
  HIPCHK(h, h->d_bh.assign(bh, (size_t)n_sizes, st));
  HIPCHK(h, h->d_bw.assign(bw, (size_t)n_sizes, st));
  if (edge_masks_packed && mask_offsets) {
    HIPCHK(h, h->d_mask_off.assign(mask_offsets, (size_t)n_sizes, st));
    HIPCHK(h, h->d_masks.assign(edge_masks_packed, (size_t)mask_total, st));
    // The reference's edge masks are a function of the distance to the nearest border cell of the block (get_edge_masks,
    // MCMC.py:583-621): mask[y][x] = T[min(y, bh - 1 - y, x, bw - 1 - x)].  Checked value for value here; if every mask of the
    // table has that form, the strip kernel reads the 64-entry T from LDS instead of 8 bytes per cell from a 51 KB table.
    h->d_mask1d.reset();
    {
      std::vector<double> hm((size_t)mask_total);
      HIPCHK(h, hipMemcpyAsync(hm.data(), edge_masks_packed, sizeof(double) * (size_t)mask_total, hipMemcpyDefault, st));
      HIPCHK(h, hipStreamSynchronize(st));
      std::vector<double> t1((size_t)n_sizes * kMask1D, 0.0);
      bool one_d = true;
      for (int i = 0; i < n_sizes && one_d; ++i) {
        const double* m = hm.data() + mask_offsets[i];
        const int H = bh[i], W = bw[i];
        if ((std::min(H, W) - 1) / 2 >= kMask1D) { one_d = false; break; }
        std::vector<char> have(kMask1D, 0);
        for (int y = 0; y < H && one_d; ++y)
          for (int x = 0; x < W; ++x) {
            const int d = std::min(std::min(y, H - 1 - y), std::min(x, W - 1 - x));
            const double v = m[(size_t)y * W + x];
            double& t = t1[(size_t)i * kMask1D + d];
            if (!have[d]) { have[d] = 1; t = v; }
            else if (memcmp(&t, &v, sizeof(double)) != 0) { one_d = false; break; }
          }
      }
      if (one_d) HIPCHK(h, h->d_mask1d.assign(t1.data(), t1.size(), st));
      HIPCHK(h, hipStreamSynchronize(st));
    }
  } else {
    h->d_masks.reset();
    h->d_mask_off.reset();
    h->d_mask1d.reset();
  }
  // DFT operand tables of the proposal kernel, one set per distinct block height / width, folded to indices <= n/2
  // and zero padded to the MFMA tile grid (dimension formulas mirror propose_kernel):
  //   height n: FC[ky][y] = cos(2 pi ky y / n), FS = sin(...), ky, y <= n/2, each [KR = ceil4(n/2+1)][NR = ceil16(n/2+1)]
  //   width  n: GC[k][x]  = c_k cos(2 pi k x / n), GS = -c_k sin(...), k, x <= n/2 (c_k = 1 for k in {0, n/2}, else 2),
  //             each [Kc = ceil4(n/2+1)][M1 = ceil16(n/2+1)]
  const int max_len = std::max(max_bh, max_bw);
  std::vector<int32_t> fy_off(max_len + 1, -1), g_off(max_len + 1, -1);
  std::vector<double> tb;
  int krmax = 0, n1max = 0, m1max = 0, kcmax = 0, tiles_max = 0;
  h->prop_tiles1 = 0;
  for (int i = 0; i < n_sizes; ++i) {
    const int n = bh[i];
    const int nrow = n / 2 + 1;
    const int KR = (nrow + 3) & ~3, NR = (nrow + 15) & ~15, N1 = (n + 15) & ~15;
    krmax = std::max(krmax, KR); n1max = std::max(n1max, N1);
    if (fy_off[n] < 0) {
      fy_off[n] = (int32_t)tb.size();
      tb.resize(tb.size() + (size_t)2 * KR * NR, 0.0);
      double* FC = tb.data() + fy_off[n];
      double* FS = FC + (size_t)KR * NR;
      for (int ky = 0; ky < nrow; ++ky)
        for (int y = 0; y < nrow; ++y) {
          const double ang = 2.0 * M_PI * (double)(((int64_t)ky * y) % n) / (double)n;
          FC[ky * NR + y] = cos(ang);
          FS[ky * NR + y] = sin(ang);
        }
    }
    const int w = bw[i];
    const int ncol = w / 2 + 1, Kc = (ncol + 3) & ~3, M1 = (ncol + 15) & ~15;
    m1max = std::max(m1max, M1); kcmax = std::max(kcmax, Kc);
    tiles_max = std::max(tiles_max, (N1 / 16) * (M1 / 16));
    // stage-1 work units = 2 x this: (output tile, re | im, parity of ky) over the half range of y (proposal_device.h: dft_stage1)
    const int NRh = ((n / 2) / 2 + 16) & ~15;
    h->prop_tiles1 = std::max(h->prop_tiles1, 2 * (M1 / 16) * (NRh / 16));
    if (g_off[w] < 0) {
      g_off[w] = (int32_t)tb.size();
      tb.resize(tb.size() + (size_t)2 * Kc * M1, 0.0);
      double* GC = tb.data() + g_off[w];
      double* GS = GC + (size_t)Kc * M1;
      for (int k = 0; k < ncol; ++k) {
        const double ck = (k == 0 || k == w / 2) ? 1.0 : 2.0;
        for (int x = 0; x < ncol; ++x) {
          const double ang = 2.0 * M_PI * (double)(((int64_t)k * x) % w) / (double)w;
          GC[k * M1 + x] = ck * cos(ang);
          GS[k * M1 + x] = -ck * sin(ang);
        }
      }
    }
  }
  auto stride16mod32 = [](int v) { int s = v; while ((s & 31) != 16) ++s; return s; };
  h->lds_sx = stride16mod32(m1max);
  h->lds_st = stride16mod32(n1max);
  h->lds_x_half = (krmax * h->lds_sx + 127) & ~127;   // one of the four folded coefficient planes; whole 1 KiB LDS-DMA pieces
  h->lds_tt = 2 * kcmax * h->lds_st;
  h->prop_tiles = tiles_max;
  h->tables_len = (int)tb.size();
  h->tab_max = 0;
  for (int i = 0; i < n_sizes; ++i) {
    const int nrow = bh[i] / 2 + 1, ncol = bw[i] / 2 + 1;
    h->tab_max = std::max(h->tab_max, 2 * ((nrow + 3) & ~3) * ((nrow + 15) & ~15));
    h->tab_max = std::max(h->tab_max, 2 * ((ncol + 3) & ~3) * ((ncol + 15) & ~15));
  }
  {
    std::vector<int32_t> k2_off((size_t)n_sizes);
    int32_t tot = 0;
    for (int i = 0; i < n_sizes; ++i) { k2_off[i] = tot; tot += (bh[i] / 2 + 1) * (bw[i] / 2 + 1); }
    HIPCHK(h, h->d_k2_off.assign(k2_off.data(), k2_off.size(), st));
    h->d_k2.reset();
    HIPCHK(h, h->d_k2.ensure((size_t)tot));
    h->k2_resolution = 0.0;
  }
  HIPCHK(h, h->d_tables.assign(tb.data(), tb.size(), st));
  HIPCHK(h, h->d_fy_off.assign(fy_off.data(), fy_off.size(), st));
  HIPCHK(h, h->d_g_off.assign(g_off.data(), g_off.size(), st));
  {
    // 1-D twiddle tables: for every distinct block length n the values cos / sin(2 pi m / n), m < n -- the numbers the 2-D
    // tables above hold at (k, j) with m = (k * j) mod n (same expression, same libm calls: bit-identical operands)
    std::vector<int32_t> t1_off(max_len + 1, 0);
    std::vector<double> t1;
    std::vector<char> seen(max_len + 1, 0);
    for (int i = 0; i < n_sizes; ++i)
      for (int n : {bh[i], bw[i]}) {
        if (seen[n]) continue;
        seen[n] = 1;
        t1_off[n] = (int32_t)t1.size();
        for (int m = 0; m < n; ++m) t1.push_back(cos(2.0 * M_PI * (double)m / (double)n));
        for (int m = 0; m < n; ++m) t1.push_back(sin(2.0 * M_PI * (double)m / (double)n));
      }
    HIPCHK(h, h->d_tab1d.assign(t1.data(), t1.size(), st));
    HIPCHK(h, h->d_t1_off.assign(t1_off.data(), t1_off.size(), st));
    HIPCHK(h, hipStreamSynchronize(st));       // the host vectors end with this block
  }
  HIPCHK(h, hipStreamSynchronize(st));
  h->B.bh = h->d_bh.get(); h->B.bw = h->d_bw.get(); h->B.masks = h->d_masks.get(); h->B.mask_off = h->d_mask_off.get(); h->B.mask1d = h->d_mask1d.get();
  h->B.n_sizes = n_sizes; h->B.max_bh = max_bh; h->B.max_bw = max_bw;
  h->tile_cap = cap;
  h->field_stride = (int64_t)max_bh * max_bw;
  h->have_blocks = true;
  for (auto& s : h->scr) s = gsm_context::Scratch();
  return GSM_OK;
}

extern "C" int gsm_set_centres(gsm_handle h, const int32_t* cells, int32_t n_cells, void* stream) {
  GSM_GRID_HANDLE(h);
  if (!cells || n_cells < 1) return fail(h, GSM_E_ARG, "gsm_set_centres: empty centre list");
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, h->d_centres.assign(cells, (size_t)n_cells, st));
  HIPCHK(h, hipStreamSynchronize(st));
  h->n_centres = n_cells;
  h->have_centres = true;
  return GSM_OK;
}

extern "C" int gsm_init_loss(gsm_handle h, const void* beds, void* energy, double* loss_sum, double* loss0, void* stream) {
  GSM_GRID_HANDLE(h);
  if (!h->have_static) return fail(h, GSM_E_STATE, "gsm_init_loss: call gsm_set_static first");
  if (!beds || !energy || !loss_sum) return fail(h, GSM_E_ARG, "gsm_init_loss: NULL pointer");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, launch_init_loss(h->S, h->n_chains, beds, energy, h->f32_state, loss_sum, loss0, (hipStream_t)stream));
  return GSM_OK;
}

extern "C" int gsm_residual(gsm_handle h, const double* beds, double* residual, void* stream) {
  GSM_GRID_HANDLE(h);
  if (!h->have_static) return fail(h, GSM_E_STATE, "gsm_residual: call gsm_set_static first");
  if (!beds || !residual) return fail(h, GSM_E_ARG, "gsm_residual: NULL pointer");
  if (h->f32_state) return fail(h, GSM_E_UNSUPPORTED, "gsm_residual: fp64 beds only (create the handle with dtype 0)");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, launch_residual(h->S, h->n_chains, beds, residual, (hipStream_t)stream));
  return GSM_OK;
}

// 1 when this handle's static fields and block table go to the strip kernels (chain_strip_kernel.hip)
int gsm::strip_for(gsm_handle h) {
  return (h->use_strip && h->have_static && h->have_blocks &&
          strip_table_ok(h->S, h->B, std::max(4 * h->lds_x_half, h->lds_tt), h->prop_tiles1, h->prop_tiles)) ? 1 : 0;
}

extern "C" int gsm_strip_active(gsm_handle h) {
  GSM_GRID_HANDLE(h);
  if (!h->have_static || !h->have_blocks) return fail(h, GSM_E_STATE, "gsm_strip_active: call gsm_set_static and gsm_set_blocks first");
  return strip_for(h);
}

int gsm::read_and_clear_flag(gsm_handle h, hipStream_t st, int32_t* flag) {
  *flag = 0;
  HIPCHK(h, hipMemcpyAsync(flag, h->d_err.get(), sizeof(*flag), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  if (*flag) {
    hipMemsetAsync(h->d_err.get(), 0, sizeof(int32_t), st);
    hipStreamSynchronize(st);
  }
  return GSM_OK;
}

hipError_t gsm::ensure_mathtab(DevBuf<double>& d) {
  if (d.get()) return hipSuccess;
  double tab[kMathTabDoubles];
  build_math_tables(tab);
  hipError_t e = d.ensure(kMathTabDoubles);
  if (e == hipSuccess) e = hipMemcpy(d.get(), tab, sizeof(tab), hipMemcpyHostToDevice);
  if (e != hipSuccess) d.reset();
  return e;
}

extern "C" int gsm_cov_assemble(gsm_handle h, int32_t bh, int32_t bw, double resolution, const gsm_vario* vario,
                                const double* lag_table, double* sigma, int64_t ld, void* stream) {
  GSM_GRID_HANDLE(h);
  if (!vario || !sigma || bh < 1 || bw < 1 || ld < (int64_t)bh * bw || ld > 0x7fffffff)
    return fail(h, GSM_E_ARG, "gsm_cov_assemble: bad argument");
  if (vario->vtype < 0 || vario->vtype > 3) return fail(h, GSM_E_ARG, "gsm_cov_assemble: unknown vtype");
  if (vario->vtype == GSM_VTYPE_MATERN && !lag_table)
    return fail(h, GSM_E_ARG, "gsm_cov_assemble: the Matern model needs the host-computed lag table (scipy.special.kv)");
  if (!(vario->major_range > 0.0) || !(vario->minor_range > 0.0) || !(resolution > 0.0))
    return fail(h, GSM_E_ARG, "gsm_cov_assemble: ranges and resolution must be > 0");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, launch_cov_assemble(bh, bw, resolution, *vario, lag_table, sigma, (int)ld, (hipStream_t)stream));
  return GSM_OK;
}

extern "C" int gsm_set_factors(gsm_handle h, int32_t n_classes, const double* const* factors, void* stream) {
  GSM_GRID_HANDLE(h);
  if (!h->have_blocks) return fail(h, GSM_E_STATE, "gsm_set_factors: call gsm_set_blocks first");
  if (n_classes < 1 || !factors) return fail(h, GSM_E_ARG, "gsm_set_factors: bad argument");
  if ((int64_t)h->B.n_sizes * n_classes > 4096)      // cz_bucket_kernel keeps its per-group counters in LDS
    return fail(h, GSM_E_UNSUPPORTED, "gsm_set_factors: at most 4096 (block size, range class) groups, n_sizes * n_classes = " +
                                      std::to_string((int64_t)h->B.n_sizes * n_classes));
  const int groups = h->B.n_sizes * n_classes;
  for (int g = 0; g < groups; ++g)
    if (!factors[g]) return fail(h, GSM_E_ARG, "gsm_set_factors: NULL factor");
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(h, h->d_factors.assign(const_cast<const double**>(factors), (size_t)groups, st));
  HIPCHK(h, hipStreamSynchronize(st));
  h->n_classes = n_classes;
  return GSM_OK;
}

// sklearn clips the scores at ppf(1e-7 - spacing(1)) and ppf(1 - (1e-7 - spacing(1))) (QuantileTransformer._transform_col)
std::pair<double, double> gsm::qt_clip() {
  const double lo = 1e-7 - 2.220446049250313e-16;
  return {ns::ndtri(lo), ns::ndtri(1.0 - lo)};
}

extern "C" int gsm_qt_transform(gsm_handle h, const double* quantiles, const double* references, int32_t nq, const double* x,
                                double* out, int64_t n, int32_t inverse, void* stream) {
  GSM_GRID_HANDLE(h);
  if (!quantiles || !references || !x || !out || nq < 1 || n < 0) return fail(h, GSM_E_ARG, "gsm_qt_transform: bad argument");
  const int64_t plane = (int64_t)h->H * h->W;
  if (h->sgs_group() && (n != plane * h->n_chains || h->n_chains > 65535))
    return fail(h, GSM_E_ARG, "gsm_qt_transform: with chain groups set, n must be n_chains * H * W (and n_chains <= 65535)");
  if (n == 0) return GSM_OK;
  const auto [clip_min, clip_max] = qt_clip();
  HIPCHK(h, hipSetDevice(h->device));
  if (h->sgs_group()) {                                       // chain groups: the tables of the element's chain
    HIPCHK(h, launch_qt_groups(quantiles, references, nq, clip_min, clip_max, x, out, h->n_chains, (int)plane, h->sgs_group(), inverse,
                               (hipStream_t)stream));
    return GSM_OK;
  }
  HIPCHK(h, launch_qt(quantiles, references, nq, clip_min, clip_max, x, out, n, inverse, (hipStream_t)stream));
  return GSM_OK;
}

extern "C" int gsm_min_dist_from_mask(gsm_handle h, const double* xx, const double* yy, const uint8_t* mask,
                                      double* dist, void* stream) {
  GSM_GRID_HANDLE(h);
  if (!xx || !yy || !mask || !dist) return fail(h, GSM_E_ARG, "gsm_min_dist_from_mask: NULL pointer");
  HIPCHK(h, hipSetDevice(h->device));
  const int n = h->H * h->W;
  hipStream_t st = (hipStream_t)stream;
  DevBuf<double2> pts;          // scratch of the call
  DevBuf<int> count;
  HIPCHK(h, pts.ensure((size_t)n));
  HIPCHK(h, count.ensure(1));
  HIPCHK(h, hipMemsetAsync(count.get(), 0, sizeof(int), st));
  hipError_t e = launch_min_dist(xx, yy, mask, n, pts.get(), count.get(), dist, st);
  int m = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(&m, count.get(), sizeof(int), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return fail(h, GSM_E_HIP, std::string("gsm_min_dist_from_mask: ") + hipGetErrorString(e));
  if (m == 0) return fail(h, GSM_E_ARG, "gsm_min_dist_from_mask: mask selects no cell");
  return GSM_OK;
}

extern "C" int gsm_gaussian_filter(gsm_handle h, const double* x, double* out, int32_t n, int32_t H, int32_t W, const double* w0, int32_t lw0,
                                   const double* w1, int32_t lw1, void* stream) {
  if (!h) return GSM_E_ARG;                              // the one entry point that takes a grid with a side below 3 cells
  if (!x || !out || !w0 || !w1) return fail(h, GSM_E_ARG, "gsm_gaussian_filter: NULL pointer");
  if (x == out) return fail(h, GSM_E_ARG, "gsm_gaussian_filter: out must not alias x");
  if (n < 1) return fail(h, GSM_E_ARG, "gsm_gaussian_filter: n must be >= 1");
  if (H != h->H || W != h->W) return fail(h, GSM_E_ARG, "gsm_gaussian_filter: H, W are not the handle's");
  if (lw0 < 0 || lw1 < 0 || lw0 > kTrendMaxLw || lw1 > kTrendMaxLw)
    return fail(h, GSM_E_ARG, "gsm_gaussian_filter: lw0, lw1 must be in [0, " + std::to_string(kTrendMaxLw) + "]");
  if ((int64_t)H * W > ((int64_t)1 << 30)) return fail(h, GSM_E_ARG, "gsm_gaussian_filter: at most 2^30 cells per field");
  TrendTaps t0{}, t1{};
  t0.lw = lw0; t1.lw = lw1;
  for (int k = 0; k <= 2 * lw0; ++k) t0.w[k] = w0[k];
  for (int k = 0; k <= 2 * lw1; ++k) t1.w[k] = w1[k];
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, h->d_trend_tmp.ensure((size_t)n * H * W));
  const hipError_t e = launch_gaussian_filter(t0, t1, x, h->d_trend_tmp.get(), out, n, H, W, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) return fail(h, GSM_E_ARG, "gsm_gaussian_filter: n * H * W is more than one launch takes (2^31 workgroups)");
  HIPCHK(h, e);
  return GSM_OK;
}

extern "C" int gsm_cholesky_upper(gsm_handle h, double* a, int32_t n, int64_t ld, double jitter, void* stream) {
  GSM_GRID_HANDLE(h);
  if (!a || n < 64 || (n % 64) != 0 || ld < n || ld > 0x7fffffff)
    return fail(h, GSM_E_ARG, "gsm_cholesky_upper: n must be a positive multiple of 64 and ld >= n");
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(h, hipMemsetAsync(h->d_err.get(), 0, sizeof(int32_t), st));
  HIPCHK(h, launch_cholesky_upper(a, n, (int)ld, jitter, h->d_err.get(), st));
  int32_t info = 0;
  if (int rc = read_and_clear_flag(h, st, &info)) return rc;
  if (info != 0)
    return fail(h, GSM_E_ARG, "gsm_cholesky_upper: matrix not positive definite at pivot " + std::to_string(info) +
                              " (raise the jitter: the Gaussian covariance is numerically singular, SURVEY.md section 7)");
  return GSM_OK;
}

extern "C" int gsm_debug_normals(uint64_t seed, int64_t step, uint32_t stream_id, uint32_t idx0, int32_t n, double* out, void* stream) {
  if (!out || n < 1) return GSM_E_ARG;
  DevBuf<double> tab;
  if (ensure_mathtab(tab) != hipSuccess ||
      launch_debug_normals(seed, step, stream_id, idx0, n, tab.get(), out, (hipStream_t)stream) != hipSuccess ||
      hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return GSM_E_HIP;
  return GSM_OK;
}

extern "C" int gsm_debug_proposal_math(int32_t which, int32_t model, double smoothness, int64_t n, const void* x0, const double* x1,
                                       const double* x2, const double* x3, void* out, void* stream) {
  if (which < 0 || which >= GSM_PMATH_COUNT || n < 1 || n >= ((int64_t)1 << 31) - 256 || !x0 || !out) return GSM_E_ARG;
  DevBuf<double> tab;
  if (ensure_mathtab(tab) != hipSuccess) return GSM_E_HIP;
  const hipError_t e = launch_debug_proposal_math(which, model, smoothness, n, x0, x1, x2, x3, tab.get(), out, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) return GSM_E_ARG;
  if (e != hipSuccess || hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return GSM_E_HIP;
  return GSM_OK;
}

extern "C" int gsm_debug_stream_copy(const double* src, double* dst, int64_t n, void* stream) {
  if (!src || !dst || n < 0) return GSM_E_ARG;
  return launch_stream_copy(src, dst, n, (hipStream_t)stream) == hipSuccess ? GSM_OK : GSM_E_HIP;
}

extern "C" int gsm_struct_size(int32_t which) {
  return which == 0 ? (int)sizeof(gsm_rf_params) : which == 1 ? (int)sizeof(gsm_sgs_batch) : which == 2 ? (int)sizeof(gsm_vario) : -1;
}
