// C ABI of libgsm_hip.so, the large-scale chain: replay, the proposal generators, the Philox and noise runs and gsm_draw_pcg64.
#include "gsm_context.h"
#include "math_tables.h"
#include <string.h>
#include <algorithm>

using namespace gsm;

static int check_device_flag(gsm_handle h, hipStream_t st, const char* who) {
  int32_t flag = 0;
  if (int rc = read_and_clear_flag(h, st, &flag)) return rc;
  if (flag) return fail(h, GSM_E_DEVICE_DATA, std::string(who) + ": size index or block centre out of range in device data (those steps were skipped)");
  return GSM_OK;
}

// the step arguments of a launch of n_steps steps per chain whose records are the whole call's (callers with segments or batches
// set rec_stride / rec_offset / in_stride); the proposal inputs (size_idx, centre, u, fields) are the caller's to fill
static StepArgs make_step(gsm_handle h, int n_steps, void* beds, void* energy, uint32_t* resampled, double* loss_sum, double* loss,
                          uint8_t* accept, int32_t* blocks) {
  StepArgs a{};
  a.S = h->S; a.B = h->B;
  a.n_chains = h->n_chains; a.n_steps = n_steps; a.tile_cap = h->tile_cap; a.strip = strip_for(h);
  a.beds = beds; a.energy = energy; a.f32_state = h->f32_state; a.resampled = resampled; a.loss_sum = loss_sum;
  a.loss = loss; a.accept = accept; a.blocks = blocks;
  a.rec_stride = n_steps; a.rec_offset = 0; a.in_stride = n_steps;
  a.err_flag = h->d_err.get();
  return a;
}

extern "C" int gsm_run_replay(gsm_handle h, int32_t n_steps, void* beds, void* energy, uint32_t* resampled, double* loss_sum,
                              const int32_t* size_idx, const int32_t* centre, const double* u,
                              const double* fields, int64_t field_stride, double* loss, uint8_t* accept,
                              void* stream) {
  GSM_GRID_HANDLE(h);
  if (!h->have_static || !h->have_blocks) return fail(h, GSM_E_STATE, "gsm_run_replay: call gsm_set_static and gsm_set_blocks first");
  if (n_steps < 0) return fail(h, GSM_E_ARG, "gsm_run_replay: n_steps < 0");
  if (n_steps == 0) return GSM_OK;
  if (!beds || !energy || !resampled || !loss_sum || !size_idx || !centre || !u || !fields || !loss || !accept)
    return fail(h, GSM_E_ARG, "gsm_run_replay: NULL pointer");
  if (field_stride < (int64_t)h->B.max_bh * h->B.max_bw)
    return fail(h, GSM_E_ARG, "gsm_run_replay: field_stride smaller than the largest block");
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(h, hipSetDevice(h->device));
  StepArgs a = make_step(h, n_steps, beds, energy, resampled, loss_sum, loss, accept, nullptr);
  a.size_idx = size_idx; a.centre = centre; a.u = u; a.fields = fields; a.field_stride = field_stride;
  HIPCHK(h, launch_step(a, st));
  return check_device_flag(h, st, "gsm_run_replay");
}

// need_centres: the call draws its block centres from the list of gsm_set_centres
static int check_propose_ready(gsm_handle h, const gsm_rf_params* rf, const char* who, bool need_centres) {
  if (!h->have_blocks || !h->d_masks.get()) return fail(h, GSM_E_STATE, std::string(who) + ": call gsm_set_blocks with edge masks first");
  if (need_centres && !h->have_centres) return fail(h, GSM_E_STATE, std::string(who) + ": call gsm_set_centres first");
  if (!rf) return fail(h, GSM_E_ARG, std::string(who) + ": rf is NULL");
  if (rf->generator == GSM_GEN_CHOLESKY) {
    if (!h->d_factors.get()) return fail(h, GSM_E_STATE, std::string(who) + ": call gsm_set_factors first");
    return GSM_OK;
  }
  if (rf->generator != GSM_GEN_SPECTRAL) return fail(h, GSM_E_ARG, std::string(who) + ": unknown generator");
  if (rf->model < 0 || rf->model > 2) return fail(h, GSM_E_ARG, std::string(who) + ": unknown covariance model");
  if (!(rf->resolution > 0.0)) return fail(h, GSM_E_ARG, std::string(who) + ": rf.resolution must be > 0");
  if (rf->model == GSM_MODEL_MATERN && !(rf->smoothness > 0.0))
    return fail(h, GSM_E_ARG, std::string(who) + ": Matern needs smoothness > 0");
  const size_t lds = ((size_t)std::max(4 * h->lds_x_half, h->lds_tt) + 64 + kMathTabDoubles) * 8;
  if (lds > 160 * 1024 || h->prop_tiles > propose_max_tiles_per_wave() * propose_waves() ||
      h->prop_tiles1 > propose_max_tiles1_per_wave() * propose_waves())
    return fail(h, GSM_E_UNSUPPORTED, std::string(who) + ": block too large for the proposal kernel (LDS / accumulator tiles)");
  return GSM_OK;
}

// k^2 tables of the spectral amplitude for this resolution (built on first use, rebuilt when the resolution changes)
static int ensure_k2(gsm_handle h, const gsm_rf_params* rf, hipStream_t st) {
  HIPCHK(h, ensure_mathtab(h->d_mathtab));
  if (rf->generator != GSM_GEN_SPECTRAL || h->k2_resolution == rf->resolution) return GSM_OK;
  HIPCHK(h, launch_k2_tables(h->B, h->d_k2_off.get(), rf->resolution, h->d_k2.get(), st));
  h->k2_resolution = rf->resolution;
  return GSM_OK;
}

static int ensure_chol(gsm_handle h, int slot, size_t recs, CholArgs* out) {
  auto& c = h->chol[slot];
  const int groups = h->B.n_sizes * h->n_classes;
  if (c.recs < recs || c.groups != groups) {
    c = gsm_context::CholScratch();          // recs stays 0 until every buffer of the set exists
    const size_t nmax_pad = (size_t)((h->B.max_bh * h->B.max_bw + 63) & ~63);
    HIPCHK(h, c.ints.ensure((size_t)(6 * groups + 4)));
    HIPCHK(h, c.zoff.ensure((size_t)groups));
    HIPCHK(h, c.per_rec.ensure(2 * recs));
    HIPCHK(h, c.scale.ensure(recs));
    HIPCHK(h, c.zbuf.ensure(nmax_pad * (recs + (size_t)64 * groups)));
    c.recs = recs; c.groups = groups;
  }
  out->n_classes = h->n_classes; out->n_groups = groups; out->factors = h->d_factors.get();
  int* ints = c.ints.get();
  out->counts = ints; out->rec_off = ints + groups; out->tile_off = ints + 2 * groups + 1;
  out->work_off = ints + 4 * groups + 2; out->z_off = c.zoff.get();
  out->group_of = c.per_rec.get(); out->order = c.per_rec.get() + recs; out->scale = c.scale.get(); out->zbuf = c.zbuf.get();
  return GSM_OK;
}

// the fields of p's records, by the generator p.rf names; slot: the Cholesky generator's scratch set
static int launch_proposals(gsm_handle h, const ProposeArgs& p, int slot, size_t recs, hipStream_t st) {
  if (p.rf.generator != GSM_GEN_CHOLESKY) { HIPCHK(h, launch_propose(p, st)); return GSM_OK; }
  CholArgs c{};
  if (int rc = ensure_chol(h, slot, recs, &c)) return rc;
  HIPCHK(h, launch_propose_cholesky(p, c, st));
  return GSM_OK;
}

static ProposeArgs make_propose(gsm_handle h, const gsm_rf_params* rf, int n_steps, int64_t step0, const uint64_t* seeds) {
  ProposeArgs p{};
  p.B = h->B; p.rf = *rf; p.H = h->H; p.W = h->W;
  p.n_chains = h->n_chains; p.n_steps = n_steps; p.step0 = step0; p.seeds = seeds;
  p.centres = h->d_centres.get(); p.n_centres = h->n_centres;
  p.tables = h->d_tables.get(); p.tables_len = h->tables_len; p.tab_max = h->tab_max; p.fy_off = h->d_fy_off.get(); p.g_off = h->d_g_off.get();
  p.lds_sx = h->lds_sx; p.lds_st = h->lds_st; p.lds_x_half = h->lds_x_half; p.lds_tt = h->lds_tt;
  p.k2tab = h->d_k2.get(); p.k2_off = h->d_k2_off.get(); p.mathtab = h->d_mathtab.get();
  p.tab1d = h->d_tab1d.get(); p.t1_off = h->d_t1_off.get();
  p.lds_main = std::max(4 * h->lds_x_half, h->lds_tt);
  p.tiles1_max = h->prop_tiles1; p.tiles2_max = h->prop_tiles;
  // stage 2 split by the parity of kx: on handles whose kernels hold two tile slots per wave (the strip kernels and the stand-alone proposal
  // kernel beside them); GSM_OPT_SPLIT2 = 0 keeps the direct sums (tests/test_gpu_strip.py compares the step kernels of the two families on equal fields)
  p.split2 = (h->use_split2 && strip_for(h)) ? 1 : 0; p.parseval = p.split2;
  return p;
}

extern "C" int gsm_propose_philox(gsm_handle h, int32_t n_steps, int64_t step0, const uint64_t* seeds,
                                  const gsm_rf_params* rf, int32_t* size_idx, int32_t* centre, double* u,
                                  double* fields, int64_t field_stride, double* rf_scalars, void* stream) {
  GSM_GRID_HANDLE(h);
  int rc = check_propose_ready(h, rf, "gsm_propose_philox", true);
  if (rc) return rc;
  if (n_steps < 1 || n_steps > 65535) return fail(h, GSM_E_ARG, "gsm_propose_philox: n_steps must be in [1, 65535]");
  if (!seeds || !size_idx || !centre || !u || !fields) return fail(h, GSM_E_ARG, "gsm_propose_philox: NULL pointer");
  if (field_stride < (int64_t)h->B.max_bh * h->B.max_bw) return fail(h, GSM_E_ARG, "gsm_propose_philox: field_stride too small");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, h->d_scalars[0].ensure((size_t)h->n_chains * n_steps));
  { int rc2 = ensure_k2(h, rf, (hipStream_t)stream); if (rc2) return rc2; }
  ProposeArgs p = make_propose(h, rf, n_steps, step0, seeds);
  p.size_idx = size_idx; p.centre = centre; p.u = u; p.fields = fields; p.field_stride = field_stride;
  p.rf_scalars = rf_scalars; p.scalars = h->d_scalars[0].get();
  return launch_proposals(h, p, 0, (size_t)h->n_chains * n_steps, (hipStream_t)stream);
}

extern "C" int gsm_spectral_from_noise(gsm_handle h, int32_t n_fields, const int32_t* size_idx, const double* rf_scalars,
                                       const gsm_rf_params* rf, const double* noise_re, const double* noise_im,
                                       const double* nugget_field, double* fields, int64_t field_stride, void* stream) {
  GSM_GRID_HANDLE(h);
  gsm_rf_params rfs = rf ? *rf : gsm_rf_params{};      // the spectral generator, whatever rf names
  rfs.generator = GSM_GEN_SPECTRAL;
  int rc = check_propose_ready(h, rf ? &rfs : nullptr, "gsm_spectral_from_noise", false);   // no centre is drawn here
  if (rc) return rc;
  if (n_fields < 1 || n_fields > (1 << 20)) return fail(h, GSM_E_ARG, "gsm_spectral_from_noise: n_fields must be in [1, 2^20]");
  if (!size_idx || !rf_scalars || !noise_re || !noise_im || !fields) return fail(h, GSM_E_ARG, "gsm_spectral_from_noise: NULL pointer");
  if (field_stride < (int64_t)h->B.max_bh * h->B.max_bw) return fail(h, GSM_E_ARG, "gsm_spectral_from_noise: field_stride too small");
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(h, hipSetDevice(h->device));
  std::vector<int32_t> si((size_t)n_fields);
  HIPCHK(h, hipMemcpyAsync(si.data(), size_idx, sizeof(int32_t) * (size_t)n_fields, hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  for (int32_t v : si)
    if (v < 0 || v >= h->B.n_sizes) return fail(h, GSM_E_DEVICE_DATA, "gsm_spectral_from_noise: size index out of range");
  HIPCHK(h, h->d_scalars[0].ensure((size_t)n_fields));
  { int rc2 = ensure_k2(h, &rfs, st); if (rc2) return rc2; }
  ProposeArgs p = make_propose(h, &rfs, n_fields, 0, nullptr);
  p.n_chains = 1;
  p.fields = fields; p.field_stride = field_stride; p.scalars = h->d_scalars[0].get();
  HIPCHK(h, launch_spectral_from_noise(p, size_idx, rf_scalars, noise_re, noise_im, nugget_field, st));
  return GSM_OK;
}

extern "C" int gsm_run_noise(gsm_handle h, int32_t n_steps, void* beds, void* energy, uint32_t* resampled, double* loss_sum,
                             const int32_t* size_idx, const int32_t* centre, const double* u, const double* rf_scalars,
                             const gsm_rf_params* rf, const double* noise_re, const double* noise_im, const double* nugget_field,
                             int64_t field_stride, double* loss, uint8_t* accept, void* stream) {
  GSM_GRID_HANDLE(h);
  if (!h->have_static) return fail(h, GSM_E_STATE, "gsm_run_noise: call gsm_set_static first");
  gsm_rf_params rfs = rf ? *rf : gsm_rf_params{};
  rfs.generator = GSM_GEN_SPECTRAL;
  int rc = check_propose_ready(h, rf ? &rfs : nullptr, "gsm_run_noise", false);             // the centres arrive with the draws
  if (rc) return rc;
  if (!strip_for(h)) return fail(h, GSM_E_UNSUPPORTED, "gsm_run_noise: this block table does not go to the strip kernels (gsm_strip_active); "
                                                       "use gsm_spectral_from_noise + gsm_run_replay");
  if (n_steps < 0 || n_steps > 65535) return fail(h, GSM_E_ARG, "gsm_run_noise: n_steps must be in [0, 65535]");
  if (n_steps == 0) return GSM_OK;
  if (!beds || !energy || !resampled || !loss_sum || !size_idx || !centre || !u || !rf_scalars || !noise_re || !noise_im || !loss || !accept)
    return fail(h, GSM_E_ARG, "gsm_run_noise: NULL pointer");
  if (field_stride < (int64_t)h->B.max_bh * h->B.max_bw) return fail(h, GSM_E_ARG, "gsm_run_noise: field_stride smaller than the largest block");
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, h->d_scalars[0].ensure((size_t)h->n_chains * n_steps));
  { int rc2 = ensure_k2(h, &rfs, st); if (rc2) return rc2; }
  FusedArgs fa{};
  fa.T = make_step(h, n_steps, beds, energy, resampled, loss_sum, loss, accept, nullptr);      // strip_for(h) was checked above
  fa.P = make_propose(h, &rfs, n_steps, 0, nullptr);
  fa.P.scalars = h->d_scalars[0].get();
  fa.noise_re = noise_re; fa.noise_im = noise_im; fa.noise_nug = nugget_field; fa.noise_stride = field_stride;
  HIPCHK(h, launch_noise_chain_scalars(fa.P, size_idx, centre, u, rf_scalars, h->d_err.get(), st));
  HIPCHK(h, launch_chain_strip_noise(fa, st));
  HIPCHK(h, launch_resampled_from_records(fa, st));
  return check_device_flag(h, st, "gsm_run_noise");
}

extern "C" int gsm_last_run_fused(gsm_handle h) { return h ? h->last_fused : GSM_E_ARG; }

extern "C" int gsm_enable_timing(gsm_handle h, int32_t on) {
  GSM_GRID_HANDLE(h);
  h->timing = on != 0;
  return GSM_OK;
}

extern "C" int gsm_last_timing(gsm_handle h, double* step_ms, int32_t* step_launches, double* prop_ms, int32_t* prop_launches) {
  GSM_GRID_HANDLE(h);
  if (step_ms) *step_ms = h->n_step_launch ? h->t_step_ms / h->n_step_launch : 0.0;
  if (step_launches) *step_launches = h->n_step_launch;
  if (prop_ms) *prop_ms = h->n_prop_launch ? h->t_prop_ms / h->n_prop_launch : 0.0;
  if (prop_launches) *prop_launches = h->n_prop_launch;
  return GSM_OK;
}

// timing events of one gsm_run_philox call, PER for each launch group: (step start, step stop), behind (proposal start, proposal stop)
// when PER is 4.  No events unless gsm_enable_timing is on; they are destroyed on every path out of the call.
template <int PER>
struct RunTimer {
  std::vector<Event> ev;
  hipError_t start(gsm_handle h, int groups) {
    if (h->timing) ev.resize((size_t)PER * groups);
    for (Event& e : ev)
      if (hipError_t err = e.ensure(hipEventDefault)) return err;
    return hipSuccess;
  }
  hipError_t mark(int group, int i, hipStream_t st) { return ev.empty() ? hipSuccess : hipEventRecord(ev[(size_t)PER * group + i].get(), st); }
  void finish(gsm_handle h) {                   // after the streams have drained
    if (ev.empty()) return;
    h->t_step_ms = h->t_prop_ms = 0;
    h->n_step_launch = h->n_prop_launch = 0;
    float ms = 0;
    for (size_t g = 0; g < ev.size(); g += PER) {
      if (PER == 4 && hipEventElapsedTime(&ms, ev[g].get(), ev[g + 1].get()) == hipSuccess) { h->t_prop_ms += ms; h->n_prop_launch++; }
      if (hipEventElapsedTime(&ms, ev[g + PER - 2].get(), ev[g + PER - 1].get()) == hipSuccess) { h->t_step_ms += ms; h->n_step_launch++; }
    }
  }
};

// the (size_idx, centre, u) records of a scratch slot, with the proposal fields when field_doubles > 0
static int alloc_scratch(gsm_handle h, gsm_context::Scratch& s, size_t recs, size_t field_doubles) {
  s = gsm_context::Scratch();                  // recs stays 0 until every buffer of the slot exists
  HIPCHK(h, s.size_idx.ensure(recs));
  HIPCHK(h, s.centre.ensure(recs * 2));
  HIPCHK(h, s.u.ensure(recs));
  if (field_doubles) HIPCHK(h, s.fields.ensure(field_doubles));
  s.recs = recs;
  return GSM_OK;
}

// Spectral generator: fused launches (chain_fused_kernel.hip) -- proposals are generated and consumed on the CU, no field scratch, no
// second stream.  Segments of at most seg_max steps: the per-(chain, step) scalar records (120 + 20 bytes) are sized by the
// segment, not by the call, and a long call is a sequence of bounded launches on the caller's stream.  Counters are
// functions of the absolute step, so the split is invisible in the results (test_fused_internal_segments...).
static int run_philox_fused(gsm_handle h, FusedArgs& fa, int seg_max, int32_t n_steps, int64_t step0, const uint64_t* seeds,
                            const gsm_rf_params* rf, hipStream_t st) {
  StepArgs& a = fa.T;
  const size_t recs1 = (size_t)h->n_chains * seg_max;
  HIPCHK(h, h->d_scalars[0].ensure(recs1));
  // the scalars kernel also writes (size_idx, centre, u) records: give it the scalar-sized scratch of slot 1
  auto& sc = h->scr[1];
  if (sc.recs < recs1 || sc.fields.get())
    if (int rc = alloc_scratch(h, sc, recs1, 0)) return rc;
  const int n_seg = (n_steps + seg_max - 1) / seg_max;
  RunTimer<2> tm;
  HIPCHK(h, tm.start(h, n_seg));
  for (int k = 0; k < n_seg; ++k) {
    const int off = k * seg_max;
    const int ns = std::min(seg_max, n_steps - off);
    a.n_steps = ns; a.in_stride = ns; a.rec_offset = off;
    fa.P = make_propose(h, rf, ns, step0 + off, seeds);
    fa.P.scalars = h->d_scalars[0].get();
    fa.P.size_idx = sc.size_idx.get(); fa.P.centre = sc.centre.get(); fa.P.u = sc.u.get();
    HIPCHK(h, launch_propose_scalars(fa.P, st));
    HIPCHK(h, tm.mark(k, 0, st));
    HIPCHK(h, launch_chain_fused(fa, st));
    HIPCHK(h, tm.mark(k, 1, st));
  }
  const int rc = check_device_flag(h, st, "gsm_run_philox");
  tm.finish(h);
  return rc;
}

// The two-kernel pipeline (the Cholesky generator, GSM_OPT_FUSED = 0 and block tables beyond the fused kernel's LDS budget): the proposals
// of batch k + 1 are generated on the handle's second stream while the caller's stream steps through batch k; two scratch slots.
static int run_philox_pipelined(gsm_handle h, int32_t n_steps, int64_t step0, int32_t batch, const uint64_t* seeds, const gsm_rf_params* rf,
                                void* beds, void* energy, uint32_t* resampled, double* loss_sum, double* loss, uint8_t* accept,
                                int32_t* blocks, hipStream_t st) {
  const size_t recs = (size_t)h->n_chains * batch;
  for (auto& s : h->scr)
    if (!(s.recs >= recs && s.fields.get()))
      if (int rc = alloc_scratch(h, s, recs, recs * (size_t)h->field_stride)) return rc;
  for (int i = 0; i < 2; ++i) HIPCHK(h, h->d_scalars[i].ensure(recs));
  HIPCHK(h, h->aux.ensure(hipStreamNonBlocking));
  for (int i = 0; i < 2; ++i) {
    HIPCHK(h, h->ev_prop[i].ensure(hipEventDisableTiming));
    HIPCHK(h, h->ev_step[i].ensure(hipEventDisableTiming));
  }
  const hipStream_t aux = h->aux.get();
  const int n_batches = (n_steps + batch - 1) / batch;
  RunTimer<4> tm;
  HIPCHK(h, tm.start(h, n_batches));
  // order the aux stream behind everything already queued on the caller's stream (seeds upload etc.)
  HIPCHK(h, hipEventRecord(h->ev_step[0].get(), st));
  HIPCHK(h, hipStreamWaitEvent(aux, h->ev_step[0].get(), 0));

  auto issue_propose = [&](int k) -> int {
    const int nb = std::min(batch, n_steps - k * batch);
    auto& s = h->scr[k & 1];
    if (k >= 2) HIPCHK(h, hipStreamWaitEvent(aux, h->ev_step[k & 1].get(), 0));  // buffer free again
    ProposeArgs p = make_propose(h, rf, nb, step0 + (int64_t)k * batch, seeds);
    p.size_idx = s.size_idx.get(); p.centre = s.centre.get(); p.u = s.u.get(); p.fields = s.fields.get(); p.field_stride = h->field_stride;
    p.rf_scalars = nullptr; p.scalars = h->d_scalars[k & 1].get();
    HIPCHK(h, tm.mark(k, 0, aux));
    if (int rc2 = launch_proposals(h, p, k & 1, recs, aux)) return rc2;
    HIPCHK(h, tm.mark(k, 1, aux));
    HIPCHK(h, hipEventRecord(h->ev_prop[k & 1].get(), aux));
    return GSM_OK;
  };

  int rc = issue_propose(0);
  if (rc) return rc;
  for (int k = 0; k < n_batches; ++k) {
    if (k + 1 < n_batches) { rc = issue_propose(k + 1); if (rc) return rc; }
    const int nb = std::min(batch, n_steps - k * batch);
    auto& s = h->scr[k & 1];
    HIPCHK(h, hipStreamWaitEvent(st, h->ev_prop[k & 1].get(), 0));
    StepArgs a = make_step(h, nb, beds, energy, resampled, loss_sum, loss, accept, blocks);
    a.size_idx = s.size_idx.get(); a.centre = s.centre.get(); a.u = s.u.get(); a.fields = s.fields.get(); a.field_stride = h->field_stride;
    a.rec_stride = n_steps; a.rec_offset = (int64_t)k * batch;
    HIPCHK(h, tm.mark(k, 2, st));
    HIPCHK(h, launch_step(a, st));
    HIPCHK(h, tm.mark(k, 3, st));
    HIPCHK(h, hipEventRecord(h->ev_step[k & 1].get(), st));
  }
  rc = check_device_flag(h, st, "gsm_run_philox");
  HIPCHK(h, hipStreamSynchronize(aux));
  tm.finish(h);
  return rc;
}

extern "C" int gsm_run_philox(gsm_handle h, int32_t n_steps, int64_t step0, int32_t batch, const uint64_t* seeds,
                              const gsm_rf_params* rf, void* beds, void* energy, uint32_t* resampled, double* loss_sum,
                              double* loss, uint8_t* accept, int32_t* blocks, void* stream) {
  GSM_GRID_HANDLE(h);
  if (!h->have_static) return fail(h, GSM_E_STATE, "gsm_run_philox: call gsm_set_static first");
  int rc = check_propose_ready(h, rf, "gsm_run_philox", true);
  if (rc) return rc;
  if (n_steps < 0) return fail(h, GSM_E_ARG, "gsm_run_philox: n_steps < 0");
  if (n_steps == 0) return GSM_OK;
  if (batch < 1 || batch > 65535) return fail(h, GSM_E_ARG, "gsm_run_philox: batch must be in [1, 65535]");
  if (!seeds || !beds || !energy || !resampled || !loss_sum || !loss || !accept) return fail(h, GSM_E_ARG, "gsm_run_philox: NULL pointer");
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(h, hipSetDevice(h->device));
  if (batch > n_steps) batch = n_steps;
  if ((rc = ensure_k2(h, rf, st))) return rc;
  // one fused launch per segment where the generator and the block table allow it; GSM_OPT_FUSED = 0 keeps the two-kernel pipeline
  h->last_fused = 0;
  if (h->use_fused && rf->generator == GSM_GEN_SPECTRAL) {
    const int seg_max = std::min(n_steps, h->fused_segment);
    FusedArgs fa{};
    fa.T = make_step(h, seg_max, beds, energy, resampled, loss_sum, loss, accept, blocks);
    fa.T.rec_stride = n_steps;
    fa.P = make_propose(h, rf, seg_max, step0, seeds);
    if (fused_supported(fa)) {
      h->last_fused = 1;
      return run_philox_fused(h, fa, seg_max, n_steps, step0, seeds, rf, st);
    }
  }
  return run_philox_pipelined(h, n_steps, step0, batch, seeds, rf, beds, energy, resampled, loss_sum, loss, accept, blocks, st);
}

int gsm::ensure_pcg_tables(gsm_handle h) {
  if (h->d_pcg_tab.get()) return GSM_OK;
  std::vector<uint64_t> tab(kPcgJumpWords + 768);
  const uint64_t* zig = nullptr;
  pcg64_host_tables(tab.data(), &zig);
  memcpy(tab.data() + kPcgJumpWords, zig, 768 * sizeof(uint64_t));
  HIPCHK(h, h->d_pcg_tab.ensure(tab.size()));
  HIPCHK(h, hipMemcpy(h->d_pcg_tab.get(), tab.data(), tab.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
  return GSM_OK;
}

extern "C" int gsm_draw_pcg64(gsm_handle h, int32_t n_steps, const gsm_rf_params* rf, uint64_t* rf_state, uint64_t* chain_state,
                              const uint8_t* region_mask, int32_t* size_idx, int32_t* centre, double* u, double* rf_scalars,
                              double* noise_re, double* noise_im, double* nugget_field, int64_t field_stride, void* stream) {
  GSM_GRID_HANDLE(h);
  if (!h->have_blocks) return fail(h, GSM_E_STATE, "gsm_draw_pcg64: call gsm_set_blocks first");
  if (!rf || !rf_state || !chain_state || !size_idx || !centre || !u || !rf_scalars || !noise_re || !noise_im)
    return fail(h, GSM_E_ARG, "gsm_draw_pcg64: NULL pointer");
  if (n_steps < 1) return fail(h, GSM_E_ARG, "gsm_draw_pcg64: n_steps must be >= 1");
  if (field_stride < (int64_t)h->B.max_bh * h->B.max_bw) return fail(h, GSM_E_ARG, "gsm_draw_pcg64: field_stride too small");
  if (rf->nugget_max > 0.0 && !nugget_field) return fail(h, GSM_E_ARG, "gsm_draw_pcg64: nugget_max > 0 needs nugget_field");
  if (h->B.n_sizes < 1 || (int64_t)h->H >= 0xFFFFFFFFll) return fail(h, GSM_E_ARG, "gsm_draw_pcg64: bad block table / grid");
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(h, hipSetDevice(h->device));
  { int rc = ensure_pcg_tables(h); if (rc) return rc; }
  PcgDrawArgs a{};
  a.H = h->H; a.W = h->W; a.n_chains = h->n_chains; a.n_steps = n_steps; a.n_sizes = h->B.n_sizes; a.rf = *rf;
  a.bh = h->B.bh; a.bw = h->B.bw; a.rf_state = rf_state; a.ch_state = chain_state; a.region_mask = region_mask;
  a.jump = h->d_pcg_tab.get(); a.zig = h->d_pcg_tab.get() + kPcgJumpWords;
  a.size_idx = size_idx; a.centre = centre; a.u = u; a.rf_scalars = rf_scalars;
  a.noise_re = noise_re; a.noise_im = noise_im; a.nugget = (rf->nugget_max > 0.0) ? nugget_field : nullptr; a.field_stride = field_stride;
  a.err = h->d_err.get();
  HIPCHK(h, launch_pcg64_draw(a, st));
  return GSM_OK;          // asynchronous: a chain that finds no centre inside region_mask raises the handle's device flag,
                          // reported by the next gsm_run_replay (which would also reject the out-of-range record)
}
