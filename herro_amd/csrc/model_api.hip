// model_api.hip — the model of the C ABI (include/herro_amd.h): herro_load_model (device stage; the host stage is model_pack.h), the precision modes and
// their calibration gate, the activation scratch and the sibling-tile buffers, how a precision mode runs a launch (run_model, launch_cfg), the stand-alone
// herro_model_forward, and the model's test hooks.  Host C++ (compiled by hipcc) over model.hip and model_h.hip; the launch plan is infer_plan.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "api_job.h"
#include "model_dev.h"
#include "model_pack.h"

using namespace herro;

// How a precision mode (herro_set_precision, 0 .. 8) runs a launch, stated once for run_model and launch_cfg:
//
//   mode  operands                        tiled launch (the fused stack)      untiled launch (layer by layer)
//   0     f32 MFMA                        -                                   launch_model, precision 0
//   1     bf16 hi/lo, three terms         launch_model, precision 1           launch_model, precision 3 (bf16x3)
//   2, 3  (A/B: 3 is bf16x3 unfused)      -                                   launch_model, precision 2 / 3
//   4     f16, two terms                  launch_model_h, terms 2             launch_model, precision 3
//   5     f16, one term                   launch_model_h, terms 1             "
//   6     f16 + an e4m3 remainder term    launch_model_h, terms 3             "
//   7     proj two terms, FF one          launch_model_h, terms 21            "
//   8     proj one term, FF two           launch_model_h, terms 12            "
//
// fused: the plan may tile the windows that fit a tile (LaunchCfg::fused); a mode without a fused stack gets untiled launches only.
// terms: of launch_model_h (model_dev.h) for a tiled launch; 0: the mode runs on model.hip alone.  flat: launch_model's precision for an untiled launch.
namespace {
struct ModeRun { bool fused; int terms; int flat; };
ModeRun mode_run(int p) {
  static const int terms[9] = {0, 0, 0, 0, 2, 1, 3, 21, 12};
  const bool fused = p == 1 || p >= 4;
  return ModeRun{fused, terms[p], fused ? 3 : p};
}
}  // namespace

// Most informative rows of a window that stays on the fused stack: 64 (one tile), or 64 * FUSED_MAX_SIB with the f16 stack, which
// spreads a larger window over sibling tiles (HERRO_FUSED_BIG=0: such windows go layer by layer as before, for A/B).
uint32_t fused_tok_cap(const herro_ctx* ctx) {
  static const bool big = ab_env("HERRO_FUSED_BIG", 1) != 0;
  return (big && ctx->precision >= 4 && model_h_supported(ctx->M)) ? FUSED_MAX_TOK * FUSED_MAX_SIB : FUSED_MAX_TOK;
}
// K / V exchange buffers and flags of `n_tiles_b` sibling tiles (128 KB per tile)
int ensure_sib(herro_ctx* ctx, uint32_t n_tiles_b) {
  if (n_tiles_b <= ctx->sib_cap) return HERRO_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->sib_kv) (void)hipFree(ctx->sib_kv);
  if (ctx->sib_flag) (void)hipFree(ctx->sib_flag);
  ctx->sib_kv = nullptr; ctx->sib_flag = nullptr; ctx->sib_cap = 0;
  const uint32_t cap = n_tiles_b + n_tiles_b / 2 + 8;
  if (hipMalloc(&ctx->sib_kv, (size_t)cap * 2 * 8 * 8 * 64 * 16) != hipSuccess || hipMalloc(&ctx->sib_flag, ((size_t)cap + 1) * 4) != hipSuccess ||
      hipMemsetAsync(ctx->sib_flag, 0, ((size_t)cap + 1) * 4, ctx->stream) != hipSuccess) {   // on the stream of the launches that read the flags: in front of them by stream order (a memset on the null stream is not ordered with a non-blocking stream, and may return before it has run)
    if (ctx->sib_kv) (void)hipFree(ctx->sib_kv);
    ctx->sib_kv = nullptr;
    ctx->err = "out of device memory for the sibling-tile buffers";
    return HERRO_E_NO_DEVICE;
  }
  ctx->sib_cap = cap;
  ctx->S.sib_kv = (uint16_t*)ctx->sib_kv;
  ctx->S.sib_flag = (uint32_t*)ctx->sib_flag;
  ctx->S.sib_err = (uint32_t*)ctx->sib_flag + cap;
  return HERRO_OK;
}
// The error word of the sibling tiles, read where logits / corrected bases come back to the host (settle_model has synchronised the stream: every model pass queued
// so far is complete).  The word carries no job identity, so a raised word taints EVERY job whose sibling-tile pass has not been seen clean yet (ctx->sib_suspects): all of
// them are marked stale and each repeats its pass when it is fetched (sib_retry) — the fetch that finds the word is not necessarily the job that owned the stale keys
// (with two inferred jobs in flight the first fetch used to repeat ITS pass, clear the word, and the other job's fetch then returned invalid logits).  A job
// whose pass launched no sibling tiles cannot be affected and is served.  job == nullptr: the stand-alone forward, which is its own suspect.
static int check_sib(herro_ctx* ctx, herro_job* job) {
  if (!ctx->sib_flag) return HERRO_OK;
  uint32_t e = 0;
  HIP_TRY(ctx, hipMemcpyAsync(&e, (uint32_t*)ctx->sib_flag + ctx->sib_cap, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (e) {
    for (herro_job* j : ctx->sib_suspects) j->sib_stale = true;
    (void)hipMemsetAsync((uint32_t*)ctx->sib_flag + ctx->sib_cap, 0, 4, ctx->stream);   // reported (to its suspects): the context stays usable
  }
  ctx->sib_suspects.clear();   // clean, or marked
  if (job ? job->sib_stale : e != 0) {
    ctx->err = "fused stack: a sibling tile of a window above 64 informative rows never published its keys" + (e ? " (layer " + std::to_string(e - 1) + ")" : std::string()) + "; logits invalid";
    return HERRO_E_STATE;
  }
  return HERRO_OK;
}

// Settling the model passes queued so far, before anybody reads what they wrote: the stream goes idle, the kernel timer takes its events in, and the sibling
// tiles' error word is looked at — job's pass is clean (HERRO_OK) or not to be trusted (check_sib's code).  This half repeats nothing: settle_pass
// (job_run.hip) repeats a job's pass once on top of it; the stand-alone forward (job == nullptr) has no repeat.
int settle_model(herro_ctx* ctx, herro_job* job) {
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->timer.collect();
  return check_sib(ctx, job);
}

// One launch of the model on the context's stream, by the mode's row of the table above
void run_model(herro_ctx* ctx, const BatchDev& B, bool tiled) {
  if (B.n_tok == 0) return;
  const ModeRun m = mode_run(ctx->precision);
  const uint32_t cu = ctx->front_cu ? ctx->front_cu : ctx->n_cu;   // the front end's own count (herro_debug_set_front_cu); the tile plan took ctx->n_cu
  if (tiled && m.terms) launch_model_h(ctx->M, B, ctx->S, m.terms, ctx->stream, &ctx->timer, cu, ctx->conv_fc, &ctx->front_ran);
  else launch_model(ctx->M, B, ctx->S, tiled ? ctx->precision : m.flat, ctx->stream, &ctx->timer, cu, &ctx->front_ran);
}

// The arrays of one launch inside the descriptor image at d_image (build_launch); the caller adds the buffers the launch reads and writes.
BatchDev batch_dev(const void* d_image, const LaunchOffs& o) {
  const unsigned char* base = (const unsigned char*)d_image;
  auto u32 = [&](size_t off) { return (const uint32_t*)(base + off); };
  auto u64 = [&](size_t off) { return off == NO_ARRAY ? nullptr : (const uint64_t*)(base + off); };
  BatchDev B{};
  B.n_win = o.n_win; B.n_tok = o.n_tok; B.max_win_tok = o.max_win_tok;
  B.plane_off = u64(o.plane_off); B.plane_ld = u32(o.plane_ld); B.len = u32(o.len); B.lmax = u32(o.lmax); B.tok_off = u32(o.tok_off);
  B.sup_off = u64(o.sup_off); B.out_off = u64(o.out_off); B.rf_base = u64(o.rf_base);
  B.n_tiles = o.n_tiles; B.tile_tok0 = u32(o.tiles);
  B.n_tiles_q = o.n_tiles_q; B.tile_tok0_q = u32(o.tiles_q);
  B.n_tiles_b = o.n_tiles_b; B.tile_tok0_b = u32(o.tiles_b); B.tile_grp = u32(o.grp);
  return B;
}
LaunchCfg launch_cfg(const herro_ctx* ctx, uint32_t fused_rows, bool with_rf_base) {
  const ModeRun m = mode_run(ctx->precision);
  return LaunchCfg{m.fused, fused_rows, ctx->tile_packing, m.terms ? model_h_half_tiles(ctx->M) : 0, ctx->n_cu, with_rf_base};
}

int ensure_scratch(herro_ctx* ctx, uint32_t n_tok) {
  if (n_tok <= ctx->scratch_cap) return HERRO_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  free_all(ctx->scratch_allocs);
  const ModelHyper& h = ctx->M.h;
  const uint64_t cap = (uint64_t)n_tok + n_tok / 4 + 256;
  ModelScratch S{};
  auto A = [&](uint64_t bytes) -> void* {
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
    ctx->scratch_allocs.push_back(p);
    return p;
  };
  S.tok_win = (uint32_t*)A(cap * 4);
  S.tok_row = (uint32_t*)A(cap * 4);
  S.tok_out = (uint64_t*)A(cap * 8);
  S.tok_meta = (TokMeta*)A(cap * sizeof(TokMeta));
  S.tok_cv = (TokCv*)A(cap * sizeof(TokCv));
  S.y1 = (float*)A(cap * HERRO_ROWS * h.kw * h.c1 * 4);
  S.y2 = (float*)A(cap * HERRO_ROWS * h.c2 * 4);
  S.x = (float*)A(cap * h.d_model * 4);
  S.hbuf = (float*)A(cap * h.d_model * 4);
  S.qkv = (float*)A(cap * 3 * h.d_model * 4);
  S.att = (float*)A(cap * h.d_model * 4);
  S.ff = (float*)A(cap * h.d_ff * 4);
  S.logits = (float*)A(cap * 16 * 4);
  S.y1_hi = (uint16_t*)A(cap * HERRO_ROWS * h.kw * h.c1 * 2); S.y1_lo = (uint16_t*)A(cap * HERRO_ROWS * h.kw * h.c1 * 2);
  S.y2_hi = (uint16_t*)A(cap * HERRO_ROWS * h.c2 * 2); S.y2_lo = (uint16_t*)A(cap * HERRO_ROWS * h.c2 * 2);
  S.h_hi = (uint16_t*)A(cap * h.d_model * 2); S.h_lo = (uint16_t*)A(cap * h.d_model * 2);
  S.att_hi = (uint16_t*)A(cap * h.d_model * 2); S.att_lo = (uint16_t*)A(cap * h.d_model * 2);
  S.ff_hi = (uint16_t*)A(cap * h.d_ff * 2); S.ff_lo = (uint16_t*)A(cap * h.d_ff * 2);
  if (!S.y1_hi || !S.y1_lo || !S.y2_hi || !S.y2_lo || !S.h_hi || !S.h_lo || !S.att_hi || !S.att_lo || !S.ff_hi || !S.ff_lo ||!S.tok_win || !S.tok_row || !S.tok_out || !S.tok_meta || !S.tok_cv || !S.y1 || !S.y2 || !S.x || !S.hbuf || !S.qkv || !S.att || !S.ff || !S.logits) {
    free_all(ctx->scratch_allocs);
    ctx->scratch_cap = 0;
    ctx->err = "out of device memory for model scratch (" + std::to_string(cap) + " tokens)";
    return HERRO_E_NO_DEVICE;
  }
  S.sib_kv = ctx->S.sib_kv; S.sib_flag = ctx->S.sib_flag; S.sib_err = ctx->S.sib_err;   // ensure_sib's, sized on their own
  ctx->S = S;
  ctx->scratch_cap = (uint32_t)cap;
  return HERRO_OK;
}

// ---- model ---------------------------------------------------------------------------------------
// Calibration of the f16 modes on the loaded model: 4 windows x 96 rows, 64 informative rows each (fused tiles), pileup-shaped — a target column, 30 read
// columns that cover a stretch of the window on one strand and agree with the target but for ~3 % mismatches and ~2 % gaps, '.' outside their stretch,
// insertion rows ('*' in the target, a base in a fifth of the reads), qualities ~N(22, 8).  Reference = mode 0 (f32 MFMA).  Fills ctx->calib[mode] for the
// listed modes with max |logit(mode) - logit(mode 0)| (inf when the run fails or is not finite); ctx->precision is restored.
static int calibrate(herro_ctx* ctx, const int* modes, int n_modes) {
  const uint32_t B = 4, L = 96, NS = 64;
  std::vector<uint8_t> cb((size_t)B * L * HERRO_ROWS), cq(cb.size());
  uint64_t x = 0x9E3779B97F4A7C15ull;
  auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
  auto uni = [&]() { return (double)(rnd() >> 11) * (1.0 / 9007199254740992.0); };
  for (uint32_t b = 0; b < B; b++) {
    std::vector<uint8_t> truth(L);
    for (uint32_t r = 0; r < L; r++) truth[r] = uni() < 0.08 ? 4 : (uint8_t)(rnd() & 3);   // 4: an insertion row ('*' in the target)
    for (uint32_t c = 0; c < HERRO_ROWS; c++) {
      const uint32_t strand = c ? (uint32_t)(rnd() & 1) : 0u, gap = 4 + 5 * strand;
      const uint32_t lo = c && uni() < 0.3 ? (uint32_t)(uni() * 30) : 0u, hi = c && uni() < 0.3 ? L - (uint32_t)(uni() * 30) : L;
      for (uint32_t r = 0; r < L; r++) {
        uint8_t tok;
        if (r < lo || r >= hi) tok = TOK_NONE;
        else if (c == 0) tok = truth[r];
        else if (truth[r] == 4) tok = uni() < 0.2 ? (uint8_t)((rnd() & 3) + 5 * strand) : (uint8_t)gap;
        else { const double u = uni(); tok = u < 0.95 ? (uint8_t)(truth[r] + 5 * strand) : (u < 0.98 ? (uint8_t)(((truth[r] + 1 + (rnd() % 3)) & 3) + 5 * strand) : (uint8_t)gap); }
        double g = 0; for (int k = 0; k < 12; k++) g += uni();   // ~N(6, 1)
        const double q = std::min(50.0, std::max(2.0, std::floor(22.0 + 8.0 * (g - 6.0) + 0.5)));
        const bool has_q = tok != TOK_NONE && tok != gap && tok != 4;
        const size_t i = ((size_t)b * L + r) * HERRO_ROWS + c;
        cb[i] = tok; cq[i] = has_q ? (uint8_t)(33 + q) : (uint8_t)33;
      }
    }
  }
  std::vector<int32_t> lens(B, (int32_t)NS), idx((size_t)B * NS);
  for (uint32_t b = 0; b < B; b++) for (uint32_t k = 0; k < NS; k++) idx[(size_t)b * NS + k] = (int32_t)(16 + k);
  std::vector<float> i1((size_t)B * NS), b1((size_t)B * NS * 5), i4(i1.size()), b4(b1.size());
  const int keep = ctx->precision;
  ctx->precision = 0;
  const int rc = herro_model_forward(ctx, B, L, cb.data(), cq.data(), lens.data(), idx.data(), i1.data(), b1.data());
  if (rc != HERRO_OK) { ctx->precision = keep; return rc; }
  for (int m = 0; m < n_modes; m++) {
    const int mode = modes[m];
    if (mode < 4 || mode > 8) continue;
    ctx->precision = mode;
    float err = INFINITY;
    if ((mode != 6 || model_h_f8_supported(ctx->M)) && herro_model_forward(ctx, B, L, cb.data(), cq.data(), lens.data(), idx.data(), i4.data(), b4.data()) == HERRO_OK) {
      err = 0.f;
      bool finite = true;
      for (size_t i = 0; i < i1.size(); i++) { finite = finite && std::isfinite(i4[i]); err = std::max(err, std::fabs(i4[i] - i1[i])); }
      for (size_t i = 0; i < b1.size(); i++) { finite = finite && std::isfinite(b4[i]); err = std::max(err, std::fabs(b4[i] - b1[i])); }
      if (!finite) err = INFINITY;
    }
    ctx->calib[mode] = err;
  }
  ctx->precision = keep;
  return HERRO_OK;
}

// The gate of the f16 modes (4 .. 8) on the loaded model, stated once for herro_load_model and herro_set_precision.  A mode exists when the f16 stack serves
// the model's shapes, every weight lies inside the f16 range (|w| >= 65520 rounds to inf, the remainder term to -inf: NaN logits) and, for mode 6, the e4m3
// copies are there; because the margin of the f16 formats to the 1e-3 contract was measured on random-init weights only, it is then held to a calibration
// run on THIS model (ctx->calib[mode]; run here unless `measure` is off or the value is already there): within half the contract of mode 0.
// forced: HERRO_FORCE_PRECISION=1 (A/B builds) or herro_debug_force_precision keep a mode that missed the bound, for measurements.
struct F16Gate {
  bool shapes, range, f8;
  int rc = HERRO_OK;      // of the calibration run, where one was needed
  bool within = false;
  bool forced;
  bool available() const { return shapes && range && f8; }
};
static F16Gate f16_gate(herro_ctx* ctx, int mode, bool measure = true) {
  static const bool env_force = ab_env("HERRO_FORCE_PRECISION", 0) != 0;
  F16Gate g;
  g.shapes = model_h_supported(ctx->M);
  g.range = ctx->wmax < 65504.f;
  g.f8 = mode != 6 || model_h_f8_supported(ctx->M);
  g.forced = env_force || ctx->debug_force_precision;
  if (!g.available()) return g;
  if (measure && ctx->calib[mode] < 0.f) g.rc = calibrate(ctx, &mode, 1);
  g.within = g.rc == HERRO_OK && ctx->calib[mode] <= 5e-4f;
  return g;
}

// Device stage of herro_load_model: every blob of the host form (model_pack.h) to the device, M's pointers from their places, the PE table.  Returns with
// the stream idle — until then hm, which the copies read, must live.  allocs: what the caller frees on failure and keeps with the model otherwise.
static int upload_model(herro_ctx* ctx, const HostModel& hm, ModelDev& M, std::vector<void*>& allocs) {
  std::vector<void*> dev(hm.blobs.size(), nullptr);
  for (size_t i = 0; i < dev.size(); i++) {
    const Blob& b = hm.blobs[i];
    HIP_TRY(ctx, hipMalloc(&dev[i], std::max<size_t>(b.bytes, 1)));
    allocs.push_back(dev[i]);
    if (b.bytes) HIP_TRY(ctx, hipMemcpyAsync(dev[i], b.p, b.bytes, hipMemcpyHostToDevice, ctx->stream));
  }
  auto f32 = [&](int i) { return i < 0 ? nullptr : (const float*)dev[i]; };
  auto u16 = [&](int i) { return i < 0 ? nullptr : (const uint16_t*)dev[i]; };
  auto weight = [&](const HostWeight& w) {
    Weight d;
    d.K = w.K; d.N = w.N; d.s8 = w.s8;
    d.f32 = f32(w.blob[W_F32]); d.bias = f32(w.blob[W_BIAS]);
    d.hi = u16(w.blob[W_HI]); d.lo = u16(w.blob[W_LO]); d.phi = u16(w.blob[W_PHI]); d.plo = u16(w.blob[W_PLO]);
    d.h16 = u16(w.blob[W_H16]); d.l16 = u16(w.blob[W_L16]); d.ph16 = u16(w.blob[W_PH16]);
    d.p8 = w.blob[W_P8] < 0 ? nullptr : (const uint8_t*)dev[w.blob[W_P8]];
    return d;
  };
  M = ModelDev{};
  M.h = hm.file.h;
  M.t1 = f32(hm.t1); M.wq1 = f32(hm.wq1); M.b1 = f32(hm.b1); M.pe_div = f32(hm.pe_div);
  M.conv1g = weight(hm.conv1g); M.conv2 = weight(hm.conv2); M.fc = weight(hm.fc); M.heads = weight(hm.heads);
  for (uint32_t l = 0; l < M.h.n_layers; l++) {
    const HostLayer& y = hm.layer[l];
    M.layer[l].ln1_g = f32(y.ln1_g); M.layer[l].ln1_b = f32(y.ln1_b); M.layer[l].ln2_g = f32(y.ln2_g); M.layer[l].ln2_b = f32(y.ln2_b);
    M.layer[l].qkv = weight(y.qkv); M.layer[l].proj = weight(y.proj); M.layer[l].ff1 = weight(y.ff1); M.layer[l].ff2 = weight(y.ff2);
  }
  M.lnf_g = f32(hm.lnf_g); M.lnf_b = f32(hm.lnf_b);
  M.act = hm.act; M.norm_first = hm.norm_first; M.pe_kind = hm.pe_kind; M.final_norm = hm.final_norm;
  M.pe_learned = f32(hm.pe_learned); M.pe_learned_rows = hm.pe_learned_rows;
  if (model_h_supported(M)) {   // the positional encoding of rows 0 .. 16383 (a 4096-base window has ~4700 rows, an 8192-base one ~9500), 16 MB; k_layers_p computes the rows beyond it itself
    const uint32_t rows = 16384;
    float* tab = nullptr;
    if (hipMalloc(&tab, (size_t)rows * M.h.d_model * 4) == hipSuccess) {
      allocs.push_back(tab);
      launch_pe_table(M.pe_div, tab, rows, M.h.d_model, ctx->stream);
      M.pe_tab = tab;
      M.pe_rows = rows;
    } else (void)hipGetLastError();
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return HERRO_OK;
}

// Operand format of the model just loaded.  bf16 hi/lo x3 (mode 1, ~1e-5) always works; an f16 mode has to pass f16_gate.
static void choose_precision(herro_ctx* ctx) {
  if (ctx->precision_set) {   // the caller's choice stands — held to the same bound as the library's own (a mode set before the load used to go unchecked)
    if (ctx->precision < 4) return;
    F16Gate g = f16_gate(ctx, ctx->precision);
    if (!g.shapes || !g.range) { ctx->precision = 1; ctx->calib_note = "f16 modes unavailable for this model (shapes or weight range): mode 1"; return; }
    if (!g.f8) { ctx->precision = 4; ctx->calib_note = "no e4m3 weight copies for this model (K % 128): mode 4"; g = f16_gate(ctx, 4); }
    if (!g.within) {
      char buf[200];
      snprintf(buf, sizeof buf, "requested mode %d measured %.3g (> 5e-4) against mode 0 on the calibration batch%s", ctx->precision, (double)ctx->calib[ctx->precision], g.forced ? " (forced)" : ": mode 1");
      ctx->calib_note = buf;
      if (!g.forced) ctx->precision = 1;
    }
    return;
  }
  ctx->precision = 1;
  if (const F16Gate g = f16_gate(ctx, 4, false); !g.available()) {
    ctx->calib_note = g.shapes ? "a weight lies outside the f16 range: mode 1" : "no f16 kernels for these shapes: mode 1";
    return;
  }
  // the tiers, cheapest first (MFMA call-terms per encoder layer: 12, 13, 20, 21): the first one within the gate's bound of mode 0 is kept (round 6).
  // Mode 6 (e4m3 remainder) measures no faster than 4 and is not a candidate; herro_set_precision(6) calibrates it on demand.
  static const int tiers[4] = {5, 7, 8, 4};
  if (calibrate(ctx, tiers, 4) != HERRO_OK) { ctx->calib_note = "calibration run failed: mode 1"; return; }   // (one run of mode 0 for the four of them)
  for (int t : tiers) if (f16_gate(ctx, t).within) { ctx->precision = t; break; }
  char buf[400];
  snprintf(buf, sizeof buf, "calibration (256 pileup-shaped rows): max |logit(mode) - logit(mode 0, f32)| = %.3g (mode 5, f16 single terms) / %.3g (mode 7, FF single) / "
           "%.3g (mode 8, proj single) / %.3g (mode 4, f16) -> mode %d (the cheapest within 5e-4)",
           (double)ctx->calib[5], (double)ctx->calib[7], (double)ctx->calib[8], (double)ctx->calib[4], ctx->precision);
  ctx->calib_note = buf;
}

extern "C" {

int herro_load_model(herro_ctx* ctx, const char* path) {
  if (!ctx || !path) return HERRO_E_INVALID;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // 1. the host form of the file (model_pack.h).  A file that is not a model leaves the context as it was: the model it holds keeps serving.
  HostModel hm;
  std::string why;
  if (const int rc = load_host_model(path, hm, why)) { ctx->err = why; return rc; }
  // 2. the old model goes, the new one goes up.  From here to the end of the upload the context has no model.
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->has_model = false;
  ctx->M = ModelDev{};
  free_all(ctx->model_allocs);
  // the activation scratch is sized by the hyper-parameters of the model that was loaded when it was allocated (ensure_scratch: kw * c1, c2, d_model, d_ff per
  // token): it goes with that model.  Kept, a larger model loaded into the same context wrote its y1 / y2 / ff rows past the ends of the smaller model's
  // buffers as long as the token count fitted (a kw 1 model, then the default one: three times y1) — tests/test_gpu_rf_models.py, which loads one model
  // behind another, met it as an illegal memory access.  (The stream is idle here: synchronised above.)
  free_all(ctx->scratch_allocs);
  ctx->scratch_cap = 0;
  ModelDev M;
  std::vector<void*> allocs;
  if (const int rc = upload_model(ctx, hm, M, allocs)) { free_all(allocs); return rc; }
  ctx->model_allocs = std::move(allocs);
  ctx->M = M;
  ctx->wmax = hm.wmax;
  ctx->has_model = true;
  for (float& c : ctx->calib) c = -1.f;
  ctx->calib_note.clear();
  // 3. the operand format
  choose_precision(ctx);
  return HERRO_OK;
}

int64_t herro_model_describe(const herro_ctx* ctx, char* out, uint64_t cap) {
  if (!ctx || !out || !cap) return HERRO_E_INVALID;
  std::string t;
  if (!ctx->has_model) t = "no model loaded";
  else {
    const ModelHyper& h = ctx->M.h;
    const uint32_t rf = 4 * (h.kw / 2) + 1;   // rows of the window the two stacked convs see around an informative row
    const double conv = 2.0 * HERRO_ROWS * (2.0 * (h.kw / 2) + 1) * (7.0 * h.kw) * h.c1 + 2.0 * HERRO_ROWS * (double)h.kw * h.c1 * h.c2;
    const double fc = 2.0 * HERRO_ROWS * h.c2 * (double)h.d_model;
    const double layer = 2.0 * h.d_model * 3.0 * h.d_model + 2.0 * h.d_model * (double)h.d_model + 4.0 * h.d_model * (double)h.d_ff;
    const double per_tok = conv + fc + h.n_layers * layer + 2.0 * h.d_model * 6.0;
    char buf[1024];
    snprintf(buf, sizeof buf,
             "rows %u, conv kw %u (%u -> %u ch), d_model %u, heads %u, d_ff %u, layers %u; receptive field of an informative row: %u rows "
             "(a dense evaluation would run the conv stack and the projection on every one of the ~4700 rows of a window); GEMM FLOP per "
             "informative row %.3g (conv %.3g, projection %.3g, encoder %.3g), per 4096-bp window at 15 informative rows %.3g, + attention "
             "4 * n^2 * d_model per window; max |weight| %.4g; precision mode %d%s%s",
             h.rows, h.kw, h.c1, h.c2, h.d_model, h.n_heads, h.d_ff, h.n_layers, rf, per_tok, conv, fc, h.n_layers * layer, 15.0 * per_tok,
             (double)ctx->wmax, ctx->precision, ctx->calib_note.empty() ? "" : "; ", ctx->calib_note.c_str());
    t = buf;
    {  // the variant of the family and the kernels that serve it
      const ModelDev& M = ctx->M;
      static const char* act_n[3] = {"ReLU", "GELU (erf)", "GELU (tanh)"};
      static const char* pe_n[3] = {"sinusoidal position", "learned position table", "no position term"};
      char vb[400];
      snprintf(vb, sizeof vb, "; variant: %s, %s, %s%s, %s, head dim %u; kernels: %s", M.norm_first ? "Pre-LN" : "Post-LN", act_n[M.act % 3], pe_n[M.pe_kind % 3],
               M.pe_kind == 1 ? (" of " + std::to_string(M.pe_learned_rows) + " rows").c_str() : "", M.final_norm ? "final LayerNorm" : "no final LayerNorm",
               h.d_model / std::max(h.n_heads, 1u),
               model_h_supported(M) ? (model_h_conv_supported(M) ? "f16 MFMA (k_conv_m, k_fc_r, k_layers_p)" : "generic bf16x3 conv / FC in front of the f16 MFMA stack (k_layers_p)") :
               (model_default_variant(M) && h.d_model == 256 && h.n_heads == 8 && h.d_ff % 256 == 0 ? "generic conv / FC + the fused bf16x3 stack (k_layers)" : "generic bf16x3, layer by layer"));
      t += vb;
    }
  }
  const uint64_t n = std::min<uint64_t>(t.size(), cap - 1);
  std::memcpy(out, t.data(), n);
  out[n] = 0;
  return (int64_t)t.size();
}

int herro_set_precision(herro_ctx* ctx, int mode) {
  if (!ctx || mode < 0 || mode > 8) return HERRO_E_INVALID;
  if (mode >= 4 && ctx->has_model) {   // f16_gate: the mode is measured here if the load did not (mode 6 always; any mode when the load-time choice was switched off by an earlier call)
    const F16Gate g = f16_gate(ctx, mode);
    if (!g.range) {
      ctx->err = "precision 4 .. 8 (f16 operands): a weight of this model lies outside the f16 range";
      return HERRO_E_UNSUPPORTED;
    }
    if (!g.shapes) {
      ctx->err = "precision 4 .. 8 (the f16 encoder stack) need d_model 256, 8 heads of 32, d_ff % 256 == 0 and the default variant (Pre-LN, ReLU, sinusoidal position, final LayerNorm)";
      return HERRO_E_UNSUPPORTED;
    }
    if (!g.f8) {
      ctx->err = "precision 6 needs the e4m3 copies of proj / ff1 / ff2 (K % 128 == 0)";
      return HERRO_E_UNSUPPORTED;
    }
    if (g.rc != HERRO_OK) return g.rc;
    if (!g.within && !g.forced) {
      char buf[200];
      snprintf(buf, sizeof buf, "precision %d refused: the calibration of this model measured a logit difference of %.3g (> 5e-4) for the f16 kernels", mode, (double)ctx->calib[mode]);
      ctx->err = buf;
      return HERRO_E_UNSUPPORTED;
    }
  }
  ctx->precision = mode;
  ctx->precision_set = true;
  return HERRO_OK;
}

int herro_precision(const herro_ctx* ctx) { return ctx ? ctx->precision : HERRO_E_INVALID; }

float herro_calibration_error(const herro_ctx* ctx, int mode) { return (ctx && mode >= 4 && mode <= 8) ? ctx->calib[mode] : -1.f; }

int herro_debug_force_precision(herro_ctx* ctx, int on) {
  if (!ctx) return HERRO_E_INVALID;
  ctx->debug_force_precision = on != 0;
  return HERRO_OK;
}

// ---- stand-alone model entry (inference.rs:147-175) ----------------------------------------------
int herro_model_forward(herro_ctx* ctx, uint32_t B, uint32_t L, const uint8_t* bases, const uint8_t* quals,
                        const int32_t* lens, const int32_t* indices, float* info_logits, float* bases_logits) {
  if (!ctx || !bases || !quals || !lens) return HERRO_E_INVALID;
  if (!ctx->has_model) { ctx->err = "no model loaded"; return HERRO_E_NO_MODEL; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  uint64_t N = 0;
  std::vector<uint32_t> tok_off(B + 1, 0), srow;
  for (uint32_t b = 0; b < B; b++) {
    if (lens[b] < 0) return HERRO_E_INVALID;
    tok_off[b + 1] = tok_off[b] + (uint32_t)lens[b];
    N += (uint64_t)lens[b];
  }
  if (N && (!indices || !info_logits || !bases_logits)) return HERRO_E_INVALID;
  srow.resize(N);
  for (uint64_t i = 0; i < N; i++) {
    if (indices[i] < 0 || (uint32_t)indices[i] >= L) { ctx->err = "index out of range"; return HERRO_E_REFERENCE_PANIC; }
    if (ctx->M.pe_kind == 1 && (uint32_t)indices[i] >= ctx->M.pe_learned_rows) { ctx->err = "index beyond the model's learned position table"; return HERRO_E_REFERENCE_PANIC; }
    srow[i] = (uint32_t)indices[i];
  }
  if (N == 0) return HERRO_OK;
  const uint64_t cells = (uint64_t)B * L * HERRO_ROWS;
  struct Temps { std::vector<void*> v; ~Temps() { free_all(v); } } tmp;   // the temporaries of the call: freed on every return.  The late returns have waited for the stream; the early ones (out of memory, ensure_scratch) may leave copies and transposes queued and rely on hipFree's own device synchronisation
  auto A = [&](uint64_t bytes) -> void* { void* p = nullptr; if (hipMalloc(&p, std::max<uint64_t>(bytes, 16)) == hipSuccess) tmp.v.push_back(p); return p; };
  hipStream_t st = ctx->stream;
  hipError_t e = hipSuccess;
  auto up = [&](const void* src, uint64_t bytes) -> void* {
    void* p = A(bytes);
    if (p && bytes && e == hipSuccess) e = hipMemcpyAsync(p, src, bytes, hipMemcpyHostToDevice, st);
    return p;
  };
  uint8_t* d_src_b = (uint8_t*)up(bases, cells); uint8_t* d_src_q = (uint8_t*)up(quals, cells);
  uint8_t* d_pb = (uint8_t*)A(cells + 16); uint8_t* d_pq = (uint8_t*)A(cells + 16);   // + slack: k_conv_m reads up to 2 bytes behind a plane row (masked)
  uint32_t* d_sr = (uint32_t*)up(srow.data(), N * 4);
  float* d_info = (float*)A(N * 4); float* d_base = (float*)A(N * 20);
  if (!d_src_b || !d_src_q || !d_pb || !d_pq || !d_sr || !d_info || !d_base) { ctx->err = "out of device memory"; return HERRO_E_NO_DEVICE; }
  launch_transpose_blr(d_src_b, d_pb, B, L, st);
  launch_transpose_blr(d_src_q, d_pq, B, L, st);
  int rc = HERRO_OK;
  if ((rc = ensure_scratch(ctx, (uint32_t)N))) return rc;
  // one group of B windows through the builder herro_job_infer uses.  The row cap is fused_tok_cap whatever happened before: job->no_sib is the retry of a job
  // whose sibling tiles timed out, and a forward has no retry (settle_model below reports such a pass as failed).  No rf_base: the kernels read the planes at out_off.
  std::vector<PlanWin> wins(B);
  for (uint32_t b = 0; b < B; b++) wins[b] = PlanWin{(uint32_t)lens[b], L, L, L, (uint64_t)b * HERRO_ROWS * L, tok_off[b], tok_off[b], 0};
  std::vector<unsigned char> image;   // complete before its upload, alive until the stream is synchronised below
  std::vector<LaunchOffs> offs;
  build_launch(wins, launch_cfg(ctx, fused_tok_cap(ctx), false), image, offs);
  const void* d_image = up(image.data(), image.size());
  if (!d_image || e != hipSuccess) { ctx->err = e != hipSuccess ? hipGetErrorString(e) : "out of device memory"; (void)hipStreamSynchronize(st); return HERRO_E_NO_DEVICE; }
  for (const LaunchOffs& o : offs) {
    if (o.n_tiles_b && (rc = ensure_sib(ctx, o.n_tiles_b))) { (void)hipStreamSynchronize(st); return rc; }
    BatchDev bd = batch_dev(d_image, o);
    bd.planes_b = d_pb; bd.planes_q = d_pq; bd.rf_q = nullptr; bd.sup_row = d_sr; bd.out_info = d_info; bd.out_base = d_base;
    run_model(ctx, bd, o.tiled);
  }
  if ((e = hipGetLastError()) != hipSuccess) { ctx->err = hipGetErrorString(e); (void)hipStreamSynchronize(st); return HERRO_E_NO_DEVICE; }   // a launch was refused
  if ((rc = settle_model(ctx, nullptr))) return rc;
  HIP_TRY(ctx, hipMemcpy(info_logits, d_info, N * 4, hipMemcpyDeviceToHost));
  HIP_TRY(ctx, hipMemcpy(bases_logits, d_base, N * 20, hipMemcpyDeviceToHost));
  return HERRO_OK;
}

int herro_debug_set_conv_fc(herro_ctx* ctx, int mode) {
  if (!ctx || mode < -1 || mode > 1) return HERRO_E_INVALID;
  ctx->conv_fc = mode;
  return HERRO_OK;
}

// The front end's view of the device (front_end_plan, infer_plan.h): n_cu compute units from now on, 0 the device's own.  The encoder stack's tile plan
// (plan_tiles, LaunchCfg::n_cu) keeps ctx->n_cu: its tiles, and so its bits, stay where they are.
int herro_debug_set_front_cu(herro_ctx* ctx, uint32_t n_cu) {
  if (!ctx || n_cu > (1u << 20)) return HERRO_E_INVALID;
  ctx->front_cu = n_cu;
  return HERRO_OK;
}
// out[5] = fused, FC tile rows, FC grid, conv grid, conv units of the front end of the context's last model launch (FrontEndPlan)
int herro_debug_front_last(const herro_ctx* ctx, uint32_t* out) {
  if (!ctx || !out) return HERRO_E_INVALID;
  const FrontEndPlan& p = ctx->front_ran;
  out[0] = p.fused; out[1] = p.fc_rows; out[2] = p.fc_grid; out[3] = p.conv_grid; out[4] = p.conv_units;
  return HERRO_OK;
}
// front_end_plan without a device or a context, for the `count` launches of n_tok, n_tok + 1 ... tokens: out[count][5] as above
int herro_debug_front_end_plan(uint32_t n_tok, uint32_t count, uint32_t n_cu, int mode, uint32_t* out) {
  if (!out || n_tok == 0 || count == 0 || n_tok + count < n_tok || n_cu == 0 || n_cu > (1u << 20) || mode < -1 || mode > 1) return HERRO_E_INVALID;
  for (uint32_t i = 0; i < count; i++, out += 5) {
    const FrontEndPlan p = front_end_plan(n_tok + i, n_cu, mode);
    out[0] = p.fused; out[1] = p.fc_rows; out[2] = p.fc_grid; out[3] = p.conv_grid; out[4] = p.conv_units;
  }
  return HERRO_OK;
}

// Test hooks of the sibling-tile recovery: raise the context's sticky error word as a tile that timed out would (layer 0), and count the repeats.
int herro_debug_sib_fault(herro_ctx* ctx) {
  if (!ctx) return HERRO_E_INVALID;
  if (int rc = ensure_sib(ctx, 1)) return rc;
  const uint32_t one = 1;
  HIP_TRY(ctx, hipMemcpyAsync((uint32_t*)ctx->sib_flag + ctx->sib_cap, &one, 4, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return HERRO_OK;
}
int herro_debug_sib_retries(const herro_ctx* ctx) { return ctx ? (int)ctx->n_sib_retry : HERRO_E_INVALID; }

uint32_t herro_debug_e4m3(float x) { return f32_to_e4m3(x); }   // the host encoder of the precision-6 weight copies (tests)

// One tensor of a model file through the loader's own reader and packers (model_pack.h), no device and no context (tests/test_model_pack.py).
int64_t herro_debug_model_pack(const char* path, const char* tensor, uint32_t K, uint32_t N, int form, void* out, uint64_t cap, uint32_t* s8) {
  if (!path || !out || form < 0 || form > 6 || (form != 6 && !tensor) || (form == 5 && !s8)) return HERRO_E_INVALID;
  ModelFile mf;
  std::string why;
  if (const int rc = read_model_file(path, mf, why)) return rc;
  auto data = [&](const char* n, size_t expect) -> const float* {
    auto it = mf.T.find(n);
    return it == mf.T.end() || it->second.data.size() != expect ? nullptr : it->second.data.data();
  };
  std::vector<uint16_t> r16;
  std::vector<uint8_t> r8;
  if (form == 6) {
    const ModelHyper& h = mf.h;
    const float *t1 = data("t1", (size_t)h.kw * 12 * h.c1), *wq1 = data("wq1", (size_t)h.kw * h.c1), *b1 = data("b1", h.c1);
    if (h.kw != 3 || h.c1 != 64 || !t1 || !wq1 || !b1) return HERRO_E_NO_MODEL;
    r16 = pack_frag16(conv1_gemm_rows(t1, wq1, b1).data(), 96, 64);
  } else {
    const float* w = data(tensor, (size_t)K * N);
    if (!w) return HERRO_E_NO_MODEL;
    if (form <= 2 || form == 5) if (!K || !N || N % 32 || K % (form == 5 ? 128 : 32)) return HERRO_E_INVALID;
    if (form == 5) r8 = pack_frag8(w, K, N, *s8);
    else {
      Split16 s = form <= 1 ? split_bf16(w, (size_t)K * N) : split_f16(w, (size_t)K * N);
      const std::vector<uint16_t>& plane = form == 1 || form == 4 ? s.lo : s.hi;
      r16 = form <= 2 ? pack_frag16(plane.data(), K, N) : plane;
    }
  }
  const uint64_t bytes = form == 5 ? r8.size() : r16.size() * 2;
  if (bytes > cap) return HERRO_E_INVALID;
  if (bytes) std::memcpy(out, form == 5 ? (const void*)r8.data() : (const void*)r16.data(), bytes);
  return (int64_t)bytes;
}

// The token-tile plan of one fused launch over windows of cnt[i] informative rows (1..64): order[i] = index of the i-th
// window of the token stream; returns the number of tiles (packed != 0: tile_pack_order; 0: batch order).
// (packed >> 1) & 3: qmode of plan_tiles — 1 the f16 stack's default (32-token tiles for a short last round of n_cu compute
// units), 2 every small window in 32-token tiles (*n_half receives their number; the return value counts the 64-token tiles
// at the head of the stream); tile_tok (capacity n + 2, may be null) receives the first tokens of all tiles, 64-token ones first, + end.
int64_t herro_debug_tile_plan(const uint32_t* cnt, uint32_t n, int packed, uint32_t n_cu, uint32_t* order, uint32_t* n_half, uint32_t* tile_tok) {
  if (!cnt || !order) return HERRO_E_INVALID;
  std::vector<uint32_t> c(cnt, cnt + n);
  for (uint32_t v : c) if (v == 0 || v > FUSED_MAX_TOK) return HERRO_E_INVALID;
  const TilePlan P = plan_tiles(c, (packed & 1) != 0, (packed >> 1) & 3, n_cu);
  for (uint32_t i = 0; i < n; i++) order[i] = P.order[i];
  for (size_t k = 0; k + 1 < P.tiles.size(); k++) if (P.tiles[k + 1] - P.tiles[k] > FUSED_MAX_TOK) return HERRO_E_STATE;
  for (size_t k = 0; k + 1 < P.tiles_q.size(); k++) if (P.tiles_q[k + 1] - P.tiles_q[k] > FUSED_HALF_TOK) return HERRO_E_STATE;
  if (!P.tiles.empty() && !P.tiles_q.empty() && P.tiles.back() != P.tiles_q.front()) return HERRO_E_STATE;
  const size_t n64 = P.tiles.empty() ? 0 : P.tiles.size() - 1, n32 = P.tiles_q.empty() ? 0 : P.tiles_q.size() - 1;
  if (n_half) *n_half = (uint32_t)n32;
  if (tile_tok) {
    size_t k = 0;
    for (size_t i = 0; i < n64; i++) tile_tok[k++] = P.tiles[i];
    for (size_t i = 0; i < n32; i++) tile_tok[k++] = P.tiles_q[i];
    tile_tok[k] = n32 ? P.tiles_q.back() : (n64 ? P.tiles.back() : 0);
  }
  return (int64_t)n64;
}

// The same with windows above 64 rows admitted (up to 64 * 8: the f16 stack's sibling tiles, plan_tiles): n_tiles[3] = sibling tiles,
// 64-token tiles, 32-token tiles; tile_tok (capacity sum(ceil(cnt / 64)) + 2) the first tokens of all tiles in stream order
// (sibling tiles first) + end; grp (capacity = the sibling tiles) as BatchDev::tile_grp.
int herro_debug_tile_plan_sib(const uint32_t* cnt, uint32_t n, int packed, uint32_t n_cu, uint32_t* order, uint32_t* n_tiles, uint32_t* tile_tok, uint32_t* grp) {
  if (!cnt || !order || !n_tiles) return HERRO_E_INVALID;
  std::vector<uint32_t> c(cnt, cnt + n);
  for (uint32_t v : c) if (v == 0 || v > FUSED_MAX_TOK * FUSED_MAX_SIB) return HERRO_E_INVALID;
  const TilePlan P = plan_tiles(c, (packed & 1) != 0, (packed >> 1) & 3, n_cu);
  for (uint32_t i = 0; i < n; i++) order[i] = P.order[i];
  const size_t nb = P.grp.size(), n64 = P.tiles.empty() ? 0 : P.tiles.size() - 1, n32 = P.tiles_q.empty() ? 0 : P.tiles_q.size() - 1;
  if (nb && P.tiles_b.size() != nb + 1) return HERRO_E_STATE;
  n_tiles[0] = (uint32_t)nb; n_tiles[1] = (uint32_t)n64; n_tiles[2] = (uint32_t)n32;
  if (tile_tok) {
    size_t k = 0;
    uint32_t end = 0;
    for (size_t i = 0; i < nb; i++) tile_tok[k++] = P.tiles_b[i];
    if (nb) end = P.tiles_b.back();
    for (size_t i = 0; i < n64; i++) tile_tok[k++] = P.tiles[i];
    if (n64) end = P.tiles.back();
    for (size_t i = 0; i < n32; i++) tile_tok[k++] = P.tiles_q[i];
    if (n32) end = P.tiles_q.back();
    tile_tok[k] = end;
  }
  if (grp) for (size_t i = 0; i < nb; i++) grp[i] = P.grp[i];
  return HERRO_OK;
}

// The launch plan herro_job_infer would make of a job whose windows have nsup[w] informative rows and L' = Lf[w] (include/herro_amd.h): plan_batches,
// group_batches and build_launch, read back from the descriptor image itself — every window enters with its index as out_off.
int64_t herro_debug_launch_plan(const uint32_t* nsup, const uint32_t* Lf, uint32_t n_win, const uint32_t* tgt_win_off, uint32_t n_targets, uint32_t batch_size,
                                int batch_mode, int fused, uint32_t fused_rows, int packed, uint32_t n_cu, uint32_t* launch, uint32_t* pos, uint32_t* lmax) {
  if ((n_win && (!nsup || !Lf || !launch || !pos || !lmax)) || !tgt_win_off || batch_size == 0) return HERRO_E_INVALID;
  for (uint32_t t = 0; t < n_targets; t++) if (tgt_win_off[t] > tgt_win_off[t + 1] || tgt_win_off[t + 1] > n_win) return HERRO_E_INVALID;
  const std::vector<uint32_t> ns(nsup, nsup + n_win), lf(Lf, Lf + n_win);
  const std::vector<BatchPlan> batches = plan_batches(ns, lf, std::vector<uint32_t>(tgt_win_off, tgt_win_off + n_targets + 1), batch_size, batch_mode);
  const LaunchCfg cfg{fused != 0, fused_rows, (packed & 1) != 0, (packed >> 1) & 3, n_cu, false};
  std::vector<unsigned char> image;
  std::vector<LaunchOffs> offs;
  std::vector<PlanWin> wins;
  for (const LaunchGroup& g : group_batches(batches)) {
    wins.clear(); wins.reserve(g.n_win);
    for (size_t bi = g.b0; bi < g.b1; bi++)
      for (uint32_t w : batches[bi].wins) wins.push_back(PlanWin{ns[w], 0, lf[w], batches[bi].lmax, 0, 0, w, 0});
    build_launch(wins, cfg, image, offs);
  }
  for (uint32_t w = 0; w < n_win; w++) { launch[w] = 0xffffffffu; pos[w] = 0; lmax[w] = 0; }
  for (size_t l = 0; l < offs.size(); l++)
    for (uint32_t k = 0; k < offs[l].n_win; k++) {
      uint64_t w;
      std::memcpy(&w, image.data() + offs[l].out_off + 8ull * k, 8);
      std::memcpy(&lmax[w], image.data() + offs[l].lmax + 4ull * k, 4);
      launch[w] = (uint32_t)l; pos[w] = k;
    }
  return (int64_t)offs.size();
}

}  // extern "C"
