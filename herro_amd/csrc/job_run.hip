// job_run.hip — the passes of a job (include/herro_amd.h): herro_job_featurize, herro_job_infer, herro_job_consensus; job_sync (the counts of the
// featurize pass on the host), which gather of the receptive fields serves a model pass (rf_resolve), and settling a model pass before its results are
// read (settle_pass, sib_retry).  Host C++ (compiled by hipcc) over pileup.hip; the model's launches are model_api.hip, the launch plan infer_plan.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "api_job.h"
#include "job_layout.h"

using namespace herro;

// logits + compact receptive-field qualities of the job: room for `rows` informative rows (grow-only; a change waits for the stream)
static int ensure_logits(herro_job* job, uint64_t rows) {
  herro_ctx* ctx = job->ctx;
  if (job->d_info && job->logit_cap >= rows) return HERRO_OK;
  if (job->d_info) { HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); small_release(ctx, job->a_logits); job->d_info = job->d_base = nullptr; }
  job->logit_cap = std::max<uint64_t>(rows + rows / 8, 1);
  const LogitsLayout L = logits_layout(job->logit_cap);
  job->a_logits = small_acquire(ctx, L.bytes);
  if (!job->a_logits.p) { ctx->err = "out of device memory for the logits"; return HERRO_E_NO_DEVICE; }
  const LogitsView V = bind_logits(job->a_logits.p, L);
  job->d_info = V.info; job->d_base = V.base; job->d_rfq = V.rfq;
  job->gather = RfGather{};   // whatever was gathered lived in the old block
  return HERRO_OK;
}

// the counts the featurize pass left per window, on the host (waits for the pass's event, once)
int job_sync(herro_job* job) {
  herro_ctx* ctx = job->ctx;
  if (!job->featurized) { ctx->err = "herro_job_featurize has not run"; return HERRO_E_STATE; }
  if (job->synced) return HERRO_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const uint32_t n = job->J.n_win;
  { ProfSpan span_(ctx, "wait_counts"); if (n) HIP_TRY(ctx, hipEventSynchronize(job->ev_counts)); }
  job->h_Lf.assign(job->h_counts, job->h_counts + n);
  job->h_nsup.assign(job->h_counts + n, job->h_counts + 2ull * n);
  job->h_nkept.assign(job->h_counts + 2ull * n, job->h_counts + 3ull * n);
  job->h_rfbase.assign(job->h_counts + 3ull * n, job->h_counts + 4ull * n);
  job->rf_total = job->h_counts[4ull * n];
  if (ctx->timer.on) {  // per-kernel timing reads its events back: needs the whole stream
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->timer.collect();
  }
  job->sup_off.assign(n + 1, 0);
  for (uint32_t w = 0; w < n; w++) job->sup_off[w + 1] = job->sup_off[w] + job->h_nsup[w];
  job->synced = true;
  return HERRO_OK;
}

// Which gather serves this pass (model with receptive-field half width rf_half, total_sup informative rows), from what herro_job_featurize left in job->gather.
// compact: the model reads the compact records (tokens + qualities) in d_rfq, else the planes; todo: what herro_job_infer still has to gather — every window, the
// windows k_rows reserved but left to k_rfq, nothing.  Fills job->rf_base, rf_fused_used and rf_left_windows.
struct RfPlan { bool compact; enum { ALL, LEFT, NOTHING } todo; };
static RfPlan rf_resolve(herro_job* job, uint32_t rf_half, uint64_t total_sup) {
  const uint32_t n = job->J.n_win;
  const RfGather& g = job->gather;
  RfPlan r{job->d_rfq && 2 * rf_half + 1 <= 8, RfPlan::ALL};
  // the records k_rows placed are usable if they were gathered for the field of the model that is loaded NOW (herro_load_model between featurize and infer:
  // the slots k_rows handed out are not the ones k_rfq fills when infer gathers again, so rf_base must not point at them), the buffer had room and every
  // window got its slots (k_rows gathers for a half width of 2 only, which is compact)
  bool by_rows = g.who == RfGather::BY_ROWS && g.half == rf_half && job->rf_total == total_sup && total_sup <= g.cap;
  uint32_t left = 0;   // windows whose slots k_rows reserved but did not fill (above the rows it stages): k_rfq fills exactly those
  for (uint32_t w = 0; w < n && by_rows; w++) {
    if (job->h_nsup[w] == 0) continue;
    by_rows = job->h_rfbase[w] != 0xffffffffu;
    left += by_rows && (job->h_rfbase[w] & 0x80000000u) ? 1u : 0u;
  }
  const bool by_rfq = r.compact && g.who == RfGather::BY_RFQ && g.half == rf_half && g.cap >= total_sup;   // k_rfq behind featurize covers the pass
  job->rf_fused_used = by_rows;
  job->rf_left_windows = by_rows ? left : 0;
  job->rf_base.resize(n);
  for (uint32_t w = 0; w < n; w++) job->rf_base[w] = by_rows ? (uint64_t)(job->h_rfbase[w] & 0x7fffffffu) : job->sup_off[w];
  if (by_rows) r.todo = left ? RfPlan::LEFT : RfPlan::NOTHING;
  else if (by_rfq || (!r.compact && job->quals_full)) r.todo = RfPlan::NOTHING;   // (the planes path reads the complete quality planes once they exist)
  return r;
}

extern "C" {

int herro_job_featurize(herro_job* job) {
  if (!job) return HERRO_E_INVALID;
  herro_ctx* ctx = job->ctx;
  if (job->reads_gen != ctx->reads_gen) { ctx->err = "the read store was replaced (herro_set_reads) after this job was created"; return HERRO_E_STATE; }
  ProfSpan span_(ctx, "featurize");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // everything derived from a previous pass over this job is stale from here on
  job->synced = false; job->inferred = false; job->quals_full = false;
  job->lean = ctx->lean; job->tokens_full = !ctx->lean;
  job->consensus_done = false; job->consensus_on_host = false; job->logits_on_host = false;
  if (job->J.n_win == 0) { job->featurized = true; return HERRO_OK; }
  // (the receptive fields are gathered ahead of herro_job_infer exactly when a model is loaded: a context that only writes features — `herro features` — loads
  // none and pays for no gather; the call-history heuristic of round 5 made jobs 5.. of a featurize-all-then-infer caller lose the early gather: ADVICE r5)
  const uint32_t rf_half = ctx->has_model ? 2 * (ctx->M.h.kw / 2) : 0;
  // The model's receptive fields are gathered by k_rows itself on the lean path (records placed by one atomic per window), into a buffer sized by the
  // job's previous pass or by an estimate; if it turns out too small — or a window has more informative rows than k_rows stages — herro_job_infer
  // gathers with k_rfq instead.  HERRO_RF_FUSED=0: always k_rfq (A/B).
  // WHEN: if the caller pipelines its jobs (another job of this context is featurized and waits for its herro_job_infer), the GPU has that job's kernels
  // to run while the host plans this one, and the fused gather is the faster one (k_rows + k_rfq 276 -> 230 us per 4096 windows, +3.8 % at the bench's
  // default size).  A job on its own (the driver's 20-step run) is better served by k_rfq launched BEHIND the copy of the counts: the host wakes up and
  // plans the batches while it runs, instead of the GPU idling for the plan (same-box A/B, profiles/r5_ab_runs.json r5i: 2.04 vs 1.96 M windows/s).
  // HERRO_RF_FUSED=1 / 0 forces one or the other (A/B).
  static const int fuse_rf = ab_env("HERRO_RF_FUSED", -1) < 0 ? -1 : (ab_env("HERRO_RF_FUSED", -1) != 0 ? 1 : 0);
  const bool pipelined = ctx->n_pending.load() - (job->pending ? 1 : 0) > 0;
  if (!job->pending) { job->pending = true; ctx->n_pending++; }
  job->gather = RfGather{};   // nothing is gathered for this pass yet
  job->J.rf = nullptr;
  if (job->lean && (fuse_rf == 1 || (fuse_rf < 0 && pipelined)) && ctx->has_model && rf_half == 2) {
    const uint64_t want = job->logit_cap > 1 ? job->logit_cap : (uint64_t)job->J.n_win * 24;   // ~15 informative rows per window at the bench workload
    if (ensure_logits(job, want) == HERRO_OK) {
      job->J.rf = job->d_rfq; job->J.rf_cap = std::min<uint64_t>(job->logit_cap, 0xfffffff0ull / HERRO_ROWS); job->J.rf_half = rf_half;
      job->gather = RfGather{RfGather::BY_ROWS, rf_half, job->J.rf_cap};
      HIP_TRY(ctx, hipMemsetAsync(job->J.rf_alloc, 0, 4, ctx->stream));
    }
  }
  launch_featurize(job->J, ctx->stream, &ctx->timer, job->lean);
  HIP_TRY(ctx, hipGetLastError());
  // the per-window counts follow the kernels into pinned memory; whoever needs them waits for the event,
  // not for the stream, so the next job's kernels can already be queued behind this one
  HIP_TRY(ctx, hipMemcpyAsync(job->h_counts, job->d_counts, (uint64_t)job->J.n_win * 16 + 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipEventRecord(job->ev_counts, ctx->stream));
  job->featurized = true;
  // The model's receptive-field qualities, gathered NOW (k_rfq needs the informative rows and their job-level slots — a device
  // prefix — not the batch plan): by the time the host has the counts and has planned the batches, the GPU is through this
  // kernel instead of having waited for the plan.  The buffer is sized by the job's previous pass or by an estimate; if the
  // count turns out larger, herro_job_infer gathers again.  HERRO_RFQ_EARLY=0: gather in herro_job_infer (A/B).
  static const bool early = ab_env("HERRO_RFQ_EARLY", 1) != 0;
  if (early && job->gather.who == RfGather::NONE && ctx->has_model && 2 * rf_half + 1 <= 8) {
    const uint32_t n = job->J.n_win;
    if (!job->a_supoff_dev.p) job->a_supoff_dev = small_acquire(ctx, ((uint64_t)n + 1) * 8);
    const uint64_t want = job->logit_cap > 1 ? job->logit_cap : (uint64_t)n * 24;   // ~15 informative rows per window at the bench workload
    if (job->a_supoff_dev.p && ensure_logits(job, want) == HERRO_OK) {
      launch_supoff(job->J, (uint64_t*)job->a_supoff_dev.p, ctx->stream);
      launch_rf_quals(job->J, rf_half, (const uint64_t*)job->a_supoff_dev.p, job->d_rfq, job->logit_cap, job->lean, ctx->stream, &ctx->timer);
      HIP_TRY(ctx, hipGetLastError());
      job->gather = RfGather{RfGather::BY_RFQ, rf_half, job->logit_cap};
    }
  }
  return HERRO_OK;
}

int herro_job_infer(herro_job* job, uint32_t batch_size, int batch_mode) {
  if (!job || batch_size == 0) return HERRO_E_INVALID;
  herro_ctx* ctx = job->ctx;
  if (!ctx->has_model) { ctx->err = "no model loaded"; return HERRO_E_NO_MODEL; }
  ProfSpan span_(ctx, "infer");
  job->last_batch_size = batch_size; job->last_batch_mode = batch_mode;
  if (job->pending) { job->pending = false; ctx->n_pending--; }
  int rc = job_sync(job);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const uint32_t n = job->J.n_win;
  const uint64_t total_sup = job->sup_off[n];
  if (total_sup > 0xffffffffull / HERRO_ROWS) { ctx->err = "job too large (informative rows x 31 exceed 2^32: TokMeta::rf_idx is a 32-bit job-level index)"; return HERRO_E_UNSUPPORTED; }
  if ((rc = ensure_logits(job, total_sup))) return rc;
  if (ctx->M.pe_kind == 1)   // a learned position table is indexed by the row: a window longer than the table would raise an index error in the archive
    for (uint32_t w = 0; w < n; w++)
      if (job->h_nsup[w] && job->h_Lf[w] > ctx->M.pe_learned_rows) {
        ctx->err = "a window of " + std::to_string(job->h_Lf[w]) + " rows exceeds the model's learned position table (" + std::to_string(ctx->M.pe_learned_rows) + " rows): the archive would raise an index error";
        return HERRO_E_REFERENCE_PANIC;
      }
  const uint32_t rf_half = 2 * (ctx->M.h.kw / 2);   // the qualities the model will read: rows within 2 * (kw / 2) of an informative row (two stacked convs)
  const RfPlan rf = rf_resolve(job, rf_half, total_sup);
  // ---- the plan (infer_plan.h): batches, launch groups, per group the descriptor arrays of its launches
  const std::vector<BatchPlan> batches = plan_batches(job->h_nsup, job->h_Lf, job->tgt_win_off, batch_size, batch_mode);
  const std::vector<LaunchGroup> groups = group_batches(batches);
  if (job->a_bdesc.p) HIP_TRY(ctx, hipEventSynchronize(job->ev_blob));  // a previous upload of the blob is over
  std::vector<unsigned char>& blob = job->blob;
  blob.clear();
  const LaunchCfg cfg = launch_cfg(ctx, job->no_sib ? FUSED_MAX_TOK : fused_tok_cap(ctx), true);
  std::vector<LaunchOffs> offs;
  std::vector<PlanWin> wins;
  for (const LaunchGroup& g : groups) {
    wins.clear(); wins.reserve(g.n_win);   // (exactly: a vector grown by doubling would cross the allocator's mmap threshold at the bench's job size, on every pass)
    for (size_t bi = g.b0; bi < g.b1; bi++)
      for (uint32_t w : batches[bi].wins) {
        const WinDesc& wd = job->win[w];
        wins.push_back(PlanWin{job->h_nsup[w], wd.lub, job->h_Lf[w], batches[bi].lmax, wd.fin_off, wd.row_off, job->sup_off[w], job->rf_base[w]});
      }
    build_launch(wins, cfg, blob, offs);
  }
  uint32_t max_tok = 0, max_tiles_b = 0;
  for (const LaunchOffs& o : offs) { max_tok = std::max(max_tok, o.n_tok); max_tiles_b = std::max(max_tiles_b, o.n_tiles_b); }
  const size_t supoff_at = image_put(blob, job->sup_off);  // consensus reads it from the same blob
  if (job->a_bdesc.cap < blob.size()) {
    if (job->a_bdesc.p) { HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); small_release(ctx, job->a_bdesc); }
    job->a_bdesc = small_acquire(ctx, blob.size() + blob.size() / 4 + 4096);
    if (!job->a_bdesc.p) { ctx->err = "out of device memory for the batch descriptors"; return HERRO_E_NO_DEVICE; }
  }
  HIP_TRY(ctx, hipMemcpyAsync(job->a_bdesc.p, blob.data(), blob.size(), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipEventRecord(job->ev_blob, ctx->stream));
  job->d_supoff_blob = (const uint64_t*)((const unsigned char*)job->a_bdesc.p + supoff_at);
  if ((rc = ensure_scratch(ctx, max_tok))) return rc;
  if (max_tiles_b && (rc = ensure_sib(ctx, max_tiles_b))) return rc;
  // ---- the gather, unless featurize did it
  if (!groups.empty()) {
    if (!rf.compact && !job->tokens_full) {   // a receptive field above 8 rows: token planes + row map first
      launch_full_tokens(job->J, ctx->stream, &ctx->timer);
      job->tokens_full = true;
    }
    uint8_t* const rfq = rf.compact ? job->d_rfq : nullptr;
    if (rf.todo == RfPlan::ALL) launch_rf_quals(job->J, rf_half, job->d_supoff_blob, rfq, job->logit_cap, job->lean, ctx->stream, &ctx->timer);
    else if (rf.todo == RfPlan::LEFT) launch_rf_quals(job->J, rf_half, job->d_supoff_blob, rfq, job->logit_cap, job->lean, ctx->stream, &ctx->timer, /*left_only=*/true);
    // RfPlan::NOTHING: the records (or the complete quality planes) are there
  }
  for (const LaunchOffs& o : offs) {
    BatchDev B = batch_dev(job->a_bdesc.p, o);
    B.planes_b = job->J.fin_b; B.planes_q = job->J.fin_q; B.sup_row = job->J.sup_row;
    B.rf_q = rf.compact ? job->d_rfq : nullptr;
    B.out_info = job->d_info; B.out_base = job->d_base;
    if (o.tiled && o.n_tiles_b && std::find(ctx->sib_suspects.begin(), ctx->sib_suspects.end(), job) == ctx->sib_suspects.end()) ctx->sib_suspects.push_back(job);
    run_model(ctx, B, o.tiled);
  }
  HIP_TRY(ctx, hipGetLastError());
  job->sib_stale = false;   // (a new pass supersedes whatever the previous one was suspected of; this pass is a suspect again if it launched sibling tiles)
  job->inferred = true;
  job->logits_on_host = false;
  job->consensus_done = false;
  return HERRO_OK;
}

int herro_job_consensus(herro_job* job) {
  if (!job) return HERRO_E_INVALID;
  herro_ctx* ctx = job->ctx;
  ProfSpan span_(ctx, "consensus");
  int rc = job_sync(job);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const uint32_t n = job->J.n_win;
  if (job->sup_off.back() > 0 && !job->inferred) { ctx->err = "herro_job_infer has not run"; return HERRO_E_STATE; }
  const uint64_t* d_so = job->d_supoff_blob;
  if (!job->inferred || !d_so) {  // nothing informative anywhere: infer never ran for this job
    if (!job->d_supoff) {
      job->a_supoff = small_acquire(ctx, std::max<uint64_t>(n, 1) * 8);
      if (!job->a_supoff.p) { ctx->err = "out of device memory"; return HERRO_E_NO_DEVICE; }
      job->d_supoff = (uint64_t*)job->a_supoff.p;
    }
    if (!job->d_base) {  // a dummy logits buffer
      job->a_logits = small_acquire(ctx, 512);
      if (!job->a_logits.p) { ctx->err = "out of device memory"; return HERRO_E_NO_DEVICE; }
      job->d_info = (float*)job->a_logits.p;
      job->d_base = (float*)((unsigned char*)job->a_logits.p + 256);
      job->logit_cap = 1;
    }
    if (n) HIP_TRY(ctx, hipMemcpyAsync(job->d_supoff, job->sup_off.data(), n * 8ull, hipMemcpyHostToDevice, ctx->stream));
    d_so = job->d_supoff;
  }
  launch_consensus(job->J, d_so, job->d_base, job->lean, ctx->stream, &ctx->timer);
  HIP_TRY(ctx, hipGetLastError());
  job->consensus_done = true;
  job->consensus_on_host = false;
  return HERRO_OK;
}

}  // extern "C"

// A sibling tile that never saw its group (check_sib, model_api.hip) is not the caller's problem: the model pass of every job the raised word may belong to — and its
// consensus pass, if that had run — is repeated ONCE with its windows above 64 informative rows on the layer-by-layer kernels, which have no cross-workgroup wait,
// each when it is fetched (the job that fetches first is not the only one).  Returns check_sib's code when the repeat cannot run or fails too.
static int sib_retry(herro_job* job, int rc_sib) {
  herro_ctx* ctx = job->ctx;
  if (job->no_sib || !job->last_batch_size) return rc_sib;
  const bool had_consensus = job->consensus_done;
  const std::string why = ctx->err.c_str();
  job->no_sib = true;
  job->sib_stale = false;
  ctx->n_sib_retry++;
  int rc = herro_job_infer(job, job->last_batch_size, job->last_batch_mode);
  if (!rc && had_consensus) rc = herro_job_consensus(job);
  if (rc) { const std::string second = ctx->err.c_str(); ctx->err = why + "; the repeat without sibling tiles failed: " + second; return rc; }
  return settle_model(ctx, job);
}

// Settling a job's model pass before its results are read (the logits, the corrected bases, the text formed from them): settle_model (model_api.hip: the stream
// idle, the timer's events in, the sibling tiles' error word), and on a raised word the repeat of the pass, once.  HERRO_OK: what the device holds of the job is
// to be trusted; *repeated (may be null): it is the second pass's, so whatever the caller queued in front of the wait read the first one's.
int settle_pass(herro_job* job, bool* repeated) {
  if (repeated) *repeated = false;
  int rc = settle_model(job->ctx, job);
  if (!rc || (rc = sib_retry(job, rc))) return rc;
  if (repeated) *repeated = true;
  return HERRO_OK;
}

extern "C" {

int herro_debug_set_featurize_planes(herro_ctx* ctx, int on) {
  if (!ctx) return HERRO_E_INVALID;
  ctx->lean = on == 0;
  return HERRO_OK;
}

// 1: the last herro_job_infer read the receptive fields k_rows gathered behind featurize; 0: k_rfq gathered them (a window above 256 informative
// rows, a buffer sized too small by the estimate of a first pass, the planes path, HERRO_RF_FUSED=0)
int herro_debug_job_rf_fused(const herro_job* job) { return job && job->inferred ? (job->rf_fused_used ? 1 : 0) : HERRO_E_STATE; }
int herro_debug_job_rf_left(const herro_job* job) { return job && job->inferred ? (int)job->rf_left_windows : HERRO_E_STATE; }

// the receptive-field records the model read for window w (valid once herro_job_infer has run with a compact receptive field)
int64_t herro_debug_job_rf(herro_job* job, uint32_t w, uint8_t* out, uint64_t cap) {
  if (!job || w >= job->win.size() || !out) return HERRO_E_INVALID;
  herro_ctx* ctx = job->ctx;
  if (!job->inferred || !job->d_rfq) { ctx->err = "herro_job_infer has not run"; return HERRO_E_STATE; }
  const uint64_t n = (uint64_t)job->h_nsup[w] * HERRO_ROWS;
  if (n * 16 > cap) { ctx->err = "output buffer too small"; return HERRO_E_INVALID; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (n) HIP_TRY(ctx, hipMemcpy(out, job->d_rfq + job->rf_base[w] * HERRO_ROWS * 16, n * 16, hipMemcpyDeviceToHost));
  return (int64_t)n;
}

}  // extern "C"
