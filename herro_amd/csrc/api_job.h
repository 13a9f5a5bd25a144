// api_job.h — what the translation units of the C ABI share of a JOB (api_ctx.h: of a context): herro_job itself, and the helpers that cross units —
// job_create.hip builds a job, job_run.hip runs its passes (featurize, infer, consensus), job_out.hip fetches and writes what they left, model_api.hip
// owns the model and its launches, herro_api.hip the context's memory.  Internal: nothing here is exported.  Host only: no kernel reads this header.
#pragma once
#include <chrono>
#include <cmath>
#include <cstdio>

#include "api_ctx.h"
#include "infer_plan.h"

// HERRO_HOST_PROFILE=2: one stderr line per API call with its start time and duration (host-side timeline of a pipeline).
struct ProfSpan {
  static int level() { static const int l = [] { const char* e = getenv("HERRO_HOST_PROFILE"); return e ? atoi(e) : 0; }(); return l; }
  static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
  const void* who; const char* name; double t0;
  ProfSpan(const void* w, const char* n) : who(w), name(n), t0(level() >= 2 ? now_ms() : 0) {}
  ~ProfSpan() { if (level() >= 2) { const double t1 = now_ms(); fprintf(stderr, "TL %p %-14s %.3f %.3f\n", who, name, fmod(t0, 1e6), t1 - t0); } }
};

// array inside the job's pinned host arena
template <class T>
struct harr {
  T* p = nullptr;
  size_t n = 0;
  T& operator[](size_t i) { return p[i]; }
  const T& operator[](size_t i) const { return p[i]; }
  size_t size() const { return n; }
  T* data() { return p; }
  const T* data() const { return p; }
};

// What herro_job_featurize gathered of the model's receptive fields ahead of herro_job_infer: at most one of k_rows itself on the lean path (records placed by one
// atomic per window, JobDev::win_rfbase) and k_rfq right behind the featurize kernels (records at the device prefix of the informative rows), for a receptive field
// of half width `half`, into room for `cap` informative rows.  rf_resolve decides in herro_job_infer whether the records serve the pass.
struct RfGather { enum Who : uint8_t { NONE, BY_ROWS, BY_RFQ } who = NONE; uint32_t half = 0; uint64_t cap = 0; };

struct herro_job {
  herro_job() = default;
  herro_job(const herro_job&) = delete;
  ~herro_job();   // job_create.hip: returns the arenas, the small buffers and the events
  herro_ctx* ctx = nullptr;
  // ---- build (herro_job_create*): descriptors, arenas, what was left out
  uint32_t W = 0, n_targets = 0;
  harr<herro::WinDesc> win;
  harr<herro::OwDesc> ow;
  harr<uint32_t> ops;
  std::vector<uint32_t> tgt_win_off;  // [n_targets+1]
  harr<uint32_t> tile_win, tile_r0;
  herro::JobDev J{};
  Arena dev{}, pin{};              // device arena (descriptors + every scratch / result array), pinned host arena
  Arena scan{};                    // device: the op array written by the CIGAR scan (+ the staged text it was read from)
  uint64_t scan_ops = 0;           // slots in it
  std::vector<uint32_t> dbg_ops;   // herro_debug_job_array(ops) of such a job: fetched on demand
  bool dev_built = false;          // windows and descriptors were built on the device (build_dev.hip): the overlap descriptors and the tile list exist there only
  std::vector<herro::OwDesc> dbg_ow;      // ... and come down for herro_debug_job_array
  bool from_ops_text = false;      // herro_job_create_aligned built it from the TEXT of its ops (its direct path was not taken or did not settle the job)
  std::vector<uint32_t> dbg_tw, dbg_tr;
  uint64_t reads_gen = 0;
  uint32_t n_skipped_alns = 0, n_failed_targets = 0;  // inputs the library does not support, left out (herro_job_skipped)
  std::string first_skip;
  uint64_t row_elems = 0;
  uint64_t alg_read_bytes = 0, alg_op_bytes = 0;
  // ---- featurize results (herro_job_featurize, job_sync)
  bool featurized = false, synced = false, inferred = false;
  bool pending = false;      // counted in herro_ctx::n_pending
  bool lean = false;         // the last featurize pass ran the lean path (k_rows): votes in position space, no row map
  bool tokens_full = false;  // the token planes + row map exist (planes path, or launch_full_tokens behind a lean pass)
  bool quals_full = false;   // the complete quality planes exist (featurize never writes them)
  uint32_t* d_counts = nullptr;      // [4][n_win] + 1: L', informative rows, kept overlaps, k_rows' first record (win_rfbase), then the records it handed out in all (one D2H per job)
  uint32_t* h_counts = nullptr;      // pinned
  hipEvent_t ev_counts = nullptr;    // featurize + the copy of the counts finished
  std::vector<uint32_t> h_Lf, h_nsup, h_nkept;   // host copies after sync
  std::vector<uint64_t> sup_off;     // [n_win+1] prefix of nsup
  // ---- gather of the receptive fields
  RfGather gather;                   // what featurize gathered early
  std::vector<uint32_t> h_rfbase;    // per window: first record k_rows reserved (bit 31: left to k_rfq, above the rows k_rows stages; 0xffffffff: none, the buffer was full)
  uint32_t rf_total = 0;             // records k_rows handed out, in informative rows
  Arena a_supoff_dev{};              // u64[n_win + 1] written by k_supoff for the early k_rfq
  bool rf_fused_used = false;        // herro_job_infer read the records k_rows gathered (herro_debug_job_rf_fused)
  uint32_t rf_left_windows = 0;      // ... of which this many windows were filled by k_rfq behind it (herro_debug_job_rf_left)
  std::vector<uint64_t> rf_base;     // per window: first record of its receptive fields in d_rfq (whichever kernel wrote them), valid after herro_job_infer
  // ---- inference (herro_job_infer, the fetch of the logits)
  uint64_t logit_cap = 0;    // informative rows a_logits has room for
  Arena a_logits{};
  float *d_info = nullptr, *d_base = nullptr;   // inside a_logits
  uint8_t* d_rfq = nullptr;  // inside a_logits: the receptive fields, compact (BatchDev::rf_q)
  std::vector<float> h_info, h_base;
  bool logits_on_host = false;
  Arena a_bdesc{};                   // device: the descriptor image of the pass (infer_plan.h: build_launch) + sup_off
  std::vector<unsigned char> blob;   // its host image (kept alive: its upload is asynchronous)
  hipEvent_t ev_blob = nullptr;      // upload of blob finished
  bool sib_stale = false;       // the context's sibling-tile error word was found raised while this job's pass was unchecked: its logits are not to be trusted (sib_retry repeats the pass)
  bool no_sib = false;          // a sibling tile of this job timed out once: its windows above 64 rows go layer by layer from now on (sib_retry)
  uint32_t last_batch_size = 0; int last_batch_mode = 0;   // arguments of the last herro_job_infer (sib_retry repeats it)
  // ---- consensus
  Arena a_supoff{};
  uint64_t* d_supoff = nullptr;
  const uint64_t* d_supoff_blob = nullptr;  // sup_off inside a_bdesc (valid once infer has run)
  bool consensus_done = false, consensus_on_host = false;
  uint32_t* h_cons_len = nullptr;   // pinned (inside the host arena): landing zone of the corrected bases
  uint8_t* h_cons_seq = nullptr;
};

static constexpr uint32_t FUSED_MAX_SIB = 8;     // sibling tiles of one window in the f16 stack (k_layers_p<., 4, true>): windows of up to 512 informative rows stay fused (the plan in infer_plan.h never reads it; tests/capacity_cases.py reads it here; fused_tok_cap, model_api.hip)

// ---- which windows of a target yield corrected text (consensus.rs:90-101), valid once job_sync has run
// n_alns of window w: its kept overlaps, as far as the pileup has rows for them
inline uint32_t window_alns(const herro_job* job, uint32_t w) { const uint32_t kept = job->h_nkept[w]; return kept < HERRO_MAX_ALNS ? kept : HERRO_MAX_ALNS; }
// a window with fewer than two alignments is not corrected: the read is split there
inline bool window_corrected(const herro_job* job, uint32_t w) { return window_alns(job, w) >= 2; }
// [*st, *en): the first to the last corrected window of target t; false: it has none
inline bool corrected_span(const herro_job* job, uint32_t t, uint32_t* st, uint32_t* en) {
  bool any = false;
  for (uint32_t w = job->tgt_win_off[t]; w < job->tgt_win_off[t + 1]; w++)
    if (window_corrected(job, w)) { if (!any) *st = w; *en = w + 1; any = true; }
  return any;
}

// ---- helpers that cross units
// herro_api.hip: the context's recycled memory, and the host ranges registered for zero-copy job creation
Arena small_acquire(herro_ctx* ctx, size_t need);
void small_release(herro_ctx* ctx, Arena& a);
Arena arena_acquire(herro_ctx* ctx, std::vector<Arena>& list, size_t need, int kind);
void arena_release(herro_ctx* ctx, std::vector<Arena>& list, Arena& a, int kind);
bool host_range_registered(const unsigned char* lo, const unsigned char* hi, const unsigned char** dev = nullptr);
extern std::atomic<uint64_t> g_zero_copy_jobs;
// model_api.hip: the model's buffers, and one launch of the model
int ensure_scratch(herro_ctx* ctx, uint32_t n_tok);
int ensure_sib(herro_ctx* ctx, uint32_t n_tiles_b);
uint32_t fused_tok_cap(const herro_ctx* ctx);
LaunchCfg launch_cfg(const herro_ctx* ctx, uint32_t fused_rows, bool with_rf_base);
herro::BatchDev batch_dev(const void* d_image, const LaunchOffs& o);
void run_model(herro_ctx* ctx, const herro::BatchDev& B, bool tiled);
int settle_model(herro_ctx* ctx, herro_job* job);
// job_run.hip
int job_sync(herro_job* job);
int settle_pass(herro_job* job, bool* repeated = nullptr);
