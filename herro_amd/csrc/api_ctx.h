// api_ctx.h — what the translation units of the C ABI share (herro_api.hip: contexts; model_api.hip: the model; job_create.hip, job_run.hip, job_out.hip: jobs,
// which share api_job.h on top; frontend_api.hip: reads alone -> records -> ops on the device): the context, its last-error slot, HIP_TRY and the host pool.
// Internal: nothing here is exported.
// (The host half of herro_load_model — file reader, number formats, weight layouts — is model_pack.h, which knows neither a context nor HIP.)
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdlib>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/herro_amd.h"
#include "job_dev.h"
#include "model_dev.h"

// Last-error text of a context.  Job creation may run on a second thread (herro_amd.h, "Threading"), so assignment is
// serialised; the text read back is the most recent failure of either thread, kept in a buffer that only assignment replaces.
struct ErrSlot {
  std::mutex mu;
  std::string s;
  ErrSlot& operator=(const std::string& v) { std::lock_guard<std::mutex> lk(mu); s = v; return *this; }
  ErrSlot& operator=(const char* v) { std::lock_guard<std::mutex> lk(mu); s = v; return *this; }
  // the text handed out is a per-thread copy: an assignment by another thread (job creation may run beside the execution
  // calls) cannot pull the buffer away under the reader
  const char* c_str() const {
    thread_local std::string snap;
    { std::lock_guard<std::mutex> lk(const_cast<std::mutex&>(mu)); snap = s; }
    return snap.c_str();
  }
};

#define HIP_TRY(ctx, expr)                                                              \
  do {                                                                                  \
    hipError_t _e = (expr);                                                             \
    if (_e != hipSuccess) {                                                             \
      (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(_e);                   \
      return HERRO_E_NO_DEVICE;                                                         \
    }                                                                                   \
  } while (0)

// ---- host thread pool, one per context (created on first use).  herro_job_create used to start and join
// min(cores, 64) std::threads twice per call; on a 256-core box that alone was ~3 of its 15 ms per 4096 windows.
struct HostPool {
  std::vector<std::thread> th;
  std::mutex m;
  std::condition_variable cv, done_cv;
  const std::function<void(uint32_t)>* fn = nullptr;
  std::atomic<uint32_t> next{0};
  uint32_t n = 0, active = 0;
  uint64_t gen = 0;
  bool stop = false;
  explicit HostPool(uint32_t workers) {
    for (uint32_t i = 0; i < workers; i++) th.emplace_back([this] { loop(); });
  }
  ~HostPool() {
    { std::lock_guard<std::mutex> lk(m); stop = true; }
    cv.notify_all();
    for (auto& t : th) t.join();
  }
  void work() {
    for (;;) {
      const uint32_t i = next.fetch_add(1, std::memory_order_relaxed);
      if (i >= n) break;
      (*fn)(i);
    }
  }
  void loop() {
    uint64_t seen = 0;
    for (;;) {
      {
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [&] { return stop || gen != seen; });
        if (stop) return;
        seen = gen;
      }
      work();
      std::lock_guard<std::mutex> lk(m);
      if (--active == 0) done_cv.notify_one();
    }
  }
  // fn(i) for i in [0, count), on the workers and the calling thread; returns when all are done.  One run at a time: a second
  // caller (herro_set_reads beside a herro_job_create of another thread on the same context) waits its turn.
  std::mutex run_mu;
  void run(uint32_t count, const std::function<void(uint32_t)>& f) {
    if (count == 0) return;
    if (th.empty() || count == 1) { for (uint32_t i = 0; i < count; i++) f(i); return; }
    std::lock_guard<std::mutex> one_run(run_mu);
    {
      std::lock_guard<std::mutex> lk(m);
      fn = &f; n = count; next.store(0); active = (uint32_t)th.size(); gen++;
    }
    cv.notify_all();
    work();
    std::unique_lock<std::mutex> lk(m);
    done_cv.wait(lk, [&] { return active == 0; });
  }
};

// Device scratch of one call: MiB from the environment (at least 1), else default_mb
inline uint64_t scratch_budget(const char* env_name, uint64_t default_mb = 4096) { const char* e = getenv(env_name); return e ? (uint64_t)std::max(1ll, atoll(e)) << 20 : default_mb << 20; }

// a list of device allocations (the model's, the activation scratch's, the temporaries of a call) goes
inline void free_all(std::vector<void*>& v) {
  for (void* p : v) if (p) (void)hipFree(p);
  v.clear();
}

struct Arena { void* p = nullptr; size_t cap = 0; };

// The smallest block of a free list that holds `need` bytes, taken out of the list (null: none does).  The caller holds the list's lock; what a list's
// fresh blocks are made of, and with how much slack, is the caller's.
inline Arena best_fit_take(std::vector<Arena>& list, size_t need) {
  size_t best = list.size();
  for (size_t i = 0; i < list.size(); i++)
    if (list[i].cap >= need && (best == list.size() || list[i].cap < list[best].cap)) best = i;
  if (best == list.size()) return Arena{};
  const Arena a = list[best];
  list.erase(list.begin() + best);
  return a;
}

// Pinned host blocks that results handed to the caller live in (herro_fasta_text): recycled like the job arenas — hipHostMalloc of a text's size
// costs more than forming the text —, and shared between the context and its handles, so that a handle freed after its context still has
// somewhere to give its block back to; the blocks go with the last holder.
struct PinPool {
  std::mutex mu;
  std::vector<Arena> free;
  ~PinPool() { for (Arena& a : free) (void)hipHostFree(a.p); }
  Arena acquire(size_t need) {
    Arena a;
    { std::lock_guard<std::mutex> lk(mu); a = best_fit_take(free, need); }
    if (a.p) return a;
    a.cap = need + need / 8 + 4096;
    if (hipHostMalloc(&a.p, a.cap, hipHostMallocDefault) != hipSuccess) { a.p = nullptr; a.cap = 0; }
    return a;
  }
  void release(Arena& a) {
    if (!a.p) return;
    std::lock_guard<std::mutex> lk(mu);
    if (free.size() < 4) free.push_back(a); else (void)hipHostFree(a.p);
    a = Arena{};
  }
};

struct herro_ctx {
  int device = 0;
  uint32_t n_cu = 256;   // compute units of the device: one round of the fused stack (plan_tiles)
  hipStream_t own_stream = nullptr, stream = nullptr;
  ErrSlot err;
  // read store
  uint32_t n_reads = 0;
  std::vector<uint32_t> read_len, name_class;
  std::vector<uint64_t> h_word_off, h_qual_off;  // host copies: overlap descriptors carry them (saves the kernel a dependent load)
  bool host_only = false;  // herro_debug_host_ctx: no device; herro_job_create stops after the host half
  // lean: herro_job_featurize derives informative rows, votes and receptive fields without writing the token planes (k_rows); the planes are
  // built when somebody asks for them.  HERRO_FEATURIZE_PLANES=1 (or herro_debug_set_featurize_planes): the planes path of rounds 3-4 (A/B, parity tests)
  bool lean = [] { const char* e = getenv("HERRO_FEATURIZE_PLANES"); return !e || atoi(e) == 0; }();
  int conv_fc = -1;   // front end of the f16 model (launch_model_h): -1 chosen per launch (conv_fc_faster), 0 k_conv_m + k_fc_r, 1 k_conv_fc wherever its shapes allow (herro_debug_set_conv_fc)
  uint32_t front_cu = 0;   // herro_debug_set_front_cu: the compute units the FRONT END plans for (front_end_plan), 0 = n_cu; plan_tiles and LaunchCfg never see it
  FrontEndPlan front_ran{false, 0, 0, 0, 0};   // what the front end of the last model launch sent out (herro_debug_front_last)
  bool tile_packing = herro::ab_env("HERRO_TILE_PACK", 1) != 0;  // 0 (A/B builds): windows in batch order
  uint64_t* d_words = nullptr;
  uint32_t* d_p0 = nullptr;
  uint32_t* d_p1 = nullptr;
  uint64_t* d_word_off = nullptr;
  uint8_t* d_qual = nullptr;
  uint64_t* d_qual_off = nullptr;
  double* d_ln = nullptr;
  uint32_t ln_n = 0;
  uint64_t read_bytes = 0, qual_bytes = 0, n_words = 0;
  // the device arrays of the read store belong to this owner: the contexts of one device can share ONE store (herro_share_reads);
  // its memory is freed when the last context holding it lets go
  std::shared_ptr<void> store_owner;
  herro_seed_rescue_params seed_rescue{};   // herro_set_seed_rescue: occ_dist 0 = off; rescue_max_occ as given (0 = 4095 where it is used)
  uint32_t chain_lookback = 64;             // herro_set_chain_params: the predecessors a chain step looks at, a multiple of 64 in 64 .. 1024
  herro_index_params index_parts{};         // herro_set_index_params: max_kmers 0 = off, the index of a finder call is built in one piece
  uint64_t debug_adapter_cap = 0;          // herro_debug_set_adapter_cap: hits the first scan's buffer of herro_find_adapters holds (0: the default)
  std::shared_ptr<PinPool> text_pin = std::make_shared<PinPool>();   // herro_job_fasta_dev: where its texts land
  uint64_t debug_fasta_chunk = 0;           // herro_debug_set_fasta_chunk: text bytes of a chunk of herro_job_fasta_dev (0: a sixteenth of HERRO_FASTA_SCRATCH_MB)
  // model
  bool has_model = false;
  herro::ModelDev M{};
  std::vector<void*> model_allocs;
  int precision = 1;
  bool precision_set = false;   // herro_set_precision was called: herro_load_model keeps the caller's choice
  bool debug_force_precision = false;   // herro_debug_force_precision: herro_set_precision skips the calibration gate (tests measure the modes a model's calibration refuses)
  float wmax = 0.f;             // largest |weight| of the loaded model
  float calib[9] = {-1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f};   // [mode]: max |logit difference| of f16 mode 4 .. 8 vs mode 0 (f32 MFMA) on the calibration batch (-1: not run)
  std::string calib_note;
  herro::ModelScratch S{};
  uint32_t scratch_cap = 0;
  void* sib_kv = nullptr;       // sibling tiles of the f16 stack (ensure_sib): K / V exchange, flags + error word
  void* sib_flag = nullptr;
  uint32_t sib_cap = 0;
  std::vector<void*> scratch_allocs;
  herro::KernelTimer timer;
  // job memory: ONE device arena and ONE pinned host arena per job, recycled through these free lists (a job used to
  // cost 36 hipMallocs + a hipHostMalloc, ~4 ms per 4096 windows, and its descriptors went up from pageable memory)
  std::unique_ptr<HostPool> pool;
  std::mutex arena_mu;
  std::vector<Arena> free_scan, free_stage;            // device op array + staged CIGAR text of a job; pinned staging of one herro_job_create
  hipStream_t prep_stream = nullptr;                   // CIGAR scan of the job being created: its own (high-priority) stream, so that it does not queue behind the pileup / model kernels of earlier jobs
  hipEvent_t prep_ev = nullptr;
  unsigned long long* d_prof = nullptr;                // HERRO_PROF_BUILD + HERRO_PROF=1: per-kernel phase cycles (job_dev.h PROF_MARK), printed by herro_destroy
  bool dev_scan = true;                                // HERRO_HOST_SCAN=1: decode the text on the host instead (A/B, debugging)
  bool dev_build = true;                               // windows and descriptors on the device behind the scan (build_dev.hip); herro_debug_set_host_build(ctx, 1): by the host from the cut records, as until round 5
  std::vector<Arena> free_dev, free_pin, free_small;   // free_small: the buffers a job needs only once its counts are known (logits, batch descriptors)
  std::atomic<uint32_t> live_jobs{0};   // herro_job_create may run on another thread than the context's execution calls
  uint64_t reads_gen = 0;   // bumped by herro_set_reads: a job built on an older store refuses to run
  uint32_t n_sib_retry = 0;        // model passes repeated without sibling tiles (sib_retry)
  std::vector<herro_job*> sib_suspects;   // jobs whose last model pass launched sibling tiles and has not been seen clean yet (check_sib): a raised error word is theirs
  std::atomic<int> n_pending{0};   // jobs of this context that are featurized and not yet inferred: > 0 when herro_job_featurize is called means the caller pipelines its jobs
  std::atomic<int> create_code{0};   // HERRO_E_* of the last herro_job_create that returned NULL (herro_job_create_status)
};

HostPool& host_pool(herro_ctx* ctx);   // herro_api.hip: the context's pool, created on first use
std::shared_ptr<void> make_store_owner(int dev, void* const ptrs[6]);   // herro_api.hip: what a context's store_owner holds (herro_set_reads, herro_store_cut)
