// herro_api.hip — C ABI (include/herro_amd.h) over the HIP kernels.  Host C++ (compiled by hipcc).
// No CPU fallback anywhere: if HIP is unavailable every device call returns HERRO_E_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <chrono>
#include <map>
#include <memory>
#include <string>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/herro_amd.h"
#include "api_ctx.h"
#include "aligned_dev.h"
#include "host_cpus.h"
#include "job_dev.h"
#include "model_dev.h"
#include "model_pack.h"
#include "infer_plan.h"
#include "windowing.hpp"
#include "build_dev.h"
#include "cigar_dev.h"
#include "job_layout.h"
#include "align_dev.h"
#include "overlap_dev.h"
#include "fasta_dev.h"

using namespace herro;

namespace {
std::string g_create_err;

// HERRO_HOST_PROFILE=2: one stderr line per API call with its start time and duration (host-side timeline of a pipeline).
struct ProfSpan {
  static int level() { static const int l = [] { const char* e = getenv("HERRO_HOST_PROFILE"); return e ? atoi(e) : 0; }(); return l; }
  static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
  const void* who; const char* name; double t0;
  ProfSpan(const void* w, const char* n) : who(w), name(n), t0(level() >= 2 ? now_ms() : 0) {}
  ~ProfSpan() { if (level() >= 2) { const double t1 = now_ms(); fprintf(stderr, "TL %p %-14s %.3f %.3f\n", who, name, fmod(t0, 1e6), t1 - t0); } }
};

template <typename T>
T* dev_alloc_copy(const std::vector<T>& v, hipStream_t st, hipError_t& err) {
  T* p = nullptr;
  const size_t bytes = std::max<size_t>(v.size(), 1) * sizeof(T);
  err = hipMalloc((void**)&p, bytes);
  if (err != hipSuccess) return nullptr;
  if (!v.empty()) err = hipMemcpyAsync(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, st);
  return p;
}
}  // namespace

// vector whose resize() leaves trivially-constructible elements uninitialised: the big job arrays are filled by
// the thread pool right after, so zeroing them (and first-touching their pages) on one thread was pure cost
template <class T>
struct dinit_alloc : std::allocator<T> {
  template <class U> struct rebind { using other = dinit_alloc<U>; };
  template <class U> void construct(U* p) noexcept { ::new ((void*)p) U; }
  template <class U, class... A> void construct(U* p, A&&... a) { ::new ((void*)p) U(std::forward<A>(a)...); }
};
template <class T> using uvec = std::vector<T, dinit_alloc<T>>;

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
  ~herro_job();   // returns the arenas, the small buffers and the events
  herro_ctx* ctx = nullptr;
  // ---- build (herro_job_create*): descriptors, arenas, what was left out
  uint32_t W = 0, n_targets = 0;
  harr<WinDesc> win;
  harr<OwDesc> ow;
  harr<uint32_t> ops;
  std::vector<uint32_t> tgt_win_off;  // [n_targets+1]
  harr<uint32_t> tile_win, tile_r0;
  JobDev J{};
  Arena dev{}, pin{};              // device arena (descriptors + every scratch / result array), pinned host arena
  Arena scan{};                    // device: the op array written by the CIGAR scan (+ the staged text it was read from)
  uint64_t scan_ops = 0;           // slots in it
  std::vector<uint32_t> dbg_ops;   // herro_debug_job_array(ops) of such a job: fetched on demand
  bool dev_built = false;          // windows and descriptors were built on the device (build_dev.hip): the overlap descriptors and the tile list exist there only
  std::vector<OwDesc> dbg_ow;      // ... and come down for herro_debug_job_array
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

// herro_debug_job_array: n elements of a job's device array, behind everything the device has in flight, into the debug vector v
template <class T>
static int64_t debug_fetch(herro_job* job, std::vector<T>& v, const void* d_src, size_t n, const void** ptr) {
  v.resize(n);
  if (hipSetDevice(job->ctx->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
      (n && hipMemcpy(v.data(), d_src, n * sizeof(T), hipMemcpyDeviceToHost) != hipSuccess)) return HERRO_E_NO_DEVICE;
  *ptr = v.data();
  return (int64_t)n;
}

static int job_sync(herro_job* job);
static int ensure_logits(herro_job* job, uint64_t rows);

HostPool& host_pool(herro_ctx* ctx) {
  if (!ctx->pool) {
    const uint32_t cpus = usable_cpus();
    const char* env = getenv("HERRO_HOST_THREADS");
    // several contexts share the host (one or two per GPU): a quarter of the hardware threads each, never more than the
    // CPU quota.  Two pools of 128 on 256 hardware threads measured 50 ms builds (2-7 ms alone).
    const uint32_t want = env ? (uint32_t)std::max(1, atoi(env)) : std::min(std::min(std::max(std::thread::hardware_concurrency() / 4u, 1u), 64u), cpus);
    ctx->pool = std::make_unique<HostPool>(want - 1);  // the calling thread works too
  }
  return *ctx->pool;
}

// late, small device buffers of a job (sized by results): recycled per context like the arenas — hipMalloc / hipFree
// synchronise the whole device, which would serialise the feeder threads of a GPU on every job
static Arena small_acquire(herro_ctx* ctx, size_t need) {
  Arena a;
  { std::lock_guard<std::mutex> lk(ctx->arena_mu); a = best_fit_take(ctx->free_small, need); }
  if (a.p) return a;
  a.cap = need + need / 4 + 4096;
  if (hipMalloc(&a.p, a.cap) != hipSuccess) { a.p = nullptr; a.cap = 0; }
  return a;
}
static void small_release(herro_ctx* ctx, Arena& a) {
  if (!a.p) return;
  std::lock_guard<std::mutex> lk(ctx->arena_mu);
  if (ctx->free_small.size() < 24) ctx->free_small.push_back(a); else (void)hipFree(a.p);
  a = Arena{};
}

// A job-sized block from one of the context's free lists (best fit), or a fresh one with 12 % slack.
// kind: 0 pinned host, 1 device; host-only contexts get plain malloc.
static Arena arena_acquire(herro_ctx* ctx, std::vector<Arena>& list, size_t need, int kind) {
  Arena a;
  { std::lock_guard<std::mutex> lk(ctx->arena_mu); a = best_fit_take(list, need); }
  if (a.p) return a;
  a.cap = need + need / 8 + 4096;
  if (ctx->host_only) a.p = std::malloc(a.cap);
  else if (kind == 1) { if (hipMalloc(&a.p, a.cap) != hipSuccess) a.p = nullptr; }
  else if (hipHostMalloc(&a.p, a.cap, hipHostMallocDefault) != hipSuccess) a.p = nullptr;
  if (!a.p) a.cap = 0;
  return a;
}
// ... and back: a list keeps a handful of blocks for the next jobs (the bench cycles 2-4 jobs per context); the rest goes back to where it came from
static void arena_release(herro_ctx* ctx, std::vector<Arena>& list, Arena& a, int kind) {
  if (!a.p) return;
  std::lock_guard<std::mutex> lk(ctx->arena_mu);
  if (list.size() < 6) list.push_back(a);
  else if (ctx->host_only) std::free(a.p);
  else if (kind == 1) (void)hipFree(a.p);
  else (void)hipHostFree(a.p);
  a = Arena{};
}

// Whatever a job holds of its context goes back when it is destroyed, so a herro_job_create that fails half way just lets go of the job.  Nothing of the
// job may be in flight by then: herro_job_free waits for the stream first, a failed create has waited for whatever it enqueued.
herro_job::~herro_job() {
  if (!ctx) return;
  arena_release(ctx, ctx->free_dev, dev, 1);
  arena_release(ctx, ctx->free_scan, scan, 1);
  arena_release(ctx, ctx->free_pin, pin, 0);
  small_release(ctx, a_logits);
  small_release(ctx, a_bdesc);
  small_release(ctx, a_supoff);
  small_release(ctx, a_supoff_dev);
  if (ev_counts) (void)hipEventDestroy(ev_counts);
  if (ev_blob) (void)hipEventDestroy(ev_blob);
}

static constexpr uint32_t FUSED_MAX_SIB = 8;     // sibling tiles of one window in the f16 stack (k_layers_p<., 4, true>): windows of up to 512 informative rows stay fused (the plan in infer_plan.h never reads it; tests/capacity_cases.py reads it here)
// Most informative rows of a window that stays on the fused stack: 64 (one tile), or 64 * FUSED_MAX_SIB with the f16 stack, which
// spreads a larger window over sibling tiles (HERRO_FUSED_BIG=0: such windows go layer by layer as before, for A/B).
static uint32_t fused_tok_cap(const herro_ctx* ctx) {
  static const bool big = ab_env("HERRO_FUSED_BIG", 1) != 0;
  return (big && ctx->precision >= 4 && model_h_supported(ctx->M)) ? FUSED_MAX_TOK * FUSED_MAX_SIB : FUSED_MAX_TOK;
}
// K / V exchange buffers and flags of `n_tiles_b` sibling tiles (128 KB per tile)
static int ensure_sib(herro_ctx* ctx, uint32_t n_tiles_b) {
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
// The error word of the sibling tiles, read where logits / corrected bases come back to the host (the stream has been synchronised: every model pass queued so far
// is complete).  The word carries no job identity, so a raised word taints EVERY job whose sibling-tile pass has not been seen clean yet (ctx->sib_suspects): all of
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
// One wave reads the shader clock counter (s_memtime) and the constant-rate one (s_memrealtime) around ~40 us of dependent adds: the ratio is the shader clock
// the chip runs at right behind whatever the stream just executed (bench.py's `sustained` leg samples it; the release kernels carry no timers)
__global__ void k_clock_probe(unsigned long long* out, uint32_t spin) {
  const unsigned long long c0 = clock64(), w0 = wall_clock64();
  uint32_t x = threadIdx.x;
  for (uint32_t i = 0; i < spin; i++) x = x * 1664525u + 1013904223u;
  const unsigned long long c1 = clock64(), w1 = wall_clock64();
  if (threadIdx.x == 0) { out[0] = c1 - c0; out[1] = w1 - w0; out[2] = x; }
}

static void run_model(herro_ctx* ctx, const BatchDev& B, bool tiled) {
  if (B.n_tok == 0) return;
  const int p = ctx->precision;
  const uint32_t cu = ctx->front_cu ? ctx->front_cu : ctx->n_cu;   // the front end's own count (herro_debug_set_front_cu); the tile plan took ctx->n_cu
  if (!tiled) { launch_model(ctx->M, B, ctx->S, (p == 1 || p >= 4) ? 3 : p, ctx->stream, &ctx->timer, cu, &ctx->front_ran); return; }
  if (p >= 4) launch_model_h(ctx->M, B, ctx->S, p == 4 ? 2 : (p == 6 ? 3 : (p == 7 ? 21 : (p == 8 ? 12 : 1))), ctx->stream, &ctx->timer, cu, ctx->conv_fc, &ctx->front_ran);
  else launch_model(ctx->M, B, ctx->S, p, ctx->stream, &ctx->timer, cu, &ctx->front_ran);
}

extern "C" {

const char* herro_version(void) { return "herro_amd 0.1 (gfx950)"; }

const char* herro_last_error(const herro_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

herro_ctx* herro_create(int device_id) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    g_create_err = std::string("no HIP device: ") + (e != hipSuccess ? hipGetErrorString(e) : "device count 0");
    return nullptr;
  }
  if (device_id < 0 || device_id >= n) { g_create_err = "device id out of range"; return nullptr; }
  if ((e = hipSetDevice(device_id)) != hipSuccess) { g_create_err = hipGetErrorString(e); return nullptr; }
  auto ctx = std::make_unique<herro_ctx>();
  ctx->device = device_id;
  if ((e = hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking)) != hipSuccess) {
    g_create_err = hipGetErrorString(e);
    return nullptr;
  }
  ctx->stream = ctx->own_stream;
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess && cus > 0) ctx->n_cu = (uint32_t)cus;
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);   // hi = numerically lowest = highest priority
    if ((e = hipStreamCreateWithPriority(&ctx->prep_stream, hipStreamNonBlocking, hi)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&ctx->prep_ev, hipEventDisableTiming | hipEventBlockingSync)) != hipSuccess) {
      g_create_err = hipGetErrorString(e);
      return nullptr;
    }
#ifdef HERRO_PROF_BUILD
    if (const char* pe = getenv("HERRO_PROF"); pe && atoi(pe)) {
      if (hipMalloc((void**)&ctx->d_prof, 256 * 32 * 8) == hipSuccess) (void)hipMemset(ctx->d_prof, 0, 256 * 32 * 8); else ctx->d_prof = nullptr;
    }
#endif
    ctx->dev_scan = ab_env("HERRO_HOST_SCAN", 0) == 0;
    { const char* e = getenv("HERRO_HOST_BUILD"); ctx->dev_build = !(e && atoi(e)); }   // HERRO_HOST_BUILD=1: windows and descriptors by the host, as until round 5 (same results; for comparisons)
  }
  // ln(k+1) table from the host libm — what Rust's f64::ln calls on Linux (features.rs:507)
  std::vector<double> ln(1u << 20);
  for (size_t k = 0; k < ln.size(); k++) ln[k] = std::log((double)k + 1.0);
  ctx->d_ln = dev_alloc_copy(ln, ctx->stream, e);
  if (e != hipSuccess) { g_create_err = hipGetErrorString(e); return nullptr; }
  if ((e = hipStreamSynchronize(ctx->stream)) != hipSuccess) { g_create_err = hipGetErrorString(e); return nullptr; }
  ctx->ln_n = (uint32_t)ln.size();
  return ctx.release();
}

static void free_all(std::vector<void*>& v) {
  for (void* p : v) if (p) (void)hipFree(p);
  v.clear();
}

void herro_destroy(herro_ctx* ctx) {
  if (!ctx) return;
  if (ctx->host_only) { for (Arena& a : ctx->free_pin) std::free(a.p); delete ctx; return; }
  (void)hipSetDevice(ctx->device);   // teardown: nothing to report errors to
  (void)hipDeviceSynchronize();
  if (ctx->d_prof) {
    std::vector<unsigned long long> raw(256 * 32);
    unsigned long long h[256] = {0};
    if (hipMemcpy(raw.data(), ctx->d_prof, raw.size() * 8, hipMemcpyDeviceToHost) == hipSuccess) {
      for (int i = 0; i < 256; i++) for (int sh = 0; sh < 32; sh++) h[i] += raw[(size_t)i * 32 + sh];
      for (int k = 0; k < 16; k++)
        if (h[k * 16 + 15]) {
          fprintf(stderr, "PROF kernel %d (%llu workgroups), cycles per workgroup by phase:", k, h[k * 16 + 15]);
          for (int ph = 0; ph < 15; ph++) if (h[k * 16 + ph]) fprintf(stderr, " %d:%.0f", ph, (double)h[k * 16 + ph] / (double)h[k * 16 + 15]);
          fprintf(stderr, "\n");
        }
    }
    (void)hipFree(ctx->d_prof);
#ifdef HERRO_PROF_BUILD
    model_h_prof_dump();
#endif
  }
  ctx->timer.reset();
  ctx->store_owner.reset();   // the read store goes with its last holder
  if (ctx->d_ln) (void)hipFree(ctx->d_ln);
  free_all(ctx->model_allocs);
  free_all(ctx->scratch_allocs);
  if (ctx->sib_kv) (void)hipFree(ctx->sib_kv);
  if (ctx->sib_flag) (void)hipFree(ctx->sib_flag);
  for (Arena& a : ctx->free_dev) (void)hipFree(a.p);
  for (Arena& a : ctx->free_pin) (void)hipHostFree(a.p);
  for (Arena& a : ctx->free_small) (void)hipFree(a.p);
  for (Arena& a : ctx->free_scan) (void)hipFree(a.p);
  for (Arena& a : ctx->free_stage) (void)hipHostFree(a.p);
  if (ctx->prep_ev) (void)hipEventDestroy(ctx->prep_ev);
  if (ctx->prep_stream) (void)hipStreamDestroy(ctx->prep_stream);
  if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
  delete ctx;
}

int herro_set_stream(herro_ctx* ctx, void* s) {
  if (!ctx) return HERRO_E_INVALID;
  if (ctx->host_only) return HERRO_OK;   // no device, no stream
  const hipStream_t to = s ? (hipStream_t)s : ctx->own_stream;
  if (to == ctx->stream) return HERRO_OK;
  // A switch orders: everything this context has queued on the stream it leaves is complete before anything runs on the new one.  Queued work is
  // normal here (herro_job_featurize returns with k_rfq queued, herro_job_infer with the descriptor upload and the whole model), the next call reads
  // what it writes, and every guard in front of recycled memory (herro_job_free, ensure_sib / ensure_logits / ensure_scratch) waits for ctx->stream
  // alone — so the stream that is left must be idle.  The call is rare: the wait is the simple way.  (Work on prep_stream never outlives the call
  // that queued it: herro_job_create waits for prep_ev itself.)
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->stream = to;
  return HERRO_OK;
}

int herro_synchronize(herro_ctx* ctx) {
  if (!ctx) return HERRO_E_INVALID;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->timer.collect();
  return HERRO_OK;
}

// ---- codec ---------------------------------------------------------------------------------------
// A table instead of a switch: random bases make every case a mispredicted branch (0.1 Gbases/s); whole words of plain ACGT / acgt take the
// table path, a word with anything else goes through the reference's byte-by-byte rule (the 255 of a non-ACGT byte is OR-ed in UNMASKED,
// haec_io.rs:126-128, and a byte >= 128 is its panic).
static const uint8_t* enc_table() {
  static const struct T {
    uint8_t t[256];
    T() {
      for (int i = 0; i < 256; i++) t[i] = 255;
      t[(int)'A'] = t[(int)'a'] = 0; t[(int)'C'] = t[(int)'c'] = 1; t[(int)'G'] = t[(int)'g'] = 2; t[(int)'T'] = t[(int)'t'] = 3;
    }
  } tab;
  return tab.t;
}
int64_t herro_encode_2bit(const uint8_t* seq, uint64_t n, uint64_t* words) {
  const uint8_t* T = enc_table();
  uint64_t nw = 0;
  for (uint64_t i = 0; i < n;) {
    const uint32_t m = (uint32_t)std::min<uint64_t>(32, n - i);
    uint64_t block = 0;
    uint32_t seen = 0;
    if (m == 32) {
#pragma unroll
      for (int j = 0; j < 32; j++) {
        const uint32_t c = T[seq[i + j]];
        seen |= c;
        block |= (uint64_t)(c & 3u) << (2 * j);
      }
    } else {
      for (uint32_t j = 0; j < m; j++) {
        const uint32_t c = T[seq[i + j]];
        seen |= c;
        block |= (uint64_t)(c & 3u) << (2 * j);
      }
    }
    if (seen & 0x80u) {   // something that is not ACGT / acgt in this word: the reference's rule, byte by byte
      block = 0;
      for (uint32_t j = 0; j < m; j++) {
        const uint8_t b = seq[i + j];
        if (b >= 128) return HERRO_E_REFERENCE_PANIC;
        block |= (uint64_t)T[b] << (2 * j);   // 255, unmasked: it spills over the next three bases (and off the word's end)
      }
    }
    words[nw++] = block;
    i += m;
  }
  return (int64_t)nw;
}

int herro_decode_2bit(const uint64_t* words, uint64_t length, uint64_t start, uint64_t end, int rc,
                      uint8_t* out) {
  if (end > length) return HERRO_E_REFERENCE_PANIC;  // "Out of bounds for 2-bit sequence decoding."
  static const char D[4] = {'A', 'C', 'G', 'T'};
  for (uint64_t k = 0; start + k < end; k++) {
    const uint64_t i = rc ? end - 1 - k : start + k;
    const uint64_t code = ((words[i >> 5] >> ((i << 1) & 63)) & 3) ^ (rc ? 3 : 0);
    out[k] = (uint8_t)D[code];
  }
  return HERRO_OK;
}

// ---- read store ----------------------------------------------------------------------------------
}  // extern "C"
// The owner of a store's six device arrays (api_ctx.h): freed on their device when the last context holding the owner lets go.
std::shared_ptr<void> make_store_owner(int dev, void* const ptrs[6]) {
  struct Owned { int dev; void* p[6]; };
  return std::shared_ptr<void>(new Owned{dev, {ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], ptrs[5]}}, [](void* v) {
    Owned* o = (Owned*)v;
    int cur = 0;
    const bool have = hipGetDevice(&cur) == hipSuccess;
    (void)hipSetDevice(o->dev);
    for (void* q : o->p) if (q) (void)hipFree(q);
    if (have) (void)hipSetDevice(cur);
    delete o;
  });
}
extern "C" {

static int upload_reads(herro_ctx* ctx, uint32_t n_reads, const std::vector<uint64_t>& words,
                        const std::vector<uint64_t>& word_off, const uint8_t* qual,
                        const std::vector<uint64_t>& qual_off, const uint32_t* name_class) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // nothing may still read the store that is about to be replaced
  ctx->store_owner.reset();   // frees the previous store unless another context of the device still shares it
  ctx->d_p0 = nullptr; ctx->d_p1 = nullptr;
  ctx->d_words = nullptr; ctx->d_word_off = nullptr; ctx->d_qual = nullptr; ctx->d_qual_off = nullptr;
  hipError_t e;
  // an error part way through (out of memory, a failed copy) must not leak what was allocated so far: until the owner
  // below takes the six arrays over, this guard frees them and leaves the context without a store
  struct Partial {
    herro_ctx* c; bool armed = true;
    ~Partial() {
      if (!armed) return;
      void* p[6] = {(void*)c->d_words, (void*)c->d_word_off, (void*)c->d_qual, (void*)c->d_qual_off, (void*)c->d_p0, (void*)c->d_p1};
      for (void* q : p) if (q) (void)hipFree(q);
      c->d_words = nullptr; c->d_word_off = nullptr; c->d_qual = nullptr; c->d_qual_off = nullptr; c->d_p0 = nullptr; c->d_p1 = nullptr;
    }
  } partial{ctx};
  std::vector<uint64_t> wp(words);
  wp.push_back(0);  // pad word: get16() may touch one word past a read
  ctx->d_words = dev_alloc_copy(wp, ctx->stream, e); HIP_TRY(ctx, e);
  {  // bit-plane copy of the same bases (pass 1 counts symbols bit-sliced): even / odd bits of every word, compacted
    std::vector<uint32_t> p0(words.size() + 2, 0), p1(words.size() + 2, 0);
    auto compact = [](uint64_t t) -> uint32_t {  // bits 0, 2, 4, ... of t -> bits 0, 1, 2, ...
      t &= 0x5555555555555555ull;
      t = (t | (t >> 1)) & 0x3333333333333333ull;
      t = (t | (t >> 2)) & 0x0f0f0f0f0f0f0f0full;
      t = (t | (t >> 4)) & 0x00ff00ff00ff00ffull;
      t = (t | (t >> 8)) & 0x0000ffff0000ffffull;
      t = (t | (t >> 16)) & 0x00000000ffffffffull;
      return (uint32_t)t;
    };
    const size_t CH = 1u << 16, nch = (words.size() + CH - 1) / CH;
    host_pool(ctx).run((uint32_t)nch, [&](uint32_t c) {
      const size_t a = c * CH, b = std::min(words.size(), a + CH);
      for (size_t i = a; i < b; i++) { p0[i] = compact(words[i]); p1[i] = compact(words[i] >> 1); }
    });
    ctx->d_p0 = dev_alloc_copy(p0, ctx->stream, e); HIP_TRY(ctx, e);
    ctx->d_p1 = dev_alloc_copy(p1, ctx->stream, e); HIP_TRY(ctx, e);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // p0 / p1 go out of scope below
  }
  ctx->d_word_off = dev_alloc_copy(word_off, ctx->stream, e); HIP_TRY(ctx, e);
  ctx->d_qual_off = dev_alloc_copy(qual_off, ctx->stream, e); HIP_TRY(ctx, e);
  const uint64_t nq = qual_off[n_reads];
  HIP_TRY(ctx, hipMalloc((void**)&ctx->d_qual, std::max<uint64_t>(nq, 1) + 8));
  ctx->qual_bytes = nq;
  ctx->n_words = words.size();
  if (nq) HIP_TRY(ctx, hipMemcpyAsync(ctx->d_qual, qual, nq, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->n_reads = n_reads;
  ctx->h_word_off = word_off;
  ctx->h_qual_off = qual_off;
  ctx->read_len.resize(n_reads);
  for (uint32_t i = 0; i < n_reads; i++) ctx->read_len[i] = (uint32_t)(qual_off[i + 1] - qual_off[i]);
  ctx->name_class.resize(n_reads);
  for (uint32_t i = 0; i < n_reads; i++) ctx->name_class[i] = name_class ? name_class[i] : i;
  ctx->read_bytes = words.size() * 8 + nq;
  ctx->reads_gen++;   // jobs built on the previous store hold descriptors into freed memory: they refuse to run from here on
  {
    void* const ptrs[6] = {(void*)ctx->d_words, (void*)ctx->d_word_off, (void*)ctx->d_qual, (void*)ctx->d_qual_off, (void*)ctx->d_p0, (void*)ctx->d_p1};
    ctx->store_owner = make_store_owner(ctx->device, ptrs);
    partial.armed = false;
  }
  return HERRO_OK;
}

int herro_share_reads(herro_ctx* ctx, const herro_ctx* from) {
  if (!ctx || !from || ctx == from) return HERRO_E_INVALID;
  if (ctx->host_only || from->host_only) return HERRO_E_INVALID;
  if (ctx->device != from->device) { ctx->err = "herro_share_reads: the contexts are on different devices"; return HERRO_E_INVALID; }
  if (!from->store_owner) { ctx->err = "herro_share_reads: the source context has no read store"; return HERRO_E_STATE; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // nothing may still read the store that is about to be replaced
  ctx->store_owner = from->store_owner;
  ctx->d_words = from->d_words; ctx->d_word_off = from->d_word_off; ctx->d_qual = from->d_qual; ctx->d_qual_off = from->d_qual_off;
  ctx->d_p0 = from->d_p0; ctx->d_p1 = from->d_p1;
  ctx->qual_bytes = from->qual_bytes; ctx->n_words = from->n_words; ctx->read_bytes = from->read_bytes;
  ctx->n_reads = from->n_reads;
  ctx->h_word_off = from->h_word_off; ctx->h_qual_off = from->h_qual_off;
  ctx->read_len = from->read_len; ctx->name_class = from->name_class;
  ctx->reads_gen++;
  return HERRO_OK;
}

int herro_set_reads(herro_ctx* ctx, uint32_t n_reads, const uint8_t* seq, const uint8_t* qual,
                    const uint64_t* off, const uint32_t* name_class) {
  if (!ctx || (n_reads && (!seq || !qual || !off))) return HERRO_E_INVALID;
  std::vector<uint64_t> word_off(n_reads + 1, 0), qual_off(off, off + n_reads + 1);
  for (uint32_t i = 0; i < n_reads; i++) {
    if (off[i + 1] < off[i] || off[i + 1] - off[i] > 0xffffffffull) { ctx->err = "bad read offsets"; return HERRO_E_INVALID; }
    word_off[i + 1] = word_off[i] + (off[i + 1] - off[i] + 31) / 32;
  }
  std::vector<uint64_t> words(word_off[n_reads]);
  std::atomic<int64_t> bad{-1};
  host_pool(ctx).run(n_reads, [&](uint32_t i) {
    if (herro_encode_2bit(seq + off[i], off[i + 1] - off[i], words.data() + word_off[i]) < 0) bad.store((int64_t)i);
  });
  if (bad.load() >= 0) { ctx->err = "read " + std::to_string(bad.load()) + ": byte >= 128 in sequence"; return HERRO_E_REFERENCE_PANIC; }
  // qualities are addressed relative to off[0]
  std::vector<uint64_t> qo(n_reads + 1);
  for (uint32_t i = 0; i <= n_reads; i++) qo[i] = off[i] - off[0];
  return upload_reads(ctx, n_reads, words, word_off, qual + off[0], qo, name_class);
}

int herro_set_reads_packed(herro_ctx* ctx, uint32_t n_reads, const uint64_t* words, const uint64_t* word_off,
                           const uint8_t* qual, const uint64_t* qual_off, const uint32_t* name_class) {
  if (!ctx || (n_reads && (!words || !word_off || !qual || !qual_off))) return HERRO_E_INVALID;
  std::vector<uint64_t> w(words + word_off[0], words + word_off[n_reads]);
  std::vector<uint64_t> wo(n_reads + 1), qo(n_reads + 1);
  for (uint32_t i = 0; i <= n_reads; i++) { wo[i] = word_off[i] - word_off[0]; qo[i] = qual_off[i] - qual_off[0]; }
  return upload_reads(ctx, n_reads, w, wo, qual + qual_off[0], qo, name_class);
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

int herro_debug_set_host_build(herro_ctx* ctx, int on) {
  if (!ctx) return HERRO_E_INVALID;
  ctx->dev_build = on == 0;
  return HERRO_OK;
}

int herro_debug_job_dev_built(const herro_job* job) { return job ? (job->dev_built && !job->from_ops_text ? 1 : 0) : HERRO_E_INVALID; }

int herro_debug_force_precision(herro_ctx* ctx, int on) {
  if (!ctx) return HERRO_E_INVALID;
  ctx->debug_force_precision = on != 0;
  return HERRO_OK;
}

static int ensure_scratch(herro_ctx* ctx, uint32_t n_tok) {
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


namespace {
// Everything herro_job_create derives from ONE target read, with target-local offsets.
struct TargetOut {
  BuildError err;
  std::vector<uint32_t> ops;
  std::vector<OwDesc> ow;    // win / cls / op_begin / scr_off are target-local
  std::vector<WinDesc> win;  // ow_begin target-local; device offsets filled at merge
  uint32_t n_cls = 0;
  uint64_t scr_ops = 0, alg_read_bytes = 0, alg_op_bytes = 0;
  uint32_t n_skipped = 0;   // alignments left out (see skip() in build_target)
  std::vector<std::pair<uint32_t, std::vector<uint32_t>>> op_patches;   // device-scan mode: (slot, ops) of texts only the host could read (e.g. 11+ digit zero padding)
  bool failed = false;      // the whole target was left without overlaps
  std::string first_skip;
};

// Results of the device CIGAR scan of a job's alignments (pinned host copies), indexed like the job's alignment range.
struct DevScanView { const CigIn* in; const CigOut* out; const CigCut* cuts; };

// ds == nullptr: the text is decoded here (scan_cigar) and the ops collect in out.ops.  Otherwise the ops are already in
// the job's device op array (at in[g].op_off, absolute) and only the scan's cut records are read; g0 = index of the
// target's first alignment in the scan arrays.
void build_target(const herro_ctx* ctx, uint32_t rid, const herro_alignment* alns, uint32_t n_aln, uint32_t W,
                  TargetOut& out, const DevScanView* ds = nullptr, uint64_t g0 = 0) {
  auto fail = [&](int code, const std::string& m) { out.err = BuildError{code, m}; };
  if (rid >= ctx->n_reads) return fail(HERRO_E_REFERENCE_PANIC, "target rid out of range (reads[rid])");
  const uint32_t tlen = ctx->read_len[rid];
  const uint32_t n_windows = (tlen + W - 1) / W;  // features.rs:338
  if (n_windows > 65535) return fail(HERRO_E_UNSUPPORTED, "more than 65535 windows in a read (wid is u16 in the reference)");
  // collect (window, overlap) in alignment order, then bucket by window (stable)
  struct Tmp { HostOw h; uint32_t op_base; uint32_t aln; };
  std::vector<Tmp> tmp;
  CigarScan cs;
  std::vector<HostOw> hows;
  std::unordered_map<uint32_t, uint32_t> cls_of_name;  // name class -> accumulator slot
  std::unordered_map<uint32_t, uint32_t> seen_qid;
  // Alignments parse_paf itself would have dropped before extract_features ever saw them (self overlaps, a second
  // alignment of a (query, target) pair — overlaps.rs:175-185) are left out and counted (herro_job_skipped).  Everything
  // else the reference processes is processed — consecutive insertion ops, an alignment that starts inside a window with
  // an insertion, any number of overlaps per window.  Inputs on which the reference PANICS fail the call: the reference
  // would have aborted the run there (Cargo.toml:18).
  auto skip = [&](uint32_t a, const char* why) {
    if (!out.n_skipped++) out.first_skip = "target rid " + std::to_string(rid) + ", alignment " + std::to_string(a) + " (qid " + std::to_string(alns[a].qid) + "): " + why;
  };
  std::vector<uint32_t> spare_ops;   // device-scan mode: ops of the rare alignment the host has to read itself
  if (!ds) {
    size_t op_room = 0;
    for (uint32_t a = 0; a < n_aln; a++) op_room += alns[a].cigar_len / 2 + 1;
    out.ops.reserve(op_room);
  }
  for (uint32_t a = 0; a < n_aln; a++) {
    const herro_alignment& al = alns[a];
    if (al.tid != rid) return fail(HERRO_E_INVALID, "alignment tid != target rid (parse_paf groups by target, overlaps.rs:189-192)");
    if (al.qid >= ctx->n_reads) return fail(HERRO_E_REFERENCE_PANIC, "alignment qid out of range");
    if (al.qid == rid) { skip(a, "self overlap (dropped by parse_paf, overlaps.rs:175-179)"); continue; }
    if (seen_qid.count(al.qid)) { skip(a, "second alignment of the same (query,target) pair (dropped by parse_paf, overlaps.rs:181-185)"); continue; }
    seen_qid[al.qid] = a;
    if (al.tlen != tlen) return fail(HERRO_E_INVALID, "alignment tlen differs from the stored read length");
    if (al.qend > ctx->read_len[al.qid] || al.tend > tlen) return fail(HERRO_E_REFERENCE_PANIC, "alignment coordinates exceed the read length");
    BuildError be;
    uint32_t op_base;
    if (ds) {
      const CigIn& ci = ds->in[g0 + a];
      const CigOut& co = ds->out[g0 + a];
      op_base = ci.op_off;
      if (co.flags & ~(uint32_t)CIG_INS_PAIR) {   // rare: malformed text (the message comes from here), more cuts than the coordinates allow
        spare_ops.resize((size_t)al.cigar_len / 2 + 1);
        if (!scan_cigar(al.cigar, al.cigar_len, al.tstart, W, spare_ops.data(), cs, be)) return fail(be.code, be.msg);
        if (co.flags & CIG_MALFORMED)   // legal text the kernel does not read (lengths padded to 11+ digits): its ops go up from here
          out.op_patches.emplace_back(ci.op_off, std::vector<uint32_t>(spare_ops.begin(), spare_ops.begin() + cs.n_ops));
      } else {
        cs.n_ops = co.n_ops; cs.t_end = co.t_end; cs.q_end = co.q_end; cs.ins_end = co.ins_end; cs.op0 = co.op0; cs.opn = co.opn;
        cs.ins_pairs.clear(); cs.cuts.clear();
        for (uint32_t c = 0; c < co.n_cuts; c++) {
          const CigCut& k = ds->cuts[ci.cut_off + c];
          cs.cuts.push_back(Cut{k.k, k.t, k.q, k.ins, k.o0, k.o1, k.o2});
        }
        std::sort(cs.cuts.begin(), cs.cuts.end(), [](const Cut& x, const Cut& y) { return x.k < y.k; });   // discovery order on the device
      }
    } else {
      // the ops are decoded straight into the target's op array (one pass over the text, scan_cigar); they stay there
      // only if the alignment contributes a window
      op_base = (uint32_t)out.ops.size();
      out.ops.resize((size_t)op_base + al.cigar_len / 2 + 1);
      if (!scan_cigar(al.cigar, al.cigar_len, al.tstart, W, out.ops.data() + op_base, cs, be)) return fail(be.code, be.msg);
    }
    hows.clear();
    if (!window_cuts(cs, al, W, n_windows, hows, be)) return fail(be.code, be.msg);
    if (!ds) out.ops.resize((size_t)op_base + (hows.empty() ? 0u : cs.n_ops));
    for (auto& h : hows) tmp.push_back(Tmp{h, op_base, a});
    const uint32_t nc = ctx->name_class[al.qid];
    if (!cls_of_name.count(nc)) cls_of_name[nc] = out.n_cls++;
  }
  std::vector<uint32_t> cnt(n_windows + 1, 0);
  for (auto& x : tmp) cnt[x.h.win + 1]++;
  for (uint32_t i = 0; i < n_windows; i++) cnt[i + 1] += cnt[i];
  out.ow.resize(tmp.size());
  std::vector<uint32_t> fill(cnt.begin(), cnt.end() - 1);
  std::vector<uint64_t> ins_sum(n_windows, 0);
  for (auto& x : tmp) {
    const herro_alignment& al = alns[x.aln];
    const uint32_t wi = x.h.win;
    const uint32_t win_start = wi * W;
    const uint32_t win_len = (wi == n_windows - 1) ? tlen - wi * W : W;
    OwDesc d{};
    d.win = wi;
    d.qid = al.qid;
    d.cls = cls_of_name[ctx->name_class[al.qid]];
    d.tstart = x.h.tstart;
    d.qlen = x.h.qend - x.h.qstart;
    d.strand = al.strand ? 1 : 0;
    if (x.h.qend < x.h.qstart) return fail(HERRO_E_REFERENCE_PANIC, "window qend < qstart");
    if (d.strand == 0) d.qbeg = al.qstart + x.h.qstart;
    else {
      if (al.qend < x.h.qend) return fail(HERRO_E_REFERENCE_PANIC, "attempt to subtract with overflow (qend - window.qend)");
      d.qbeg = al.qend - x.h.qend;
    }
    d.op_begin = x.op_base + x.h.op_lo;
    d.op_cnt = x.h.op_hi - x.h.op_lo;
    d.start_off = x.h.start_off;
    d.end_off = x.h.end_off;
    d.scr_off = (uint32_t)out.scr_ops;
    d.wtstart = win_start;
    d.wlen = win_len;
    d.t_woff = ctx->h_word_off[rid];
    d.q_woff = ctx->h_word_off[al.qid];
    d.q_qual_off = ctx->h_qual_off[al.qid];
    // ---- validate what the reference would assert / index (features.rs:585-679, 110-237)
    if (x.h.op_hi <= x.h.op_lo) return fail(HERRO_E_REFERENCE_PANIC, "empty cigar slice");
    if (d.tstart < win_start) return fail(HERRO_E_REFERENCE_PANIC, "overlap starts before its window (usize underflow)");
    // a slice may start with an insertion (an alignment that begins inside the window with I ops): its bases go behind the position in
    // front of the overlap's first (features.rs:219-228) — unless there is none: max_ins[tpos - 1] with tpos == 0 panics (features.rs:77)
    if (op_type(x.h.op_first) == OP_I && d.tstart == win_start)
      return fail(HERRO_E_REFERENCE_PANIC, "insertion in front of the window's first position (max_ins[tpos - 1], attempt to subtract with overflow)");
    // target / query bases the TRIMMED slice consumes, from the prefix sums of the parse: the slice's first op loses
    // start_off bases, its last op counts end_off bases (effective-op-length rule, features.rs:82-90); the insertion
    // total stays untrimmed (get_max_ins, features.rs:64-79).  The slice never starts with I (checked per alignment).
    const uint32_t op_f = x.h.op_first, op_l = x.h.op_last;
    uint64_t tt = x.h.st, qq = x.h.sq;
    if (d.op_cnt == 1) {
      if (d.end_off <= d.start_off) return fail(HERRO_E_REFERENCE_PANIC, "cigar_end_offset <= cigar_start_offset");
      const uint32_t e1 = d.end_off - d.start_off, l1 = op_len(op_f);
      if (op_type(op_f) != OP_I) tt = tt - l1 + e1;
      if (op_type(op_f) != OP_D) qq = qq - l1 + e1;
    } else {
      if (op_len(op_f) <= d.start_off) return fail(HERRO_E_REFERENCE_PANIC, "op length <= cigar_start_offset");
      if (d.end_off == 0) return fail(HERRO_E_REFERENCE_PANIC, "Operation length cannot be 0");
      if (op_type(op_f) != OP_I) tt -= d.start_off;
      if (op_type(op_f) != OP_D) qq -= d.start_off;
      const uint32_t ll = op_len(op_l);
      if (op_type(op_l) != OP_I) tt = tt - ll + d.end_off;
      if (op_type(op_l) != OP_D) qq = qq - ll + d.end_off;
    }
    ins_sum[wi] += x.h.si;
    if ((uint64_t)(d.tstart - win_start) + tt > win_len) return fail(HERRO_E_REFERENCE_PANIC, "cigar slice overruns the target window");
    if (qq > d.qlen) return fail(HERRO_E_REFERENCE_PANIC, "cigar slice overruns the query region");
    if ((uint64_t)d.qbeg + d.qlen > ctx->read_len[al.qid]) return fail(HERRO_E_REFERENCE_PANIC, "query region exceeds the query read");
    out.scr_ops += d.op_cnt;
    out.alg_read_bytes += (uint64_t)d.qlen + (d.qlen + 3) / 4;
    out.alg_op_bytes += (uint64_t)d.op_cnt * 4;
    out.ow[fill[wi]++] = d;
  }
  for (uint32_t wi = 0; wi < n_windows; wi++) {
    WinDesc wd{};
    wd.rid = rid; wd.wid = wi; wd.n_wids = n_windows;
    wd.tstart = wi * W;
    wd.win_len = (wi == n_windows - 1) ? tlen - wi * W : W;
    wd.ow_begin = cnt[wi];
    wd.ow_cnt = cnt[wi + 1] - cnt[wi];
    const uint64_t lub = ((uint64_t)wd.win_len + std::min<uint64_t>(ins_sum[wi], (uint64_t)50 * wd.win_len) + 15) & ~15ull;
    wd.lub = (uint32_t)lub;
    out.alg_read_bytes += (uint64_t)wd.win_len + (wd.win_len + 3) / 4;
    out.win.push_back(wd);
  }
}
}  // namespace

// ---- host ranges registered for zero-copy job creation (herro_host_register) -----------------------------------------------------
// Process-wide: several contexts (feeder threads) create jobs from the same alignment buffer; a range is pinned once and counted.
namespace {
struct HostReg { const unsigned char* p; uint64_t n; int refs; const unsigned char* dp; };   // dp: the range as kernels see it (hipHostGetDevicePointer; null: not mapped)
std::mutex g_reg_mu;
std::vector<HostReg> g_regs;
std::atomic<uint64_t> g_zero_copy_jobs{0};   // jobs whose texts went up straight from a registered range (herro_debug_zero_copy_jobs)
// *dev (may be null): where kernels read the byte at `lo` directly, if the range is mapped AND 16-byte pieces read around [lo, hi) stay on its pinned pages
bool host_range_registered(const unsigned char* lo, const unsigned char* hi, const unsigned char** dev = nullptr) {
  std::lock_guard<std::mutex> lk(g_reg_mu);
  for (const HostReg& r : g_regs)
    if (lo >= r.p && hi <= r.p + r.n) {
      if (dev) {
        const uintptr_t page_lo = (uintptr_t)r.p & ~uintptr_t(4095), page_hi = ((uintptr_t)r.p + r.n + 4095) & ~uintptr_t(4095);
        const bool safe = ((uintptr_t)lo & ~uintptr_t(15)) >= page_lo && (((uintptr_t)hi + 31) & ~uintptr_t(15)) <= page_hi;
        *dev = (r.dp && safe) ? r.dp + (lo - r.p) : nullptr;
      }
      return true;
    }
  return false;
}
}  // namespace

int herro_host_register(herro_ctx* ctx, const void* p, uint64_t bytes) {
  if (!ctx || !p || !bytes) return HERRO_E_INVALID;
  if (ctx->host_only) return HERRO_OK;
  {
    std::lock_guard<std::mutex> lk(g_reg_mu);
    for (HostReg& r : g_regs) if (r.p == (const unsigned char*)p && r.n == bytes) { r.refs++; return HERRO_OK; }
  }
  // the pinning (a multi-GB blob takes a while) runs OUTSIDE the registry's lock: every feeder's herro_job_create looks ranges up under it
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const hipError_t e = hipHostRegister(const_cast<void*>(p), bytes, hipHostRegisterPortable | hipHostRegisterMapped);
  if (e != hipSuccess) {   // e.g. the memlock limit: not fatal — jobs over this range are staged like any unregistered text
    (void)hipGetLastError();
    ctx->err = std::string("herro_host_register: ") + hipGetErrorString(e) + " (jobs over this range will be staged)";
    return HERRO_E_UNSUPPORTED;
  }
  std::lock_guard<std::mutex> lk(g_reg_mu);
  for (HostReg& r : g_regs)
    if (r.p == (const unsigned char*)p && r.n == bytes) {   // somebody registered the same range meanwhile: one registration is enough
      r.refs++;
      (void)hipHostUnregister(const_cast<void*>(p));
      return HERRO_OK;
    }
  void* dp = nullptr;
  if (hipHostGetDevicePointer(&dp, const_cast<void*>(p), 0) != hipSuccess) { (void)hipGetLastError(); dp = nullptr; }
  g_regs.push_back(HostReg{(const unsigned char*)p, bytes, 1, (const unsigned char*)dp});
  return HERRO_OK;
}
uint64_t herro_debug_zero_copy_jobs(void) { return g_zero_copy_jobs.load(); }

// (ctx may be NULL: the registry is process-wide and the range outlives no particular context)
int herro_host_unregister(herro_ctx* ctx, const void* p) {
  if (!p) return HERRO_E_INVALID;
  if (ctx && ctx->host_only) return HERRO_OK;
  bool last = false;
  {
    std::lock_guard<std::mutex> lk(g_reg_mu);
    size_t i = 0;
    for (; i < g_regs.size(); i++) if (g_regs[i].p == (const unsigned char*)p) break;
    if (i == g_regs.size()) { if (ctx) ctx->err = "herro_host_unregister: not a registered range"; return HERRO_E_INVALID; }
    if (--g_regs[i].refs == 0) { g_regs.erase(g_regs.begin() + (long)i); last = true; }   // off the list first: no new job takes the zero-copy path over it
  }
  if (last) {
    // no copy out of the range may still be in flight — on ANY device: the registration is portable, contexts of other GPUs may be reading from it on their prep streams
    int n = 0, cur = 0;
    (void)hipGetDevice(&cur);
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    for (int d = 0; d < n; d++) if (hipSetDevice(d) == hipSuccess) (void)hipDeviceSynchronize();
    (void)hipSetDevice(cur);
    (void)hipHostUnregister(const_cast<void*>(p));
  }
  return HERRO_OK;
}

// ---- what herro_job_create settles on the host for the device build (round 6) because it needs no CIGAR: who is left out (parse_paf's rules), the ratio
// classes by read name, the windows of every target, the coordinate checks.  false: something this pass would have to report — the host build words it.
// Shared by herro_job_create and herro_job_create_aligned: the records are the same whether their ops arrive as text or from a device-resident handle.
namespace {
struct JobPrepass {
  std::vector<TgtMeta> tmeta;
  std::vector<AlnMeta> ameta;
  std::vector<uint64_t> cls;          // [n_targets + 1] prefix of the targets' ratio classes
  std::vector<uint32_t> skip;         // per target: alignments left out
  std::vector<std::string> first;     // ... and the message for its first
  uint32_t n_win = 0, n_cls = 0;
};

bool job_prepass(herro_ctx* ctx, HostPool& hpool, uint32_t n_targets, const uint32_t* rids, const uint64_t* aln_off, const herro_alignment* alns,
                 uint32_t W, std::vector<uint32_t>& tgt_win_off, JobPrepass& P) {
  const uint64_t a0 = n_targets ? aln_off[0] : 0, nA = n_targets ? aln_off[n_targets] - a0 : 0;
  std::vector<TgtMeta>& tmeta = P.tmeta;
  std::vector<AlnMeta>& ameta = P.ameta;
  tmeta.resize(n_targets);
  ameta.resize(nA);
  uint64_t nwin = 0, ncls = 0;
  for (uint32_t t = 0; t < n_targets; t++) {
    const uint32_t rid = rids[t];
    if (rid >= ctx->n_reads) return false;
    const uint32_t tlen = ctx->read_len[rid], nwt = (tlen + W - 1) / W;
    if (nwt > 65535) return false;
    tmeta[t] = TgtMeta{rid, tlen, nwt, (uint32_t)nwin, (uint32_t)(aln_off[t] - a0), (uint32_t)(aln_off[t + 1] - aln_off[t]), 0, 0};
    tgt_win_off[t] = (uint32_t)nwin;
    nwin += nwt;
  }
  if (nwin > 0xffffffffull || nwin == 0) return false;
  tgt_win_off[n_targets] = (uint32_t)nwin;
  P.cls.assign(n_targets + 1, 0);
  P.skip.assign(n_targets, 0);
  P.first.assign(n_targets, std::string());
  std::atomic<bool> ok{true};
  hpool.run(n_targets, [&](uint32_t t) {
    const TgtMeta& tm_ = tmeta[t];
    std::unordered_map<uint32_t, uint32_t> cls_of_name;
    std::unordered_map<uint32_t, uint32_t> seen_qid;
    uint32_t ncl = 0;
    for (uint32_t a = 0; a < tm_.n_aln; a++) {
      const herro_alignment& al = alns[a0 + tm_.aln0 + a];
      AlnMeta& m = ameta[tm_.aln0 + a];
      m = AlnMeta{al.qid, al.qstart, al.qend, al.tstart, al.tend, al.strand ? 1u : 0u, t, 0};
      if (al.tid != tm_.rid || al.qid >= ctx->n_reads) { ok = false; return; }
      const char* why = nullptr;
      if (al.qid == tm_.rid) why = "self overlap (dropped by parse_paf, overlaps.rs:175-179)";
      else if (seen_qid.count(al.qid)) why = "second alignment of the same (query,target) pair (dropped by parse_paf, overlaps.rs:181-185)";
      if (why) {
        m.flags |= 2u;
        if (!P.skip[t]++) P.first[t] = "target rid " + std::to_string(tm_.rid) + ", alignment " + std::to_string(a) + " (qid " + std::to_string(al.qid) + "): " + why;
        continue;
      }
      seen_qid[al.qid] = a;
      if (al.tlen != tm_.tlen || al.qend > ctx->read_len[al.qid] || al.tend > tm_.tlen) { ok = false; return; }
      const uint32_t nc = ctx->name_class[al.qid];
      auto it = cls_of_name.find(nc);
      if (it == cls_of_name.end()) it = cls_of_name.emplace(nc, ncl++).first;
      m.cls = it->second;   // target-local; the job-level base is added below
    }
    P.cls[t + 1] = ncl;
  });
  if (!ok) return false;
  for (uint32_t t = 0; t < n_targets; t++) P.cls[t + 1] += P.cls[t];
  ncls = P.cls[n_targets];
  if (ncls > 0xffffffffull) return false;
  hpool.run(n_targets, [&](uint32_t t) {
    const TgtMeta& tm_ = tmeta[t];
    for (uint32_t a = 0; a < tm_.n_aln; a++) ameta[tm_.aln0 + a].cls += (uint32_t)P.cls[t];
  });
  P.n_win = (uint32_t)nwin;
  P.n_cls = (uint32_t)ncls;
  return true;
}

// The ops of a job's alignments where they already lie on the device as `len << 2 | type` words (herro_job_create_aligned): alignment i of `alns` has
// n_ops[i] ops from word off[i] of d_store on.
struct OpsSrc { const uint32_t* d_store; const uint64_t* off; const uint32_t* n_ops; };
}  // namespace

// ---- job -------------------------------------------------------------------------------------------
// Job creation in stages ("Job creation as built"): argument checks; the scan plan (host only); staging into the pinned mirror of the scan
// block; the device pass (copies, scan, first phase of the device build, totals); the host build where the device did not settle the job; the job's
// pinned arena and the merge; the device arena and the descriptors' way into it.  Where the arrays lie inside the blocks is job_layout.h's.

// herro_job_create* return a pointer: the code of a failure travels through herro_job_create_status
static herro_job* create_fail(herro_ctx* ctx, int code, const std::string& m) {
  ctx->err = m + " [code " + std::to_string(code) + "]";
  ctx->create_code = code;
  return nullptr;
}

namespace {
using HostClock = std::chrono::steady_clock;
double ms_between(HostClock::time_point a, HostClock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }
struct CreateClock { HostClock::time_point begin, staged, scanned, built, merged; };   // HERRO_HOST_PROFILE: when each stage was over

struct CreateArgs {   // the arguments of herro_job_create*; src: see job_create_from
  herro_ctx* ctx; uint32_t n_targets; const uint32_t* rids; const uint64_t* aln_off; const herro_alignment* alns; uint32_t W; const OpsSrc* src;
  uint64_t a0, nA;    // the job's alignments are alns[a0, a0 + nA)
};

// a block of a free list for the length of a scope (the pinned staging block of one herro_job_create)
struct ArenaHold {
  herro_ctx* ctx; std::vector<Arena>* list; int kind; Arena a{};
  ~ArenaHold() { arena_release(ctx, *list, a, kind); }
};

// ---- stage 2: the scan plan.  One CigIn per alignment, the totals that size the scan block, and where the text comes from.  Host only.
struct ScanPlan {
  std::vector<CigIn> in;
  uint64_t txt = 0, opn = 0, cutn = 0;   // text bytes of the block, op slots, cut slots
  // Zero-copy (round 5): when the texts lie densely inside a range the caller registered (herro_host_register: the PAF text of
  // herro_paf_parse_view, a CIGAR blob), that range goes up in ONE copy from where it is — no staging pass over the bytes (0.9 of the
  // 3.4 ms an unloaded herro_job_create of 4096 windows took, and the part that fights the other feeders for memory bandwidth).  A
  // text keeps its alignment modulo 16: the scan kernel reads aligned 16-byte pieces and skips the bytes in front of the text.
  const unsigned char* t_lo = nullptr;   // the range of the caller's memory that holds the job's texts: [t_lo, t_lo + span)
  uint64_t span = 0, lead = 0;           // lead: t_lo modulo 16
  bool direct = false;                   // the range goes up as it is
  bool read_host = false;                // ... or not at all: the scan kernel reads it at t_dev over PCIe
  const unsigned char* t_dev = nullptr;
};

// (the totals run in locals: one pass over some 10^5 alignments per job on the feeder's own thread, where sums kept in S would go through memory every step)
bool plan_scan(const CreateArgs& A, ScanPlan& S) {
  herro_ctx* ctx = A.ctx;
  if (!A.alns) return create_fail(ctx, HERRO_E_INVALID, "null argument"), false;
  if (A.nA > 0x7fffffffull) return create_fail(ctx, HERRO_E_UNSUPPORTED, "job too large (alignments)"), false;
  const herro_alignment* alns = A.alns + A.a0;
  const uint64_t nA = A.nA;
  const uint32_t W = A.W;
  const OpsSrc* src = A.src;
  S.in.resize(nA);
  CigIn* in = S.in.data();
  uint64_t txt = 0, opn = 0, cutn = 0, txt_sum = 0;
  const unsigned char *t_lo = nullptr, *t_hi = nullptr;
  for (uint64_t g = 0; g < nA; g++) {
    const herro_alignment& al = alns[g];
    const uint32_t cap = (al.tend >= al.tstart ? (al.tend - al.tstart) / W : 0u) + 3u;   // one cut per window boundary the coordinates span, + slack
    if (src) {   // binary ops on the device (k_ops_scan): the slice's first word and its op count; the job's op array has room for exactly that many
      in[g] = CigIn{src->off[A.a0 + g], src->n_ops[A.a0 + g], al.tstart, (uint32_t)opn, (uint32_t)cutn, cap, 0};
      opn += src->n_ops[A.a0 + g];
      cutn += cap;
      continue;
    }
    if (al.cigar_len && !al.cigar) return create_fail(ctx, HERRO_E_INVALID, "alignment without cigar"), false;
    in[g] = CigIn{txt, al.cigar_len, al.tstart, (uint32_t)opn, (uint32_t)cutn, cap, 0};
    txt += ((uint64_t)al.cigar_len + 15) & ~uint64_t(15);
    opn += (uint64_t)al.cigar_len / 2 + 1;
    cutn += cap;
    if (al.cigar_len) {
      txt_sum += al.cigar_len;
      if (!t_lo || al.cigar < t_lo) t_lo = al.cigar;
      if (!t_hi || al.cigar + al.cigar_len > t_hi) t_hi = al.cigar + al.cigar_len;
    }
  }
  S.txt = txt; S.opn = opn; S.cutn = cutn; S.t_lo = t_lo;
  if (opn > 0xffffffffull || cutn > 0xffffffffull) return create_fail(ctx, HERRO_E_UNSUPPORTED, "job too large (ops exceed 2^32)"), false;
  // HERRO_ZERO_COPY: 0 stage every text; 1 (default) copy a registered range up as it is; 2 (round 6, measured in profiles/r6_e2e_ab.txt) no copy at all — the scan kernel
  // reads the registered range over PCIe where the caller has it (no blit kernel, no 50 MB through HBM and back per 4096 windows)
  static const int zc_mode = [] { const char* e = getenv("HERRO_ZERO_COPY"); return e ? atoi(e) : 1; }();
  const uint64_t span = t_lo ? (uint64_t)(t_hi - t_lo) : 0;
  S.span = span;
  S.direct = zc_mode != 0 && t_lo && span <= txt_sum + txt_sum / 2 + 65536 && host_range_registered(t_lo, t_hi, &S.t_dev);
  S.read_host = S.direct && zc_mode == 2 && S.t_dev != nullptr;
  if (!S.direct) return true;
  const uint64_t lead = (uintptr_t)t_lo & 15u;
  for (uint64_t g = 0; g < nA; g++) {
    const herro_alignment& al = alns[g];
    const uint64_t off = al.cigar_len ? lead + (uint64_t)(al.cigar - t_lo) : 0;
    in[g].txt_off = off & ~uint64_t(15);
    in[g].skip = (uint32_t)(off & 15u);
  }
  S.lead = lead;
  S.txt = (lead + span + 31) & ~uint64_t(15);
  g_zero_copy_jobs++;
  return true;
}

// ---- stage 3: staging.  The texts (unless they go up from where they are, or there are none), the records, and for the device build what the pre-pass
// settled, into the pinned mirror `hs` of the scan block.
void stage_scan(const CreateArgs& A, const ScanPlan& S, const JobPrepass& P, const ScanLayout& L, const ScanView& hs, HostPool& hpool) {
  const uint32_t per = 32, nblk = (uint32_t)((A.nA + per - 1) / per);
  if (!S.direct && !A.src) hpool.run(nblk, [&](uint32_t b) {
    for (uint64_t g = (uint64_t)b * per; g < std::min<uint64_t>(A.nA, (uint64_t)(b + 1) * per); g++) {
      const herro_alignment& al = A.alns[A.a0 + g];
      unsigned char* d = hs.text + S.in[g].txt_off;
      if (al.cigar_len) std::memcpy(d, al.cigar, al.cigar_len);
      std::memset(d + al.cigar_len, 0, (size_t)((((uint64_t)al.cigar_len + 15) & ~uint64_t(15)) - al.cigar_len));
    }
  });
  std::memcpy(hs.in, S.in.data(), A.nA * sizeof(CigIn));
  if (!L.try_dev) return;
  std::memcpy(hs.am, P.ameta.data(), A.nA * sizeof(AlnMeta));
  std::memcpy(hs.tm, P.tmeta.data(), (size_t)A.n_targets * sizeof(TgtMeta));
  hpool.run(A.n_targets, [&](uint32_t t) { for (uint32_t w = 0; w < P.tmeta[t].n_windows; w++) hs.win_tgt[P.tmeta[t].win0 + w] = t; });
  std::memset(hs.tot, 0, sizeof(BuildTotals));
}

// ---- stage 4: the device pass, on the context's prep stream.  The staged part goes up, the scan kernel writes the job's op array and the cut records; with
// the device build behind it (L.try_dev) the first build phase follows and 64 bytes of totals come down instead of the records.
//   BUILT        the device settled the job: *btot holds its totals, BD is bound for the second phase
//   HOST_BUILDS  the scan's records are in `hs`: the host cuts the windows from them (and words whatever is wrong with the input)
//   UNSETTLED    (ops from the device only) the text path rebuilds the job; the stream is idle: the totals' event has been waited for
//   FAILED       reported
// HERRO_HOST_PROFILE: copy up / kernels / copy down on the device clock, here and nowhere else.
enum class DevPass { BUILT, HOST_BUILDS, UNSETTLED, FAILED };

DevPass device_pass(const CreateArgs& A, const ScanPlan& S, const ScanLayout& L, const ScanView& hs, const ScanView& dv, uint32_t n_win, BuildDev& BD,
                    BuildTotals& btot, bool prof, const CreateClock& clk) {
  herro_ctx* ctx = A.ctx;
  const hipStream_t st = ctx->prep_stream;
  const uint64_t up_bytes = L.at(SP_OUT) - L.at(SP_IN), down_bytes = L.at(SP_TOTALS) - L.at(SP_OUT);   // [CigIn .. window -> target], [CigOut][cuts]
  hipEvent_t pe[4] = {nullptr, nullptr, nullptr, nullptr};
  if (prof) for (auto& ev : pe) (void)hipEventCreate(&ev);
  auto drop_events = [&] { for (auto& ev : pe) if (ev) (void)hipEventDestroy(ev); };
  if (pe[0]) (void)hipEventRecord(pe[0], st);
  hipError_t e;
  if (S.direct) {   // the texts from the caller's registered range (same alignment modulo 16), the alignment records from the staging block
    e = S.read_host ? hipSuccess : hipMemcpyAsync(dv.text + S.lead, S.t_lo, S.span, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(dv.in, hs.in, up_bytes, hipMemcpyHostToDevice, st);
  } else if (A.src) {   // no text: the alignment records alone
    e = hipMemcpyAsync(dv.in, hs.in, up_bytes, hipMemcpyHostToDevice, st);
  } else {
    e = hipMemcpyAsync(dv.text, hs.text, L.at(SP_OUT), hipMemcpyHostToDevice, st);
  }
  if (L.try_dev && e == hipSuccess) e = hipMemcpyAsync(dv.tot, hs.tot, sizeof(BuildTotals), hipMemcpyHostToDevice, st);
  if (pe[1]) (void)hipEventRecord(pe[1], st);
  if (e == hipSuccess && A.src) {
    launch_ops_scan(A.src->d_store, dv.in, dv.out, dv.cuts, dv.ops, &dv.tot->err, BLD_SCAN_FLAG, (uint32_t)A.nA, A.W, st);
    e = hipGetLastError();
  } else if (e == hipSuccess) {
    launch_cigar_scan(S.read_host ? S.t_dev - S.lead : dv.text, dv.in, dv.out, dv.cuts, dv.ops, (uint32_t)A.nA, A.W, st);
    e = hipGetLastError();
  }
  if (pe[2]) (void)hipEventRecord(pe[2], st);
  bool dev_built = false;
  if (L.try_dev && e == hipSuccess) {   // windows and counts behind the scan
    bind_build_scan(BD, dv);
    BD.n_aln = (uint32_t)A.nA; BD.n_tgt = A.n_targets; BD.n_win = n_win; BD.W = A.W;
    BD.read_word_off = ctx->d_word_off; BD.read_qual_off = ctx->d_qual_off;
    launch_build_phase1(BD, dv.ow_begin, dv.ev_off, dv.tile_off, dv.row_off, st);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(hs.tot, dv.tot, sizeof(BuildTotals), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipEventRecord(ctx->prep_ev, st);
    if (e == hipSuccess) e = hipEventSynchronize(ctx->prep_ev);
    if (e == hipSuccess) {
      std::memcpy(&btot, hs.tot, sizeof btot);
      dev_built = btot.err == 0;
    }
  }
  if (A.src && e == hipSuccess && !dev_built) { drop_events(); return DevPass::UNSETTLED; }
  if (!dev_built) {
    if (e == hipSuccess) e = hipMemcpyAsync(hs.out, dv.out, down_bytes, hipMemcpyDeviceToHost, st);
    if (pe[3]) (void)hipEventRecord(pe[3], st);
    if (e == hipSuccess) e = hipEventRecord(ctx->prep_ev, st);
    if (e == hipSuccess) e = hipEventSynchronize(ctx->prep_ev);
  } else if (pe[3]) (void)hipEventRecord(pe[3], st);
  if (prof && e == hipSuccess) {
    float up = 0, kn = 0, dn = 0;
    (void)hipEventElapsedTime(&up, pe[0], pe[1]); (void)hipEventElapsedTime(&kn, pe[1], pe[2]); (void)hipEventElapsedTime(&dn, pe[2], pe[3]);
    fprintf(stderr, "  cigar scan: %.1f MiB text staged in %.2f ms; device: copy up %.2f ms, kernel %.2f, copy down %.2f (%.1f MiB); wall %.2f ms\n", S.txt / 1048576.0,
            ms_between(clk.begin, clk.staged), up, kn, dn, (dev_built ? 64.0 : (double)down_bytes) / 1048576.0, ms_between(clk.staged, HostClock::now()));
  }
  drop_events();
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(st);
    create_fail(ctx, HERRO_E_NO_DEVICE, std::string("CIGAR scan failed: ") + hipGetErrorString(e));
    return DevPass::FAILED;
  }
  return dev_built ? DevPass::BUILT : DevPass::HOST_BUILDS;
}

// what the device build settled besides its totals (job_totals): the algorithmic bytes; the pre-pass knows who was left out
void adopt_device_build(herro_job* job, const BuildTotals& btot, const JobPrepass& P) {
  job->alg_read_bytes = btot.rd_bytes; job->alg_op_bytes = btot.op_bytes;
  for (size_t t = 0; t < P.skip.size(); t++)
    if (P.skip[t]) {
      if (!job->n_skipped_alns) job->first_skip = P.first[t];
      job->n_skipped_alns += P.skip[t];
    }
}

// ---- stage 5: the host build.  Per-target host work (CIGAR parse or the scan's records in `ds`, windowing, validation) is independent: it runs on the
// context's thread pool, each target into its own buffers with target-local offsets.  A serial pass over the per-target SIZES then fixes every base
// offset: base[t] is what the targets in front of t hold, base[n_targets] the job.
bool host_build(const CreateArgs& A, const DevScanView* ds, HostPool& hpool, herro_job* job, std::vector<TargetOut>& outs, std::vector<JobTotals>& base,
                CreateClock& clk) {
  herro_ctx* ctx = A.ctx;
  outs.resize(A.n_targets);
  hpool.run(A.n_targets, [&](uint32_t t) {
    build_target(ctx, A.rids[t], A.alns + A.aln_off[t], (uint32_t)(A.aln_off[t + 1] - A.aln_off[t]), A.W, outs[t], ds, A.aln_off[t] - A.a0);
  });
  clk.built = HostClock::now();
  base.resize(A.n_targets + 1);
  JobTotals b;
  for (uint32_t t = 0; t < A.n_targets; t++) {
    const TargetOut& o = outs[t];
    if (o.err.code != HERRO_OK) return create_fail(ctx, o.err.code, "target " + std::to_string(t) + " (rid " + std::to_string(A.rids[t]) + "): " + o.err.msg), false;
    if (o.n_skipped) {
      if (!job->n_skipped_alns && !job->n_failed_targets) job->first_skip = o.first_skip;
      job->n_skipped_alns += o.n_skipped;
      job->n_failed_targets += o.failed ? 1u : 0u;
    }
    for (auto& pt : o.op_patches) {   // rare; synchronous
      if (hipMemcpy((uint32_t*)job->scan.p + pt.first, pt.second.data(), pt.second.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
        return create_fail(ctx, HERRO_E_NO_DEVICE, "op upload failed"), false;
    }
    base[t] = b;
    b.op += o.ops.size(); b.ow += o.ow.size(); b.win += o.win.size(); b.cls += o.n_cls; b.scr += o.scr_ops;
    for (const WinDesc& wd : o.win) {
      b.tile += (wd.lub + HERRO_TILE - 1) / HERRO_TILE;
      b.fin += (uint64_t)HERRO_ROWS * wd.lub; b.row += wd.lub; b.pos += (uint64_t)A.W + 1;
      b.max_cols = std::max(b.max_cols, wd.ow_cnt + 1);
    }
    if (b.op > 0xffffffffull) return create_fail(ctx, HERRO_E_UNSUPPORTED, "job too large (ops exceed 2^32)"), false;
    job->alg_read_bytes += o.alg_read_bytes;
    job->alg_op_bytes += o.alg_op_bytes;
    job->tgt_win_off[t + 1] = (uint32_t)b.win;
  }
  base[A.n_targets] = b;
  return true;
}

// ---- stage 6: the job's pinned arena — the descriptor head, then the landing zones of the counts and of the corrected bases
bool bind_job_pin(herro_ctx* ctx, herro_job* job, const JobLayout& L, const JobTotals& tot) {
  job->pin = arena_acquire(ctx, ctx->free_pin, L.pin_bytes, 0);
  if (!job->pin.p) return create_fail(ctx, HERRO_E_NO_DEVICE, "out of pinned host memory for the job"), false;
  const JobHead H = bind_head(job->pin.p, L);
  job->ops.p = H.ops; job->ops.n = tot.op;
  job->ow.p = H.ow; job->ow.n = tot.ow;
  job->win.p = H.win; job->win.n = tot.win;
  job->tile_win.p = H.tile_win; job->tile_win.n = tot.tile;
  job->tile_r0.p = H.tile_r0; job->tile_r0.n = tot.tile;
  const JobPinTail T = bind_pin_tail(job->pin.p, L);
  job->h_counts = T.counts; job->h_cons_len = T.cons_len; job->h_cons_seq = T.cons_seq;
  return true;
}

// ... and the merge in target order (host build): the bytes are copied, and the target-local indices rebased, by the pool, straight into the head of the
// pinned arena
void merge_targets(herro_job* job, std::vector<TargetOut>& outs, const std::vector<JobTotals>& base, uint32_t W, HostPool& hpool) {
  hpool.run((uint32_t)outs.size(), [&](uint32_t t) {
    TargetOut& o = outs[t];
    const JobTotals& b = base[t];
    if (!o.ops.empty()) std::memcpy(job->ops.data() + b.op, o.ops.data(), o.ops.size() * 4);
    for (size_t i = 0; i < o.ow.size(); i++) {
      OwDesc d = o.ow[i];
      d.win += (uint32_t)b.win; d.cls += (uint32_t)b.cls; d.op_begin += (uint32_t)b.op; d.scr_off += (uint32_t)b.scr;
      job->ow[b.ow + i] = d;
    }
    uint64_t fin = b.fin, row = b.row, pos = b.pos, tile = b.tile, evo = b.scr + 2 * b.ow;
    for (size_t i = 0; i < o.win.size(); i++) {
      WinDesc wd = o.win[i];
      wd.ev_off = evo;
      for (uint32_t k = 0; k < wd.ow_cnt; k++) evo += o.ow[wd.ow_begin + k].op_cnt + 2u;   // target-local ow_begin here
      wd.ow_begin += (uint32_t)b.ow;
      wd.col_off = tile;   // first tile of the window
      wd.fin_off = fin; fin += (uint64_t)HERRO_ROWS * wd.lub;
      wd.row_off = row; row += wd.lub;
      wd.pos_off = pos; pos += (uint64_t)W + 1;
      for (uint32_t r0 = 0; r0 < wd.lub; r0 += HERRO_TILE) { job->tile_win[tile] = (uint32_t)(b.win + i); job->tile_r0[tile] = r0; tile++; }
      job->win[b.win + i] = wd;
    }
    o = TargetOut();  // release
  });
}

// ---- stage 7: the device arena and the descriptors' way into it.  ops_in_scan: the ops lie in the job's scan arena (the device scanned them).
// BD: bound by the device pass when it built the job (null: the host did).
bool job_to_device(herro_ctx* ctx, herro_job* job, const JobLayout& L, const JobTotals& tot, bool ops_in_scan, BuildDev* BD) {
  JobDev& J = job->J;
  J.read_words = ctx->d_words; J.read_word_off = ctx->d_word_off; J.read_p0 = ctx->d_p0; J.read_p1 = ctx->d_p1;
  J.read_qual = ctx->d_qual; J.read_qual_off = ctx->d_qual_off; J.read_qual_bytes = ctx->qual_bytes; J.read_n_words = ctx->n_words;
  J.ln_table = ctx->d_ln; J.ln_table_n = ctx->ln_n;
  J.prof = ctx->d_prof;
  J.n_ow = (uint32_t)tot.ow; J.n_win = (uint32_t)tot.win; J.n_cls = (uint32_t)tot.cls;
  J.n_tiles = (uint32_t)tot.tile; J.window_size = job->W; J.nw = (job->W + 31) / 32; J.max_cols = tot.max_cols;
  { const char* e = getenv("HERRO_DEBUG_CDIR_OVERFLOW"); J.dbg_flags = (e && atoi(e)) ? 1u : 0u; }
  job->dev = arena_acquire(ctx, ctx->free_dev, L.dev_bytes, 1);
  if (!job->dev.p) return create_fail(ctx, HERRO_E_NO_DEVICE, "out of device memory for the job (" + std::to_string(L.dev_bytes >> 20) + " MiB)"), false;
  bind_job_dev(J, job->dev.p, L, tot.win);
  if (ops_in_scan) J.ops = (const uint32_t*)job->scan.p;
  job->d_counts = J.win_Lf;
  J.rf = nullptr; J.rf_cap = 0; J.rf_half = 0;
  hipError_t e;
  if (BD) {
    // the descriptors are written where they are read (build_dev.hip, behind the scan on the prep stream); the window descriptors come down — the host hands
    // windows out by them — and the context's stream waits for the event, so the kernels of herro_job_featurize queue behind the build in stream order
    bind_build_head(*BD, bind_head(job->dev.p, L));
    launch_build_phase2(*BD, ctx->prep_stream);
    e = hipGetLastError();
    if (e == hipSuccess && J.n_win) e = hipMemcpyAsync(job->win.data(), BD->win, (size_t)J.n_win * sizeof(WinDesc), hipMemcpyDeviceToHost, ctx->prep_stream);
    if (e == hipSuccess) e = hipEventRecord(ctx->prep_ev, ctx->prep_stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream, ctx->prep_ev, 0);
    if (e == hipSuccess) e = hipEventSynchronize(ctx->prep_ev);
    job->dev_built = true;
  } else {
    // one copy, pinned -> device, asynchronous on the context stream: the head has the same layout in both arenas.  The kernels of herro_job_featurize
    // queue behind it in stream order, nobody waits here
    e = hipMemcpyAsync(job->dev.p, job->pin.p, L.desc_bytes, hipMemcpyHostToDevice, ctx->stream);
  }
  if (e == hipSuccess) e = hipEventCreateWithFlags(&job->ev_counts, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&job->ev_blob, hipEventDisableTiming);
  if (e == hipSuccess) return true;
  (void)hipStreamSynchronize(ctx->stream);
  return create_fail(ctx, HERRO_E_NO_DEVICE, std::string("descriptor upload failed: ") + hipGetErrorString(e)), false;
}
}  // namespace

// herro_job_create (src == nullptr: the ops come as CIGAR text) and the direct path of herro_job_create_aligned (src: they are on the device; the caller
// has checked that the context builds on the device).  *unsettled is raised, with nothing reported, when the direct path does not settle the job: the
// caller then goes through the text of the job's ops.  A job that is let go of half way returns what it holds (~herro_job).
static herro_job* job_create_from(herro_ctx* ctx, uint32_t n_targets, const uint32_t* rids, const uint64_t* aln_off,
                                  const herro_alignment* alns, uint32_t W, const OpsSrc* src, bool* unsettled) {
  if (!ctx) return nullptr;
  ctx->create_code = HERRO_OK;
  if (!ctx->d_words && !ctx->host_only) return create_fail(ctx, HERRO_E_STATE, "herro_set_reads must be called first");
  if (W < 16 || W > HERRO_MAX_WINDOW) return create_fail(ctx, HERRO_E_UNSUPPORTED, "window_size must be in [16, 8192]");
  if (n_targets && (!rids || !aln_off)) return create_fail(ctx, HERRO_E_INVALID, "null argument");
  if (!ctx->host_only && hipSetDevice(ctx->device) != hipSuccess) return create_fail(ctx, HERRO_E_NO_DEVICE, "hipSetDevice failed");
  const uint64_t a0 = n_targets ? aln_off[0] : 0;
  const CreateArgs A{ctx, n_targets, rids, aln_off, alns, W, src, a0, n_targets ? aln_off[n_targets] - a0 : 0};

  const bool prof = getenv("HERRO_HOST_PROFILE") != nullptr;
  ProfSpan span_(ctx, "create");
  CreateClock clk;
  clk.begin = clk.scanned = HostClock::now();
  auto job = std::make_unique<herro_job>();
  job->ctx = ctx;
  job->W = W;
  job->n_targets = n_targets;
  job->tgt_win_off.assign(n_targets + 1, 0);
  HostPool& hpool = host_pool(ctx);

  // ---- the CIGAR text goes to the GPU first (cigar_dev.hip): one kernel (a workgroup per alignment) writes the binary ops into the job's op array and
  // returns, per alignment, the totals and the ops that reach a window boundary.  Device build (round 6): what needs no CIGAR is settled by the pre-pass
  // and goes up beside the text; anything it would have to report sends the job down the host path, which words it.
  ArenaHold stage{ctx, &ctx->free_stage, 0};
  JobPrepass P;
  BuildDev BD{};
  BuildTotals btot{};
  DevScanView dsv{nullptr, nullptr, nullptr};
  bool scanned = false, dev_built = false;
  if (!ctx->host_only && ctx->dev_scan && A.nA) {
    ScanPlan S;
    if (!plan_scan(A, S)) return nullptr;
    const bool try_dev = ctx->dev_build && job_prepass(ctx, hpool, n_targets, rids, aln_off, alns, W, job->tgt_win_off, P);
    if (src && !try_dev) { *unsettled = true; return nullptr; }
    const ScanLayout SL = scan_layout(A.nA, n_targets, P.n_win, S.txt, S.cutn, S.opn, try_dev);
    stage.a = arena_acquire(ctx, ctx->free_stage, SL.blk_bytes, 0);
    job->scan = arena_acquire(ctx, ctx->free_scan, SL.ops_bytes + SL.dev_blk_bytes, 1);
    if (!stage.a.p || !job->scan.p)
      return create_fail(ctx, HERRO_E_NO_DEVICE, "out of memory for the CIGAR scan (" + std::to_string((SL.ops_bytes + SL.dev_blk_bytes) >> 20) + " MiB)");
    const ScanView hs = bind_scan_host(stage.a.p, SL), dv = bind_scan_dev(job->scan.p, SL);
    stage_scan(A, S, P, SL, hs, hpool);
    clk.staged = HostClock::now();
    switch (device_pass(A, S, SL, hs, dv, P.n_win, BD, btot, prof, clk)) {
      case DevPass::FAILED: return nullptr;
      case DevPass::UNSETTLED: *unsettled = true; return nullptr;
      case DevPass::BUILT: dev_built = true; break;
      case DevPass::HOST_BUILDS: break;
    }
    dsv = DevScanView{hs.in, hs.out, hs.cuts};
    scanned = true;
    job->scan_ops = S.opn;
    clk.scanned = HostClock::now();
  }
  std::vector<TargetOut> outs;
  std::vector<JobTotals> base;   // host build: per target, what lies in front of it
  JobTotals tot;
  if (dev_built) {
    clk.built = HostClock::now();
    adopt_device_build(job.get(), btot, P);
    tot = job_totals(btot, P.n_win, P.n_cls, W);
  } else {
    if (!host_build(A, scanned ? &dsv : nullptr, hpool, job.get(), outs, base, clk)) return nullptr;
    tot = base[n_targets];
  }
  // the windows' event slices live behind scr_ops + 2 * n_ow slots and are indexed with 32 bits on the device (WinDesc::ev_off -> CTab::ev_off)
  if (tot.scr + 2ull * tot.ow > 0xffffffffull) return create_fail(ctx, HERRO_E_UNSUPPORTED, "job too large (op scratch exceeds 2^32)");
  // (what was left out is reported by herro_job_skipped; the error slot is for errors only)
  const JobLayout L = job_layout(tot, W);
  if (!bind_job_pin(ctx, job.get(), L, tot)) return nullptr;
  if (!dev_built) merge_targets(job.get(), outs, base, W, hpool);
  job->row_elems = tot.row;
  job->reads_gen = ctx->reads_gen;
  clk.merged = HostClock::now();
  if (ctx->host_only) {  // test hook: the host half (descriptors) only
    if (prof) fprintf(stderr, "herro_job_create (host half): build %.2f ms, merge %.2f (%zu windows)\n", ms_between(clk.begin, clk.built), ms_between(clk.built, clk.merged), job->win.size());
  } else {
    if (!job_to_device(ctx, job.get(), L, tot, scanned, dev_built ? &BD : nullptr)) return nullptr;
    if (prof)
      fprintf(stderr, "herro_job_create: scan %.2f ms, build %.2f, merge %.2f, arena + enqueue %.2f (%u windows, %zu MiB device)\n", ms_between(clk.begin, clk.scanned),
              ms_between(clk.scanned, clk.built), ms_between(clk.built, clk.merged), ms_between(clk.merged, HostClock::now()), job->J.n_win, (size_t)(L.dev_bytes >> 20));
  }
  ctx->live_jobs++;
  return job.release();
}

herro_job* herro_job_create(herro_ctx* ctx, uint32_t n_targets, const uint32_t* rids, const uint64_t* aln_off,
                            const herro_alignment* alns, uint32_t W) {
  return job_create_from(ctx, n_targets, rids, aln_off, alns, W, nullptr, nullptr);
}

int herro_job_create_status(const herro_ctx* ctx) { return ctx ? ctx->create_code.load() : HERRO_E_INVALID; }

int herro_job_skipped(const herro_job* job, uint32_t* n_alignments, uint32_t* n_targets) {
  if (!job) return HERRO_E_INVALID;
  if (n_alignments) *n_alignments = job->n_skipped_alns;
  if (n_targets) *n_targets = job->n_failed_targets;
  return HERRO_OK;
}

void herro_job_free(herro_job* job) {
  if (!job) return;
  herro_ctx* ctx = job->ctx;
  if (ctx->live_jobs.load()) ctx->live_jobs--;
  if (job->pending) { job->pending = false; ctx->n_pending--; }   // featurized, never inferred
  ctx->sib_suspects.erase(std::remove(ctx->sib_suspects.begin(), ctx->sib_suspects.end(), job), ctx->sib_suspects.end());
  if (ctx->host_only) { delete job; return; }
  ProfSpan span_(ctx, "destroy");
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);   // nothing of this job is in flight once its memory is recycled
  delete job;
}

uint32_t herro_job_n_windows(const herro_job* job) { return job ? (uint32_t)job->win.size() : 0; }

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

}  // extern "C"

static int job_sync(herro_job* job) {
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

// The arrays of one launch inside the descriptor image at d_image (build_launch); the caller adds the buffers the launch reads and writes.
static BatchDev batch_dev(const void* d_image, const LaunchOffs& o) {
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
static LaunchCfg launch_cfg(const herro_ctx* ctx, uint32_t fused_rows, bool with_rf_base) {
  return LaunchCfg{ctx->precision == 1 || ctx->precision >= 4, fused_rows, ctx->tile_packing, ctx->precision >= 4 ? model_h_half_tiles(ctx->M) : 0, ctx->n_cu, with_rf_base};
}

extern "C" {

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

int herro_job_window_info(herro_job* job, uint32_t w, herro_window_info* info) {
  if (!job || !info || w >= job->win.size()) return HERRO_E_INVALID;
  int rc = job_sync(job);
  if (rc) return rc;
  const WinDesc& wd = job->win[w];
  info->rid = wd.rid; info->wid = wd.wid; info->n_total_wins = wd.n_wids;
  info->length = job->h_Lf[w];
  info->n_overlaps = job->h_nkept[w];
  info->n_alns = std::min<uint32_t>(job->h_nkept[w], 30);
  info->n_supported = job->h_nsup[w];
  info->win_len = wd.win_len;
  return HERRO_OK;
}

static int fetch_planes(herro_job* job, uint32_t w, std::vector<uint8_t>& pb, std::vector<uint8_t>* pq) {
  herro_ctx* ctx = job->ctx;
  const WinDesc& wd = job->win[w];
  const size_t bytes = (size_t)HERRO_ROWS * wd.lub;
  pb.resize(bytes);
  if (!job->tokens_full) {  // a lean featurize pass wrote no planes: build them (and the row map the quality planes need) for whoever asks
    launch_full_tokens(job->J, ctx->stream, nullptr);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    job->tokens_full = true;
  }
  HIP_TRY(ctx, hipMemcpy(pb.data(), job->J.fin_b + wd.fin_off, bytes, hipMemcpyDeviceToHost));
  if (pq) {
    if (!job->quals_full) {  // featurize leaves the quality planes to whoever asks for them
      launch_full_quals(job->J, ctx->stream);
      HIP_TRY(ctx, hipGetLastError());
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      job->quals_full = true;
    }
    pq->resize(bytes);
    HIP_TRY(ctx, hipMemcpy(pq->data(), job->J.fin_q + wd.fin_off, bytes, hipMemcpyDeviceToHost));
  }
  return HERRO_OK;
}

int herro_job_window_copy(herro_job* job, uint32_t w, int encoded, uint8_t* bases, uint8_t* quals,
                          uint16_t* sup_pos, uint8_t* sup_ins, uint32_t* qids) {
  if (!job || w >= job->win.size()) return HERRO_E_INVALID;
  int rc = job_sync(job);
  if (rc) return rc;
  herro_ctx* ctx = job->ctx;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const WinDesc& wd = job->win[w];
  const uint32_t L = job->h_Lf[w];
  if (bases || quals) {
    std::vector<uint8_t> pb, pq;
    rc = fetch_planes(job, w, pb, quals ? &pq : nullptr);
    if (rc) return rc;
    for (uint32_t r = 0; r < L; r++)
      for (uint32_t c = 0; c < HERRO_ROWS; c++) {
        if (bases) {
          const uint8_t t = pb[(size_t)c * wd.lub + r];
          bases[(size_t)r * HERRO_ROWS + c] = encoded ? t : (uint8_t)TOK_ASCII[t < 12 ? t : 12 - 1];
        }
        if (quals) quals[(size_t)r * HERRO_ROWS + c] = pq[(size_t)c * wd.lub + r];
      }
  }
  const uint32_t ns = job->h_nsup[w];
  if ((sup_pos || sup_ins) && ns) {
    std::vector<uint32_t> pi(ns);
    HIP_TRY(ctx, hipMemcpy(pi.data(), job->J.sup_pi + wd.row_off, ns * 4ull, hipMemcpyDeviceToHost));
    for (uint32_t k = 0; k < ns; k++) {
      if (sup_pos) sup_pos[k] = (uint16_t)(pi[k] & 0xffffu);
      if (sup_ins) sup_ins[k] = (uint8_t)(pi[k] >> 16);
    }
  }
  if (qids && job->h_nkept[w])
    HIP_TRY(ctx, hipMemcpy(qids, job->J.rank_qid + wd.ow_begin, job->h_nkept[w] * 4ull, hipMemcpyDeviceToHost));
  return HERRO_OK;
}

// A sibling tile that never saw its group (check_sib) is not the caller's problem: the model pass of every job the raised word may belong to — and its consensus
// pass, if that had run — is repeated ONCE with its windows above 64 informative rows on the layer-by-layer kernels, which have no cross-workgroup wait,
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
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->timer.collect();
  return check_sib(ctx, job);
}

static int logits_to_host(herro_job* job) {
  herro_ctx* ctx = job->ctx;
  if (!job->inferred) { ctx->err = "herro_job_infer has not run"; return HERRO_E_STATE; }
  if (job->logits_on_host) return HERRO_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const uint64_t tot = job->sup_off.back();
  job->h_info.resize(tot);
  job->h_base.resize(tot * 5);
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->timer.collect();
  if (int rc = check_sib(ctx, job)) if ((rc = sib_retry(job, rc))) return rc;
  if (tot) {
    HIP_TRY(ctx, hipMemcpy(job->h_info.data(), job->d_info, tot * 4, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(job->h_base.data(), job->d_base, tot * 20, hipMemcpyDeviceToHost));
  }
  job->logits_on_host = true;
  return HERRO_OK;
}

int herro_job_window_logits(herro_job* job, uint32_t w, float* info_logits, float* bases_logits) {
  if (!job || w >= job->win.size()) return HERRO_E_INVALID;
  int rc = logits_to_host(job);
  if (rc) return rc;
  const uint64_t o = job->sup_off[w], n = job->h_nsup[w];
  if (info_logits) std::memcpy(info_logits, job->h_info.data() + o, n * 4);
  if (bases_logits) std::memcpy(bases_logits, job->h_base.data() + o * 5, n * 20);
  return HERRO_OK;
}

// corrected bases of every window (device consensus) -> host, once per consensus pass
static int consensus_to_host(herro_job* job) {
  herro_ctx* ctx = job->ctx;
  if (job->consensus_on_host) return HERRO_OK;
  const uint32_t n = job->J.n_win;
  // device -> the job's pinned arena: no staging copy, no page pinning by the runtime at call time (a pageable destination
  // made the runtime lock user pages under the mm lock, which stalled the page faults of whoever was building the next job:
  // 40 ms spikes in the other feeder's herro_job_create)
  for (int attempt = 0;; attempt++) {
    if (n) HIP_TRY(ctx, hipMemcpyAsync(job->h_cons_len, job->J.cons_len, n * 4ull, hipMemcpyDeviceToHost, ctx->stream));
    if (job->row_elems) HIP_TRY(ctx, hipMemcpyAsync(job->h_cons_seq, job->J.cons_seq, job->row_elems, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->timer.collect();
    int rc = check_sib(ctx, job);
    if (!rc) break;
    if (attempt || (rc = sib_retry(job, rc))) return rc;   // repeated once: copy again what the second pass decoded
  }
  job->consensus_on_host = true;
  return HERRO_OK;
}

// Brings the corrected bases of the whole job to the host (what crosses PCIe on the way out: ~4 KB per window) and
// returns their number; herro_job_consensus_fasta afterwards only assembles text.  Requires herro_job_consensus.
int herro_job_consensus_fetch(herro_job* job, uint64_t* n_bases) {
  if (!job) return HERRO_E_INVALID;
  herro_ctx* ctx = job->ctx;
  if (!job->consensus_done) { ctx->err = "herro_job_consensus has not run"; return HERRO_E_STATE; }
  ProfSpan span_(ctx, "fetch");
  (void)hipSetDevice(ctx->device);
  int rc = consensus_to_host(job);
  if (rc) return rc;
  uint64_t tot = 0;
  for (uint32_t w = 0; w < job->J.n_win; w++) tot += job->h_cons_len[w];
  if (n_bases) *n_bases = tot;
  return HERRO_OK;
}

// FASTA records of target t from the device consensus (corrected bases of every window on the host already): windows are
// concatenated, the read is split where a window has fewer than two alignments (consensus.rs:90-111, lib.rs:282-317).
// out == nullptr: only the size is computed.  Returns the bytes the records take.
static uint64_t fasta_from_device_consensus(const herro_job* job, uint32_t t, const char* id, const char* desc, char* out) {
  const uint32_t w0 = job->tgt_win_off[t], w1 = job->tgt_win_off[t + 1];
  int64_t st = -1, en = -1;   // first..last window with n_alns > 1 (consensus.rs:90-101)
  for (uint32_t w = w0; w < w1; w++)
    if (std::min<uint32_t>(job->h_nkept[w], 30) > 1) { if (st < 0) st = w; en = w + 1; }
  if (st < 0) return 0;
  // segments: maximal runs of corrected windows; empty segments are dropped like empty strings in the reference
  struct Seg { uint32_t a, b; uint64_t len; };
  Seg segs_small[8];
  std::vector<Seg> segs_big;
  uint32_t n_seg = 0;
  auto push = [&](uint32_t a, uint32_t b, uint64_t len) {
    if (n_seg < 8) segs_small[n_seg] = Seg{a, b, len};
    else { if (n_seg == 8) segs_big.assign(segs_small, segs_small + 8); segs_big.push_back(Seg{a, b, len}); }
    n_seg++;
  };
  uint32_t run0 = (uint32_t)st;
  uint64_t run_len = 0;
  for (uint32_t w = (uint32_t)st; w < (uint32_t)en; w++) {
    if (std::min<uint32_t>(job->h_nkept[w], 30) < 2) {
      if (run_len) push(run0, w, run_len);
      run0 = w + 1; run_len = 0;
      continue;
    }
    run_len += job->h_cons_len[w];
  }
  if (run_len) push(run0, (uint32_t)en, run_len);
  const Seg* segs = n_seg > 8 ? segs_big.data() : segs_small;
  const size_t id_len = strlen(id), desc_len = desc ? strlen(desc) : 0;
  uint64_t o = 0;
  char num[16];
  for (uint32_t i = 0; i < n_seg; i++) {
    int nd = 0;
    if (n_seg > 1) nd = snprintf(num, sizeof num, ":%u", i);
    const uint64_t head = 1 + id_len + (uint64_t)nd + 1 + desc_len + 1;   // '>' id [:i] ' ' [desc] '\n'
    if (out) {
      char* p = out + o;
      *p++ = '>';
      memcpy(p, id, id_len); p += id_len;
      memcpy(p, num, (size_t)nd); p += nd;
      *p++ = ' ';
      if (desc_len) { memcpy(p, desc, desc_len); p += desc_len; }
      *p++ = '\n';
      for (uint32_t w = segs[i].a; w < segs[i].b; w++) {
        if (std::min<uint32_t>(job->h_nkept[w], 30) < 2) continue;
        memcpy(p, job->h_cons_seq + job->win[w].row_off, job->h_cons_len[w]);
        p += job->h_cons_len[w];
      }
      *p++ = '\n';
    }
    o += head + segs[i].len + 1;
  }
  return o;
}

// consensus.rs:86-227 + lib.rs:282-317 on the host, from device results.
int64_t herro_job_consensus_fasta(herro_job* job, uint32_t t, const char* id, const char* desc, char* out,
                                  uint64_t cap) {
  if (!job || t >= job->n_targets || !id || !out) return HERRO_E_INVALID;
  herro_ctx* ctx = job->ctx;
  int rc = job_sync(job);
  if (rc) return rc;
  const uint32_t w0 = job->tgt_win_off[t], w1 = job->tgt_win_off[t + 1];
  bool need_logits = false;
  for (uint32_t w = w0; w < w1; w++) need_logits |= job->h_nsup[w] > 0 && std::min<uint32_t>(job->h_nkept[w], 30) >= 2;
  if (need_logits && (rc = logits_to_host(job))) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // first..last window with n_alns > 1 (consensus.rs:90-101)
  int64_t st = -1, en = -1;
  for (uint32_t w = w0; w < w1; w++)
    if (std::min<uint32_t>(job->h_nkept[w], 30) > 1) { if (st < 0) st = w; en = w + 1; }
  if (st < 0) return 0;
  std::vector<std::string> seqs;
  std::string cur;
  if (job->consensus_done) {  // device consensus: concatenate the windows' corrected bases
    if ((rc = consensus_to_host(job))) return rc;
    const uint64_t need = fasta_from_device_consensus(job, t, id, desc, nullptr);
    if (need > cap) { ctx->err = "output buffer too small"; return HERRO_E_INVALID; }
    fasta_from_device_consensus(job, t, id, desc, out);
    return (int64_t)need;
  }
  static const char UP[10] = {'A', 'C', 'G', 'T', '*', 'A', 'C', 'G', 'T', '*'};
  static const int CNT[10] = {0, 1, 2, 3, 4, 0, 1, 2, 3, 4};
  std::vector<uint8_t> pb;
  for (uint32_t w = (uint32_t)st; w < (uint32_t)en; w++) {
    const uint32_t n_alns = std::min<uint32_t>(job->h_nkept[w], 30);
    if (n_alns < 2) {
      if (!cur.empty()) { seqs.push_back(cur); cur.clear(); }
      continue;
    }
    const WinDesc& wd = job->win[w];
    const uint32_t L = job->h_Lf[w], ns = job->h_nsup[w], n_rows = n_alns + 1;
    if ((rc = fetch_planes(job, w, pb, nullptr))) return rc;
    std::vector<uint32_t> srow(ns);
    if (ns) HIP_TRY(ctx, hipMemcpy(srow.data(), job->J.sup_row + wd.row_off, ns * 4ull, hipMemcpyDeviceToHost));
    const float* bl = ns ? job->h_base.data() + job->sup_off[w] * 5 : nullptr;
    uint32_t k = 0;  // informative rows are sorted by row, so one cursor replaces the hash map
    for (uint32_t r = 0; r < L; r++) {
      char base;
      if (k < ns && srow[k] == r) {
        const float* b = bl + (size_t)k * 5;
        int arg = 0;  // max_by_key: the LAST maximum wins; NaN is the greatest (consensus.rs:136-141)
        for (int c = 1; c < 5; c++) {
          const float v = b[c], m = b[arg];
          const bool ge = std::isnan(v) ? true : (std::isnan(m) ? false : v >= m);
          if (ge) arg = c;
        }
        base = "ACGT*"[arg];
        k++;
      } else {
        uint8_t counts[5] = {0, 0, 0, 0, 0};
        for (uint32_t c = 0; c < n_rows; c++) {
          const uint8_t tk = pb[(size_t)c * wd.lub + r];
          if (tk != TOK_NONE) {
            if (tk >= 10) { ctx->err = "token >= 10 in consensus"; return HERRO_E_REFERENCE_PANIC; }
            counts[CNT[tk]]++;
          }
        }
        int ord[5] = {0, 1, 2, 3, 4};
        std::stable_sort(ord, ord + 5, [&](int a, int b) { return counts[a] > counts[b]; });
        const uint8_t c0 = counts[ord[0]], c1 = counts[ord[1]];
        const char b0 = UP[ord[0]], b1 = UP[ord[1]];
        const uint8_t t0 = pb[r];
        if (t0 >= 10) { ctx->err = "target token >= 10 in consensus"; return HERRO_E_REFERENCE_PANIC; }
        const char tb = UP[t0];
        base = (c0 < 2 || (c0 == c1 && (b0 == tb || b1 == tb))) ? tb : b0;
      }
      if (base != '*') cur.push_back(base);
    }
  }
  if (!cur.empty()) seqs.push_back(cur);
  std::string fa;
  for (size_t i = 0; i < seqs.size(); i++) {  // lib.rs:282-317
    fa += ">";
    fa += id;
    if (seqs.size() == 1) fa += " ";
    else fa += ":" + std::to_string(i) + " ";
    if (desc) fa += desc;
    fa += "\n";
    fa += seqs[i];
    fa += "\n";
  }
  if (fa.size() > cap) { ctx->err = "output buffer too small"; return HERRO_E_INVALID; }
  std::memcpy(out, fa.data(), fa.size());
  return (int64_t)fa.size();
}

int64_t herro_job_fasta(herro_job* job, const char* const* ids, const char* const* descs, char* out, uint64_t cap,
                        uint64_t* rec_end) {
  if (!job || (job->n_targets && !ids)) return HERRO_E_INVALID;
  herro_ctx* ctx = job->ctx;
  if (!job->consensus_done) { ctx->err = "herro_job_consensus has not run"; return HERRO_E_STATE; }
  int rc = job_sync(job);
  if (rc) return rc;
  (void)hipSetDevice(ctx->device);
  if ((rc = consensus_to_host(job))) return rc;
  const uint32_t nt = job->n_targets;
  // sizes first (cheap: sums of window lengths), then every target's text straight into the caller's buffer by the pool
  std::vector<uint64_t> end(nt + 1, 0);
  for (uint32_t t = 0; t < nt; t++) end[t + 1] = end[t] + (ids[t] ? fasta_from_device_consensus(job, t, ids[t], descs ? descs[t] : nullptr, nullptr) : 0);
  const uint64_t tot = end[nt];
  if (rec_end) for (uint32_t t = 0; t < nt; t++) rec_end[t] = end[t + 1];
  if (!out) return (int64_t)tot;
  if (tot > cap) { ctx->err = "output buffer too small (" + std::to_string(tot) + " bytes needed)"; return HERRO_E_INVALID; }
  host_pool(ctx).run((nt + 63) / 64, [&](uint32_t b) {
    for (uint32_t t = b * 64; t < std::min(nt, (b + 1) * 64); t++)
      if (ids[t]) fasta_from_device_consensus(job, t, ids[t], descs ? descs[t] : nullptr, out + end[t]);
  });
  return (int64_t)tot;
}

// ---- the corrected reads as FASTA formed on the device, chopped for the assembler (fasta_dev.hip, chop_plan.h) ----------------
// herro_job_fasta's records (consensus.rs:90-111, lib.rs:282-317) and scripts/postprocess_corrected.sh behind them (`seqkit sliding -s 30000 -W 30000
// -g`, `seqkit seq -m 10000`), written by kernels from the bases the consensus pass left on the device: no padded window slot crosses PCIe and the
// host pool assembles nothing.  The text is copied chunk by chunk to its place in ONE pinned block that the handle owns until it is freed.
// consensus_on_host is neither read nor set: herro_job_fasta of the same job still fetches and assembles as before.
struct herro_fasta_text {
  std::shared_ptr<PinPool> pool;   // the text lies in a pinned block of the context's pool (api_ctx.h) and goes back there
  Arena block{};
  uint64_t len = 0;
  std::vector<uint64_t> target_end;
  herro::FastaStats st;
  ~herro_fasta_text() { if (pool) pool->release(block); }
};

int herro_job_fasta_dev(herro_job* job, const char* const* ids, const char* const* descs, const herro_chop_params* params, herro_fasta_text** out) {
  if (!job || !out) return HERRO_E_INVALID;
  *out = nullptr;
  herro_ctx* ctx = job->ctx;
  const char* const who = "herro_job_fasta_dev";
  if (job->n_targets && !ids) { ctx->err = std::string(who) + ": ids is NULL"; return HERRO_E_INVALID; }
  herro::ChopRule R;
  {
    std::string why;
    if (const int rc = herro::chop_check(who, params, R, why)) { ctx->err = why; return rc; }
  }
  if (!job->consensus_done) { ctx->err = "herro_job_consensus has not run"; return HERRO_E_STATE; }
  // window slots below 2^32 bytes: the base prefixes are 32-bit, and a piece has at least one base, so there are never more than 2^32 - 1 pieces
  if (job->row_elems > herro::FASTA_MAX_ROW_ELEMS) { ctx->err = std::string(who) + ": a job of 2^32 corrected bases or more (more than 2^32 - 1 pieces at chop_len 1)"; return HERRO_E_UNSUPPORTED; }
  int rc = job_sync(job);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const uint32_t nt = job->n_targets;
  herro::FastaNames names;
  names.off.assign(2ull * nt + 1, 0);
  names.present.assign(nt, 0);
  for (uint32_t t = 0; t < nt; t++) {
    names.off[2ull * t] = names.blob.size();
    if (ids[t]) { names.present[t] = 1; names.blob += ids[t]; }
    names.off[2ull * t + 1] = names.blob.size();
    if (ids[t] && descs && descs[t]) names.blob += descs[t];
  }
  names.off[2ull * nt] = names.blob.size();
  // the sibling-tile check of consensus_to_host, in front of the kernels instead of behind the copy: every model pass queued so far is complete
  // once the stream is idle, and a pass that is repeated (once) is repeated before any text is formed, so the text is the second pass's
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->timer.collect();
  if ((rc = check_sib(ctx, job)) && (rc = sib_retry(job, rc))) return rc;
  uint64_t chunk = ctx->debug_fasta_chunk;
  if (!chunk) {
    const char* e = getenv("HERRO_FASTA_SCRATCH_MB");
    const uint64_t budget = e ? (uint64_t)std::max(1ll, atoll(e)) << 20 : 1024ull << 20;
    chunk = std::max<uint64_t>(budget / 16, 16);   // the two device halves stay an eighth of the budget (the division of herro_pairs_paf's chunks)
  }
  std::unique_ptr<herro_fasta_text> h(new herro_fasta_text());
  h->pool = ctx->text_pin;
  // recycled memory: the device blocks go back to the context's list when the call is over (the stream is idle then), the pinned block with the handle
  std::vector<Arena> dev_blocks;
  herro::FastaMem mem;
  mem.dev = [&](uint64_t bytes) -> void* { dev_blocks.push_back(small_acquire(ctx, bytes)); return dev_blocks.back().p; };
  mem.text = [&](uint64_t bytes) -> char* { h->block = h->pool->acquire(bytes); return (char*)h->block.p; };
  std::string msg;
  char* text = nullptr;
  const int frc = herro::fasta_text_dev(job->J, job->row_elems, job->tgt_win_off.data(), nt, names, R, chunk, ctx->stream, mem, &text, &h->len, h->target_end, h->st, msg);
  for (Arena& a : dev_blocks) small_release(ctx, a);
  if (frc != herro::FASTA_OK) {
    ctx->err = msg;
    return HERRO_E_NO_DEVICE;
  }
  const char* e = getenv("HERRO_FASTA_STATS");   // (tools/fastarate.py): one line on stderr
  if (e && atoi(e))
    fprintf(stderr, "FASTA targets=%llu segments=%llu pieces=%llu dropped=%llu bytes=%llu chunks=%llu seg_ms=%.3f piece_ms=%.3f write_ms=%.3f\n",
            (unsigned long long)h->st.n_targets, (unsigned long long)h->st.segments, (unsigned long long)h->st.records, (unsigned long long)h->st.dropped,
            (unsigned long long)h->st.bytes, (unsigned long long)h->st.chunks, h->st.seg_ms, h->st.piece_ms, h->st.write_ms);
  *out = h.release();
  return HERRO_OK;
}

const char* herro_fasta_text_data(const herro_fasta_text* t) { return t && t->len ? (const char*)t->block.p : nullptr; }
uint64_t herro_fasta_text_len(const herro_fasta_text* t) { return t ? t->len : 0; }
const uint64_t* herro_fasta_text_target_end(const herro_fasta_text* t) { return t ? t->target_end.data() : nullptr; }
int herro_fasta_text_stats(const herro_fasta_text* t, uint64_t out[6]) {
  if (!t || !out) return HERRO_E_INVALID;
  out[0] = t->st.records; out[1] = t->st.bases; out[2] = t->st.dropped; out[3] = t->st.bases_dropped; out[4] = t->st.segments; out[5] = t->st.targets;
  return HERRO_OK;
}
void herro_fasta_text_free(herro_fasta_text* t) { delete t; }
int herro_debug_set_fasta_chunk(herro_ctx* ctx, uint64_t bytes) {
  if (!ctx) return HERRO_E_INVALID;
  ctx->debug_fasta_chunk = bytes;
  return HERRO_OK;
}

int64_t herro_job_write_features(herro_job* job, const char* base_dir, const char* const* read_names) {
  if (!job || !base_dir || !read_names) return HERRO_E_INVALID;
  herro_ctx* ctx = job->ctx;
  int rc = job_sync(job);
  if (rc) return rc;
  int64_t n = 0;
  std::vector<uint8_t> bases, quals, sins;
  std::vector<uint16_t> spos;
  std::vector<uint32_t> qids;
  std::vector<const char*> ids;
  for (uint32_t t = 0; t < job->n_targets; t++) {
    for (uint32_t w = job->tgt_win_off[t]; w < job->tgt_win_off[t + 1]; w++) {
      const WinDesc& wd = job->win[w];
      const uint32_t L = job->h_Lf[w], ns = job->h_nsup[w], nk = job->h_nkept[w];
      bases.resize((size_t)L * HERRO_ROWS); quals.resize(bases.size());
      spos.resize(ns); sins.resize(ns); qids.resize(nk); ids.resize(nk);
      if ((rc = herro_job_window_copy(job, w, 0, bases.data(), quals.data(), spos.data(), sins.data(), qids.data()))) return rc;
      for (uint32_t k = 0; k < nk; k++) {
        if (qids[k] >= ctx->n_reads || !read_names[qids[k]]) { ctx->err = "read name missing"; return HERRO_E_INVALID; }
        ids[k] = read_names[qids[k]];
      }
      if (wd.rid >= ctx->n_reads || !read_names[wd.rid]) { ctx->err = "read name missing"; return HERRO_E_INVALID; }
      const std::string dir = std::string(base_dir) + "/" + read_names[wd.rid];
      if ((rc = herro_write_window_features(dir.c_str(), wd.wid, ids.data(), nk, bases.data(), quals.data(), L, spos.data(), sins.data(), ns))) {
        ctx->err = "cannot write features under " + dir;
        return rc;
      }
      n++;
    }
  }
  return n;
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
  std::vector<void*> tmp;
  auto A = [&](uint64_t bytes) -> void* { void* p = nullptr; if (hipMalloc(&p, std::max<uint64_t>(bytes, 16)) == hipSuccess) tmp.push_back(p); return p; };
  auto done = [&](int code) { for (void* p : tmp) (void)hipFree(p); return code; };
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
  if (!d_src_b || !d_src_q || !d_pb || !d_pq || !d_sr || !d_info || !d_base) { ctx->err = "out of device memory"; return done(HERRO_E_NO_DEVICE); }
  launch_transpose_blr(d_src_b, d_pb, B, L, st);
  launch_transpose_blr(d_src_q, d_pq, B, L, st);
  int rc = HERRO_OK;
  if ((rc = ensure_scratch(ctx, (uint32_t)N))) return done(rc);
  // one group of B windows through the builder herro_job_infer uses.  The row cap is fused_tok_cap whatever happened before: job->no_sib is the retry of a job
  // whose sibling tiles timed out, and a forward has no retry (check_sib below reports such a pass as failed).  No rf_base: the kernels read the planes at out_off.
  std::vector<PlanWin> wins(B);
  for (uint32_t b = 0; b < B; b++) wins[b] = PlanWin{(uint32_t)lens[b], L, L, L, (uint64_t)b * HERRO_ROWS * L, tok_off[b], tok_off[b], 0};
  std::vector<unsigned char> image;   // complete before its upload, alive until the stream is synchronised below
  std::vector<LaunchOffs> offs;
  build_launch(wins, launch_cfg(ctx, fused_tok_cap(ctx), false), image, offs);
  const void* d_image = up(image.data(), image.size());
  if (!d_image || e != hipSuccess) { ctx->err = e != hipSuccess ? hipGetErrorString(e) : "out of device memory"; (void)hipStreamSynchronize(st); return done(HERRO_E_NO_DEVICE); }
  for (const LaunchOffs& o : offs) {
    if (o.n_tiles_b && (rc = ensure_sib(ctx, o.n_tiles_b))) { (void)hipStreamSynchronize(st); return done(rc); }
    BatchDev bd = batch_dev(d_image, o);
    bd.planes_b = d_pb; bd.planes_q = d_pq; bd.rf_q = nullptr; bd.sup_row = d_sr; bd.out_info = d_info; bd.out_base = d_base;
    run_model(ctx, bd, o.tiled);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) { ctx->err = hipGetErrorString(e); return done(HERRO_E_NO_DEVICE); }
  ctx->timer.collect();
  if ((rc = check_sib(ctx, nullptr))) return done(rc);
  HIP_TRY(ctx, hipMemcpy(info_logits, d_info, N * 4, hipMemcpyDeviceToHost));
  HIP_TRY(ctx, hipMemcpy(bases_logits, d_base, N * 20, hipMemcpyDeviceToHost));
  return done(HERRO_OK);
}

// ---- host-only test hooks: the host half of herro_job_create without a device ------------------------
// herro_debug_host_ctx builds a context that only knows the read lengths (and name classes); herro_job_create on it
// runs CIGAR parsing, windowing, validation and the merge, then stops; herro_debug_job_array exposes the descriptors.
herro_ctx* herro_debug_host_ctx(uint32_t n_reads, const uint32_t* read_len, const uint32_t* name_class) {
  auto ctx = new herro_ctx();
  ctx->host_only = true;
  ctx->n_reads = n_reads;
  ctx->read_len.assign(read_len, read_len + n_reads);
  ctx->name_class.resize(n_reads);
  for (uint32_t i = 0; i < n_reads; i++) ctx->name_class[i] = name_class ? name_class[i] : i;
  ctx->h_word_off.assign(n_reads + 1, 0);
  ctx->h_qual_off.assign(n_reads + 1, 0);
  for (uint32_t i = 0; i < n_reads; i++) {  // the layout herro_set_reads produces
    ctx->h_word_off[i + 1] = ctx->h_word_off[i] + ((uint64_t)read_len[i] + 31) / 32;
    ctx->h_qual_off[i + 1] = ctx->h_qual_off[i] + read_len[i];
  }
  return ctx;
}

// Host-only test hook: the position-space rules of k_rows (pileup_core.h: sat2_add, sat2_merge, base_row_votes) on n count vectors.
// counts[i][5] = occurrences of A C G T * on a base row (the target's own base included), target[i] = the target's base 0..3; the
// counts are fed column by column into the saturating bit-sliced counters — split[i][5] of them into a second set that is merged in,
// as the two halves of k_rows' workgroup do — and the planes are read back: sup[i] = informative, vote[i] = the decoder's call 0..4.
int herro_debug_base_row_votes(const uint8_t* counts, const uint8_t* split, const uint8_t* target, uint32_t n, uint8_t* sup, uint8_t* vote) {
  if (!counts || !target || !sup || !vote) return HERRO_E_INVALID;
  for (uint32_t g0 = 0; g0 < n; g0 += 32) {
    const uint32_t m = std::min(32u, n - g0);
    uint32_t a0[5] = {0, 0, 0, 0, 0}, a1[5] = {0, 0, 0, 0, 0}, b0[5] = {0, 0, 0, 0, 0}, b1[5] = {0, 0, 0, 0, 0}, tsym[4] = {0, 0, 0, 0};
    const uint32_t vm = m == 32 ? 0xffffffffu : ((1u << m) - 1u);
    for (uint32_t i = 0; i < m; i++) {
      if (target[g0 + i] > 3) return HERRO_E_INVALID;
      tsym[target[g0 + i]] |= 1u << i;
    }
    for (int q = 0; q < 5; q++)
      for (uint32_t k = 0; k < 255; k++) {   // column k shows symbol q where the count exceeds k
        uint32_t xa = 0, xb = 0;
        for (uint32_t i = 0; i < m; i++) {
          const uint32_t c = counts[(size_t)(g0 + i) * 5 + q], s = split ? std::min<uint32_t>(split[(size_t)(g0 + i) * 5 + q], c) : 0u;
          if (k < c - s) xa |= 1u << i;
          if (k < s) xb |= 1u << i;
        }
        if (!xa && !xb) break;
        sat2_add(a0[q], a1[q], xa);
        sat2_add(b0[q], b1[q], xb);
      }
    for (int q = 0; q < 5; q++) sat2_merge(a0[q], a1[q], b0[q], b1[q]);
    const RowVotes r = base_row_votes(a0, a1, tsym, vm);
    for (uint32_t i = 0; i < m; i++) {
      sup[g0 + i] = (uint8_t)((r.sup >> i) & 1u);
      vote[g0 + i] = (uint8_t)(((r.v0 >> i) & 1u) | (((r.v1 >> i) & 1u) << 1) | (((r.v2 >> i) & 1u) << 2));
    }
  }
  return HERRO_OK;
}

// the decoder's vote on exact counts (insertion rows of k_rows; pileup_core.h vote5)
uint32_t herro_debug_vote5(const uint32_t* c5, uint32_t tb) {
  const uint32_t c[5] = {c5[0], c5[1], c5[2], c5[3], c5[4]};
  return vote5(c, tb);
}

int herro_debug_set_featurize_planes(herro_ctx* ctx, int on) {
  if (!ctx) return HERRO_E_INVALID;
  ctx->lean = on == 0;
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

// 1: the last herro_job_infer read the receptive fields k_rows gathered behind featurize; 0: k_rfq gathered them (a window above 256 informative
// rows, a buffer sized too small by the estimate of a first pass, the planes path, HERRO_RF_FUSED=0)
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

int herro_clock_probe(herro_ctx* ctx, double* shader_mhz) {
  if (!ctx || !shader_mhz) return HERRO_E_INVALID;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int wall_khz = 0;
  HIP_TRY(ctx, hipDeviceGetAttribute(&wall_khz, hipDeviceAttributeWallClockRate, ctx->device));
  unsigned long long* d = nullptr;
  HIP_TRY(ctx, hipMalloc((void**)&d, 32));
  hipLaunchKernelGGL(k_clock_probe, dim3(1), dim3(64), 0, ctx->stream, d, 20000u);
  unsigned long long h[3] = {0, 0, 0};
  hipError_t e = hipMemcpyAsync(h, d, sizeof h, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  (void)hipFree(d);
  HIP_TRY(ctx, e);
  *shader_mhz = h[1] ? (double)h[0] / (double)h[1] * (double)wall_khz * 1e-3 : 0.0;
  return HERRO_OK;
}
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

// the directory words k_cols wrote for overlap-window `ow` (JobDev::cwd: one per word of 32 window positions; read-only, valid once herro_job_featurize
// has run, and meaningful for a slice the long-indel filter kept — a dropped slice's words are never written)
int64_t herro_debug_job_cwd(herro_job* job, uint32_t ow, uint32_t* out, uint64_t cap) {
  if (!job || !out) return HERRO_E_INVALID;
  herro_ctx* ctx = job->ctx;
  if (ctx->host_only || !job->featurized) { ctx->err = "herro_job_featurize has not run"; return HERRO_E_STATE; }
  if (ow >= job->J.n_ow || cap < job->J.nw) { ctx->err = "overlap-window index out of range or output buffer too small"; return HERRO_E_INVALID; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  HIP_TRY(ctx, hipMemcpy(out, job->J.cwd + (uint64_t)ow * job->J.nw, (size_t)job->J.nw * 4, hipMemcpyDeviceToHost));
  return (int64_t)job->J.nw;
}

// the base logits of every informative row of the job (job order, n_rows x 5) replace the model's, on the device and in the host copy; the consensus
// is dropped, so the next herro_job_consensus / herro_job_consensus_fasta decodes these (tests plant ties, infinities and NaNs for the argmax)
int herro_debug_job_set_base_logits(herro_job* job, const float* base, uint64_t n_rows) {
  if (!job || (n_rows && !base)) return HERRO_E_INVALID;
  herro_ctx* ctx = job->ctx;
  int rc = job_sync(job);
  if (rc) return rc;
  if (!job->inferred) { ctx->err = "herro_job_infer has not run"; return HERRO_E_STATE; }
  const uint64_t tot = job->sup_off.back();
  if (n_rows != tot) { ctx->err = "n_rows " + std::to_string(n_rows) + " != the job's informative rows " + std::to_string(tot); return HERRO_E_INVALID; }
  if ((rc = logits_to_host(job))) return rc;   // the model pass is settled (and its info logits on the host) before its base logits are replaced
  if (tot) {
    std::memcpy(job->h_base.data(), base, tot * 20);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpy(job->d_base, base, tot * 20, hipMemcpyHostToDevice));
  }
  job->consensus_done = false;
  job->consensus_on_host = false;
  return HERRO_OK;
}

// which: 0 ops (u32), 1 OwDesc, 2 WinDesc, 3 tile_win (u32), 4 tile_r0 (u32), 5 tgt_win_off (u32).
// Returns the element count, *ptr the array, *elem_bytes the element size.
int64_t herro_debug_job_array(herro_job* job, int which, const void** ptr, uint32_t* elem_bytes) {
  if (!job || !ptr || !elem_bytes) return HERRO_E_INVALID;
  switch (which) {
    case 0:
      *elem_bytes = 4;
      // ops written by the device scan: the whole (gapped) op array, so that OwDesc::op_begin indexes it
      if (job->scan.p) return debug_fetch(job, job->dbg_ops, job->scan.p, job->scan_ops, ptr);
      *ptr = job->ops.data();
      return (int64_t)job->ops.size();
    case 1:
      *elem_bytes = sizeof(OwDesc);
      if (job->dev_built) return debug_fetch(job, job->dbg_ow, job->J.ow, job->J.n_ow, ptr);
      *ptr = job->ow.data();
      return (int64_t)job->ow.size();
    case 2: *ptr = job->win.data(); *elem_bytes = sizeof(WinDesc); return (int64_t)job->win.size();
    case 3:
    case 4:
      *elem_bytes = 4;
      if (job->dev_built) return debug_fetch(job, which == 3 ? job->dbg_tw : job->dbg_tr, which == 3 ? job->J.tile_win : job->J.tile_r0, job->J.n_tiles, ptr);
      *ptr = which == 3 ? job->tile_win.data() : job->tile_r0.data();
      return (int64_t)(which == 3 ? job->tile_win.size() : job->tile_r0.size());
    case 5: *ptr = job->tgt_win_off.data(); *elem_bytes = 4; return (int64_t)job->tgt_win_off.size();
    default: return HERRO_E_INVALID;
  }
}

// ---- host-only test hook: the product's windowing on one alignment (no device needed) -----------
// out rows of 8 u64: window, tstart, qstart, qend, op_lo, op_hi, start_off, end_off.
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

int64_t herro_debug_extract_windows(const herro_alignment* a, uint32_t n_windows, uint32_t W, uint64_t* out,
                                    uint64_t cap, char* err, uint64_t err_cap) {
  std::vector<uint32_t> ops;
  std::vector<HostOw> hows;
  BuildError be;
  if (!a || !parse_cigar(a->cigar, a->cigar_len, ops, be) || !window_alignment(ops, *a, W, n_windows, hows, be)) {
    if (err && err_cap) { std::strncpy(err, a ? be.msg.c_str() : "null", err_cap - 1); err[err_cap - 1] = 0; }
    return a ? be.code : HERRO_E_INVALID;
  }
  if (hows.size() > cap) return HERRO_E_INVALID;
  for (size_t k = 0; k < hows.size(); k++) {
    uint64_t* o = out + 8 * k;
    o[0] = hows[k].win; o[1] = hows[k].tstart; o[2] = hows[k].qstart; o[3] = hows[k].qend;
    o[4] = hows[k].op_lo; o[5] = hows[k].op_hi; o[6] = hows[k].start_off; o[7] = hows[k].end_off;
  }
  return (int64_t)hows.size();
}

// ---- measurement -----------------------------------------------------------------------------------
int herro_timing_enable(herro_ctx* ctx, int on) { if (!ctx) return HERRO_E_INVALID; ctx->timer.on = on != 0; return HERRO_OK; }
int herro_timing_reset(herro_ctx* ctx) {
  if (!ctx) return HERRO_E_INVALID;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->timer.reset();
  return HERRO_OK;
}
int herro_timing_get(herro_ctx* ctx, char* names, uint64_t cap, double* ms, uint64_t* calls, uint32_t* n) {
  if (!ctx || !n) return HERRO_E_INVALID;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->timer.collect();
  std::string s;
  uint32_t k = 0;
  for (auto& nm : ctx->timer.order) {
    if (k < *n) {
      if (ms) ms[k] = ctx->timer.acc[nm].first;
      if (calls) calls[k] = ctx->timer.acc[nm].second;
    }
    s += nm;
    s += "\n";
    k++;
  }
  if (names && cap) { std::strncpy(names, s.c_str(), cap - 1); names[cap - 1] = 0; }
  *n = k;
  return HERRO_OK;
}

int herro_job_stats(herro_job* job, uint64_t* out) {
  if (!job || !out) return HERRO_E_INVALID;
  int rc = job_sync(job);
  if (rc) return rc;
  uint64_t sumL = 0, sumS = 0, nz = 0;
  for (size_t w = 0; w < job->win.size(); w++) { sumL += job->h_Lf[w]; sumS += job->h_nsup[w]; nz += job->h_nsup[w] > 0; }
  out[0] = job->alg_read_bytes; out[1] = job->alg_op_bytes; out[2] = 2ull * HERRO_ROWS * sumL;
  out[3] = sumL; out[4] = sumS; out[5] = nz;
  return HERRO_OK;
}

// ---- a job from device-resident alignments (the handle and its helpers: aligned_dev.h, frontend_api.hip) ----------------------
herro_job* herro_job_create_aligned(herro_ctx* ctx, uint32_t n_targets, const uint32_t* rids, const uint64_t* aln_off, const uint32_t* rec,
                                    const herro_aligned_dev* a, uint32_t W) {
  if (!ctx) return nullptr;
  auto fail = [&](int code, const std::string& m) { return create_fail(ctx, code, m); };
  ctx->create_code = HERRO_OK;
  if (!a) return fail(HERRO_E_INVALID, "herro_job_create_aligned: null handle");
  if (n_targets && (!rids || !aln_off)) return fail(HERRO_E_INVALID, "null argument");
  const uint64_t a0 = n_targets ? aln_off[0] : 0, a1 = n_targets ? aln_off[n_targets] : 0;
  if (a1 < a0) return fail(HERRO_E_INVALID, "aln_off must ascend");
  if (a1 > a0 && !rec) return fail(HERRO_E_INVALID, "herro_job_create_aligned: null rec");
  if (a->ctx != ctx) return fail(HERRO_E_INVALID, "herro_job_create_aligned: the handle belongs to another context");
  // the job's records, in its order: coordinates from the handle, ops by reference
  std::vector<herro_alignment> sel(a1);
  std::vector<uint64_t> off(a1, 0);
  std::vector<uint32_t> nops(a1, 0);
  uint64_t lo = ~0ull, hi = 0;
  for (uint64_t g = a0; g < a1; g++) {
    const uint32_t r = rec[g];
    if (r >= a->alns.size())
      return fail(HERRO_E_INVALID, "herro_job_create_aligned: rec[" + std::to_string(g) + "] = " + std::to_string(r) + " is outside the handle's " + std::to_string(a->alns.size()) + " records");
    if (!a->n_ops[r])
      return fail(HERRO_E_INVALID, "herro_job_create_aligned: rec[" + std::to_string(g) + "] = " + std::to_string(r) + " is a failed record (no ops)");
    sel[g] = a->alns[r];
    off[g] = a->op_off[r];
    nops[g] = a->n_ops[r];
    lo = std::min(lo, off[g]);
    hi = std::max(hi, off[g] + nops[g]);
  }
  if (!ctx->host_only && ctx->dev_scan && ctx->dev_build && a1 > a0) {   // direct: k_ops_scan reads the handle's store, no text anywhere
    const OpsSrc src{a->d_ops, off.data(), nops.data()};
    bool unsettled = false;
    herro_job* job = job_create_from(ctx, n_targets, rids, aln_off, sel.data(), W, &src, &unsettled);
    if (job || !unsettled) return job;
  }
  // Not taken (host build, host scan, a device-free context) or not settled (BuildTotals::err, the pre-pass): this job's ops come down, are formatted and
  // go through herro_job_create, whose results and error texts are then the text path's by construction.  The span [lo, hi) of the store comes down in one copy.
  std::vector<uint32_t> ops;
  if (a1 > a0) {
    const int rc = aligned_dev_fetch(a, lo, hi, ops);
    if (rc != HERRO_OK) return fail(rc, "herro_job_create_aligned: copying the ops down failed");
  }
  for (uint64_t g = a0; g < a1; g++) off[g] -= lo;
  std::string text;
  ops_text_block(ctx, ops.data(), off.data(), nops.data(), a0, a1, sel.data(), text);
  herro_job* job = herro_job_create(ctx, n_targets, rids, aln_off, sel.data(), W);
  if (job) job->from_ops_text = true;
  return job;
}

}  // extern "C"
