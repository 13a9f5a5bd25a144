// herro_api.hip — the context of the C ABI (include/herro_amd.h): version and last error, herro_create / herro_destroy, the stream, the 2-bit codec, the
// read store, the context's memory (host pool, arenas, small buffers, registered host ranges) and the measurement entries.  Host C++ (compiled by hipcc).
// No CPU fallback anywhere: if HIP is unavailable every device call returns HERRO_E_NO_DEVICE.  The model is model_api.hip; jobs are job_create.hip,
// job_run.hip and job_out.hip; the front end is frontend_api.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "api_job.h"
#include "host_cpus.h"

using namespace herro;

namespace {
std::string g_create_err;

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
Arena small_acquire(herro_ctx* ctx, size_t need) {
  Arena a;
  { std::lock_guard<std::mutex> lk(ctx->arena_mu); a = best_fit_take(ctx->free_small, need); }
  if (a.p) return a;
  a.cap = need + need / 4 + 4096;
  if (hipMalloc(&a.p, a.cap) != hipSuccess) { a.p = nullptr; a.cap = 0; }
  return a;
}
void small_release(herro_ctx* ctx, Arena& a) {
  if (!a.p) return;
  std::lock_guard<std::mutex> lk(ctx->arena_mu);
  if (ctx->free_small.size() < 24) ctx->free_small.push_back(a); else (void)hipFree(a.p);
  a = Arena{};
}

// A job-sized block from one of the context's free lists (best fit), or a fresh one with 12 % slack.
// kind: 0 pinned host, 1 device; host-only contexts get plain malloc.
Arena arena_acquire(herro_ctx* ctx, std::vector<Arena>& list, size_t need, int kind) {
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
void arena_release(herro_ctx* ctx, std::vector<Arena>& list, Arena& a, int kind) {
  if (!a.p) return;
  std::lock_guard<std::mutex> lk(ctx->arena_mu);
  if (list.size() < 6) list.push_back(a);
  else if (ctx->host_only) std::free(a.p);
  else if (kind == 1) (void)hipFree(a.p);
  else (void)hipHostFree(a.p);
  a = Arena{};
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

}  // extern "C"

// ---- host ranges registered for zero-copy job creation (herro_host_register) -----------------------------------------------------
// Process-wide: several contexts (feeder threads) create jobs from the same alignment buffer; a range is pinned once and counted.
namespace {
struct HostReg { const unsigned char* p; uint64_t n; int refs; const unsigned char* dp; };   // dp: the range as kernels see it (hipHostGetDevicePointer; null: not mapped)
std::mutex g_reg_mu;
std::vector<HostReg> g_regs;
}  // namespace
std::atomic<uint64_t> g_zero_copy_jobs{0};   // jobs whose texts went up straight from a registered range (plan_scan of job_create.hip counts; herro_debug_zero_copy_jobs)
// *dev (may be null): where kernels read the byte at `lo` directly, if the range is mapped AND 16-byte pieces read around [lo, hi) stay on its pinned pages
bool host_range_registered(const unsigned char* lo, const unsigned char* hi, const unsigned char** dev) {
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

extern "C" {

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

// ---- measurement -----------------------------------------------------------------------------------
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

}  // extern "C"
