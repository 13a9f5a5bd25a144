// adapter_dev.hip — the adapter scan of the read store (adapter_dev.h; specification: DESIGN.md §13, tests/adapter_ref.py).  Kernels:
//   k_adapt_scan    one lane per segment of `seg` bases of a read; per pattern slot it runs adapt_scan_lane: Myers' recurrence on one column word
//                   (32 bits for a pattern of at most 32 bases — 1.5 x the rate of the 64-bit one, DESIGN.md §13 —, 64 bits otherwise),
//                   the text's two plane words loaded once per 32 bases, the pattern's planes in scalar registers (the slot index is uniform).
//                   A hit is appended behind a 64-bit counter; a buffer that turns out too small makes the host run the scan once more at
//                   the counted size.
//   k_adapt_start   one lane per hit: adapt_start_of, at most m + k bases in front of the hit's end.
// The atomic counter decides where a hit lies in the buffer and nothing else: the caller sorts the hits by the specification's key, which is
// unique per hit, so the bytes it returns depend neither on thread order nor on seg.  A read that is one long run (a homopolymer read against a
// homopolymer-like adapter) keeps ONE lane scanning to the read's end; that is accepted.
#include "adapter_dev.h"
#include "dev_bufs.h"

#include <algorithm>
#include <chrono>

namespace herro {
namespace {

__global__ __launch_bounds__(256) void k_adapt_scan(const uint32_t* __restrict__ p0, const uint32_t* __restrict__ p1, const uint64_t* __restrict__ word_off,
                                                    const uint64_t* __restrict__ base_off, const uint32_t* __restrict__ seg_off, uint32_t n_reads,
                                                    uint32_t n_segs, uint32_t seg, const AdaptPattern* __restrict__ pats, uint32_t n_slots,
                                                    uint4* __restrict__ hits, unsigned long long cap, unsigned long long* __restrict__ counter) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g >= n_segs) return;
  uint32_t lo = 0, hi = n_reads;           // the read of segment g: seg_off[r] <= g < seg_off[r + 1] (reads without a base own no segment)
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (seg_off[mid + 1] <= g) lo = mid + 1; else hi = mid;
  }
  const uint32_t r = lo;
  const uint32_t len = (uint32_t)(base_off[r + 1] - base_off[r]);
  const uint64_t s_lo = (uint64_t)(g - seg_off[r]) * seg;
  if (s_lo >= len) return;                 // (not reached: seg_off counts ceil(len / seg) segments)
  const uint32_t seg_lo = (uint32_t)s_lo, seg_hi = s_lo + seg < len ? (uint32_t)(s_lo + seg) : len;
  const uint32_t* const r0 = p0 + word_off[r];
  const uint32_t* const r1 = p1 + word_off[r];
  for (uint32_t s = 0; s < n_slots; s++) {
    const uint32_t m = pats[s].m;
    if (!m) continue;
    const uint32_t tag = (uint32_t)pats[s].adapter | (uint32_t)pats[s].strand << 16;
    auto emit = [&](uint32_t end, uint32_t errors) {
      const unsigned long long at = atomicAdd(counter, 1ull);
      if (at < cap) hits[at] = make_uint4(r, 0u, end, tag | errors << 24);   // herro_adapter_hit: rid, start, end, adapter | strand | errors
    };
    if (m <= 32) adapt_scan_lane<uint32_t>(r0, r1, len, seg_lo, seg_hi, (uint32_t)pats[s].n0, (uint32_t)pats[s].n1, m, pats[s].k, emit);
    else adapt_scan_lane<uint64_t>(r0, r1, len, seg_lo, seg_hi, pats[s].n0, pats[s].n1, m, pats[s].k, emit);
  }
}

__global__ __launch_bounds__(256) void k_adapt_start(const uint32_t* __restrict__ p0, const uint32_t* __restrict__ p1, const uint64_t* __restrict__ word_off,
                                                     const AdaptPattern* __restrict__ pats, uint4* __restrict__ hits, uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint4 h = hits[i];
  const AdaptPattern& P = pats[2u * (h.w & 0xffffu) + ((h.w >> 16) & 0xffu)];
  const uint64_t w = word_off[h.x];
  hits[i].y = adapt_start_of(p0 + w, p1 + w, h.z, h.w >> 24, P.r0, P.r1, P.m, P.k);
}

double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

}  // namespace

static_assert(sizeof(herro_adapter_hit) == 16 && sizeof(uint4) == 16, "a hit is one 16-byte store");

#define ADAPT_TRY(what, expr) do { const hipError_t _e = (expr); if (_e != hipSuccess) { err = std::string("herro_find_adapters: ") + what + ": " + hipGetErrorString(_e); return ADAPT_HIP; } } while (0)

int adapt_find(const AdaptStore& S, const std::vector<AdaptPattern>& pats, uint32_t seg, uint64_t cap0, hipStream_t st, std::vector<herro_adapter_hit>& out,
               AdaptStats& stats, std::string& err) {
  out.clear();
  stats = AdaptStats{};
  stats.seg = seg;
  std::vector<uint32_t> seg_off((size_t)S.n_reads + 1, 0);
  uint64_t n_segs = 0;
  for (uint32_t r = 0; r < S.n_reads; r++) {
    n_segs += ((uint64_t)S.h_len[r] + seg - 1) / seg;
    if (n_segs > 0xffffffffull) { err = "herro_find_adapters: more than 2^32 - 1 segments (raise HERRO_ADAPT_SEG)"; return ADAPT_UNSUPPORTED; }
    seg_off[r + 1] = (uint32_t)n_segs;
  }
  stats.segments = n_segs;
  if (!n_segs || pats.empty()) return ADAPT_OK;
  Bufs B;
  uint32_t* d_seg_off = nullptr;
  AdaptPattern* d_pats = nullptr;
  unsigned long long* d_counter = nullptr;
  ADAPT_TRY("segment table", B.bytes(&d_seg_off, 4 * seg_off.size()));
  ADAPT_TRY("patterns", B.bytes(&d_pats, sizeof(AdaptPattern) * pats.size()));
  ADAPT_TRY("counter", B.bytes(&d_counter, 8));
  ADAPT_TRY("segment table upload", hipMemcpyAsync(d_seg_off, seg_off.data(), 4 * seg_off.size(), hipMemcpyHostToDevice, st));
  ADAPT_TRY("pattern upload", hipMemcpyAsync(d_pats, pats.data(), sizeof(AdaptPattern) * pats.size(), hipMemcpyHostToDevice, st));
  const uint32_t blocks = (uint32_t)((n_segs + 255) / 256);
  // two adapters per read of a few kilobases are one hit per ~20 default segments: an eighth of the segments holds them; a denser read set
  // (short patterns at a high error bound) runs the scan a second time at the counted size
  uint64_t cap = cap0 ? cap0 : std::max<uint64_t>(65536, n_segs / 8);
  for (int pass = 0;; pass++) {
    Bufs H;
    uint4* d_hits = nullptr;
    ADAPT_TRY("hits", H.bytes(&d_hits, 16 * cap));
    ADAPT_TRY("counter reset", hipMemsetAsync(d_counter, 0, 8, st));
    const auto t0 = std::chrono::steady_clock::now();
    k_adapt_scan<<<blocks, 256, 0, st>>>(S.d_p0, S.d_p1, S.d_word_off, S.d_base_off, d_seg_off, S.n_reads, (uint32_t)n_segs, seg, d_pats,
                                         (uint32_t)pats.size(), d_hits, cap, d_counter);
    ADAPT_TRY("k_adapt_scan launch", hipGetLastError());
    unsigned long long count = 0;
    ADAPT_TRY("count", hipMemcpyAsync(&count, d_counter, 8, hipMemcpyDeviceToHost, st));
    ADAPT_TRY("k_adapt_scan", hipStreamSynchronize(st));
    stats.scan_ms += ms_since(t0);
    stats.scans++;
    if (count > 0xffffffffull) { err = "herro_find_adapters: more than 2^32 - 1 hits"; return ADAPT_UNSUPPORTED; }
    if (count > cap) {
      if (pass) { err = "herro_find_adapters: the hit count changed between two scans of the same store"; return ADAPT_HIP; }
      cap = count;
      continue;
    }
    stats.hits = count;
    if (!count) return ADAPT_OK;
    const auto t1 = std::chrono::steady_clock::now();
    k_adapt_start<<<(uint32_t)((count + 255) / 256), 256, 0, st>>>(S.d_p0, S.d_p1, S.d_word_off, d_pats, d_hits, (uint32_t)count);
    ADAPT_TRY("k_adapt_start launch", hipGetLastError());
    out.resize(count);
    ADAPT_TRY("hits", hipMemcpyAsync(out.data(), d_hits, 16 * count, hipMemcpyDeviceToHost, st));
    ADAPT_TRY("k_adapt_start", hipStreamSynchronize(st));
    stats.start_ms = ms_since(t1);
    return ADAPT_OK;
  }
}

}  // namespace herro
