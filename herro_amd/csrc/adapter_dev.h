// adapter_dev.h — approximate matches of up to 64 short patterns (adapters, both strands) in every read of the resident store
// (adapter_dev.hip): the GPU counterpart of the adapter search of porechop / duplex_tools in the reference's scripts/preprocess.sh.
// Myers' bit-vector recurrence (1999) over the store's bit planes, one 32- or 64-bit column per pattern; the specification is DESIGN.md §13
// and tests/adapter_ref.py, and the kernels equal it record for record, whatever the segment length.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/herro_amd.h"

namespace herro {

constexpr uint32_t ADAPT_SEG_DEFAULT = 256;      // bases a lane owns
constexpr uint32_t ADAPT_SEG_MIN = 8, ADAPT_SEG_MAX = 65536;

// Slot 2 a + s of the pattern table is adapter a on strand s; m = 0: the slot is not searched (HERRO_ADAPTERS_FORWARD_ONLY).
// One pattern of m bases: bit i of its planes is base i.  The scan's match vector of a text base with code bits (b0, b1) is
// (n0 ^ -b0) & (n1 ^ -b1): n0 / n1 are the COMPLEMENTS of the pattern's low / high code-bit planes.  r0 / r1: the same of the reversed pattern
// (k_adapt_start).  Bits at and above m are never read back: carries and shifts of the recurrence only move upwards.
struct AdaptPattern {
  uint64_t n0, n1, r0, r1;
  uint32_t m, k;
  uint16_t adapter;
  uint8_t strand, pad;
  uint32_t pad2;
};

struct AdaptStore {          // the context's read store as the scan reads it
  const uint32_t* d_p0;         // low code bit of base 32 w + i = bit i of word w
  const uint32_t* d_p1;         // high code bit
  const uint64_t* d_word_off;   // [n_reads + 1] first word of a read
  const uint64_t* d_base_off;   // [n_reads + 1] first base of a read (its length by difference)
  const uint32_t* h_len;        // host: read lengths
  uint32_t n_reads;
};

// ---- the recurrence (host and device: the kernels are these two functions behind an index computation) -------------------------------------
// W: the column's word — uint64_t for every pattern, uint32_t for one of at most 32 bases (half the instructions; the kernel picks per pattern).
// one code bit as a mask of W, 0 or all ones: one 32-bit negation serves both halves (a 64-bit one is a subtract with borrow per base)
template <class W>
__host__ __device__ inline W adapt_spread(uint32_t bit) {
  const uint32_t x = 0u - bit;
  if constexpr (sizeof(W) == 8) return (uint64_t)x << 32 | x;
  else return x;
}

// One text base through Myers' column: Eq = the pattern positions the base matches, Pv / Mv = the +1 / -1 vertical differences, top = m - 1 the
// bottom row's bit.  Returns the change of the bottom cell (the score).  ANCHORED: the horizontal input of row 0 is +1 (an alignment that must
// begin at the text's first base: k_adapt_start), otherwise 0 (it may begin anywhere: the search).
template <bool ANCHORED, class W>
__host__ __device__ inline int adapt_step(W Eq, W& Pv, W& Mv, uint32_t top) {
  const W Xv = Eq | Mv;
  const W Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
  W Ph = Mv | ~(Xh | Pv);
  W Mh = Pv & Xh;
  uint32_t ph, mh;   // the word that holds the bottom row (a 64-bit shift by a variable is dearer than a select)
  if constexpr (sizeof(W) == 8) { ph = top >= 32 ? (uint32_t)(Ph >> 32) : (uint32_t)Ph; mh = top >= 32 ? (uint32_t)(Mh >> 32) : (uint32_t)Mh; }
  else { ph = Ph; mh = Mh; }
  const int d = (int)((ph >> (top & 31u)) & 1u) - (int)((mh >> (top & 31u)) & 1u);
  Ph = (Ph << 1) | (W)(ANCHORED ? 1 : 0);
  Mh <<= 1;
  Pv = Mh | ~(Xv | Ph);
  Mv = Ph & Xv;
  return d;
}

// The lane that owns the end positions (seg_lo, seg_hi] of a read of len bases (p0 / p1: the read's first plane words; seg_lo < seg_hi <= len), for
// one pattern.  It starts from the initial column at the word boundary at or below seg_lo - (m + k): an alignment of at most k errors spans at most
// m + k text bases and a later start can only raise E, so min(E, k + 1) is exact from seg_lo on.  emit(end, errors) for every run whose first
// position lies in (seg_lo, seg_hi]; the lane follows such a run past seg_hi until it ends, and leaves a run that is already open at seg_lo to
// the lane before it.
template <class W, class Emit>
__host__ __device__ inline void adapt_scan_lane(const uint32_t* __restrict__ p0, const uint32_t* __restrict__ p1, uint32_t len, uint32_t seg_lo,
                                                uint32_t seg_hi, W n0, W n1, uint32_t m, uint32_t k, Emit&& emit) {
  const uint32_t back = m + k;
  uint32_t t = (seg_lo > back ? seg_lo - back : 0u) & ~31u;
  W Pv = ~(W)0, Mv = 0;
  uint32_t score = m, best = 0, best_j = 0;
  bool in_run = false, own = false;
  for (;;) {
    uint32_t w0 = p0[t >> 5], w1 = p1[t >> 5];
    const uint32_t nb = len - t < 32u ? len - t : 32u;
    for (uint32_t b = 0; b < nb; b++) {
      const W B0 = adapt_spread<W>(w0 & 1u), B1 = adapt_spread<W>(w1 & 1u);
      w0 >>= 1; w1 >>= 1;
      score += adapt_step<false, W>((n0 ^ B0) & (n1 ^ B1), Pv, Mv, m - 1);
      const uint32_t j = t + b + 1;
      if (score <= k) {
        if (!in_run) { in_run = true; own = j > seg_lo && j <= seg_hi; best = score; best_j = j; }
        else if (score < best) { best = score; best_j = j; }
      } else if (in_run) {
        if (own) emit(best_j, best);
        in_run = false; own = false;
      }
    }
    t += 32;
    if (t >= len || (t >= seg_hi && !(in_run && own))) break;   // (a run that begins behind seg_hi is the next lane's)
  }
  if (in_run && own) emit(best_j, best);
}

// start of the hit of errors `errors` that ends at `end`: the reversed pattern (r0 / r1) over the text read downwards from end - 1, anchored at
// end; the first length at which the bottom cell equals errors is the shortest one, i.e. the largest start.  At most m + k bases.
__host__ __device__ inline uint32_t adapt_start_of(const uint32_t* __restrict__ p0, const uint32_t* __restrict__ p1, uint32_t end, uint32_t errors,
                                                   uint64_t r0, uint64_t r1, uint32_t m, uint32_t k) {
  const uint32_t L = end < m + k ? end : m + k;
  uint64_t Pv = ~0ull, Mv = 0;
  uint32_t score = m;
  for (uint32_t l = 1; l <= L; l++) {
    const uint32_t pos = end - l;
    const uint64_t B0 = adapt_spread<uint64_t>((p0[pos >> 5] >> (pos & 31u)) & 1u), B1 = adapt_spread<uint64_t>((p1[pos >> 5] >> (pos & 31u)) & 1u);
    score += adapt_step<true, uint64_t>((r0 ^ B0) & (r1 ^ B1), Pv, Mv, m - 1);
    if (score == errors) return pos;
  }
  return end;   // (not reached for a hit of the scan: some start within m + k bases of end gives its errors)
}

struct AdaptStats { uint64_t seg = 0, segments = 0, hits = 0, scans = 0; double scan_ms = 0, start_ms = 0; };

enum { ADAPT_OK = 0, ADAPT_HIP = 1, ADAPT_UNSUPPORTED = 2 };

// Every hit of every pattern in every read, complete (start included), in NO particular order: the caller sorts by the specification's key, which
// is unique per hit.  seg: bases per lane.  cap0: hits the buffer of the first scan holds (0: max(65536, segments / 8)); a scan that counts more
// is run again at the counted size.  Queued on st; returns when the hits are on the host.
int adapt_find(const AdaptStore& S, const std::vector<AdaptPattern>& pats, uint32_t seg, uint64_t cap0, hipStream_t st, std::vector<herro_adapter_hit>& out,
               AdaptStats& stats, std::string& err);

}  // namespace herro
