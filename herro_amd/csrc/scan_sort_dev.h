// scan_sort_dev.h — the two device primitives every stage of the front end stands on (scan_sort_dev.hip): the exclusive scan of u32 and the
// stable LSD radix sort of 64-bit keys with 64-bit payloads.  Clients: the overlap finder (overlap_dev.hip, overlap_rows.hip), cluster_dev.hip's
// arcs and order, fasta_dev.hip's prefixes, paf_dev.hip's line offsets (frontend_api.hip), and the test hooks herro_debug_scan_u32 /
// herro_debug_radix_sort (tests/scan_sort_cases.py).  Everything is queued on the caller's stream; nothing is awaited.  The functions return 0, or 1
// with err set — the values of OVL_OK / OVL_HIP (overlap_dev.h), whose code this was.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "dev_bufs.h"

namespace herro {

constexpr int SC_ITEMS = 8;                  // scan / sort: items per thread, 256 threads
constexpr uint32_t SC_TILE = 256 * SC_ITEMS;

inline uint32_t nblk(uint64_t n, uint32_t per = 256) { return (uint32_t)((n + per - 1) / per); }
inline uint32_t bits_of(uint64_t v) { uint32_t b = 0; while (v) { b++; v >>= 1; } return b; }   // bits to hold 0 .. v
// the 8-bit digits of a key field of nbits bits from bit lo on, appended in ascending significance (the last one may be partial)
inline void field_shifts(std::vector<uint32_t>& v, uint32_t lo, uint32_t nbits) { for (uint32_t s = lo; s < lo + nbits; s += 8) v.push_back(s); }

// ---- block helpers (256 threads = 4 waves) ------------------------------------------------------------------------------------
__device__ inline uint32_t block_excl_scan(uint32_t v, uint32_t* lds4, uint32_t& total) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(inc, o, 64);
    if ((int)lane >= o) inc += t;
  }
  if (lane == 63) lds4[wave] = inc;
  __syncthreads();
  uint32_t base = 0;
  total = 0;
#pragma unroll
  for (uint32_t i = 0; i < 4; i++) {
    const uint32_t c = lds4[i];
    if (i < wave) base += c;
    total += c;
  }
  __syncthreads();
  return base + inc - v;
}

// Exclusive scan of in[0 .. n) into out[0 .. n], out[n] = the total (k_scan_partial / k_scan_top / k_scan_final); partial: dev_scan_partials(n)
// entries of scratch.
uint32_t dev_scan_partials(uint32_t n);
int dev_scan_u32(const uint32_t* in, uint32_t n, uint32_t* out, uint32_t* partial, hipStream_t st, std::string& err);

// The sort's scratch for up to `cap` elements: three arrays of u32, as three allocations (alloc) or laid out in one block of dev_sort_scratch(cap)
// entries (in_block).  `partial` serves the scan of the histogram and is large enough for a client's scans of per-element arrays.
struct SortScratch {
  uint32_t* hist = nullptr;     // 256 x blocks
  uint32_t* offs = nullptr;     // + 1
  uint32_t* partial = nullptr;
  struct Sizes { uint64_t hist, offs, partial; };
  static Sizes sizes(uint64_t cap) {
    const uint64_t nb = nblk(cap, SC_TILE) + 1;
    return {256 * nb, 256 * nb + 1, std::max<uint64_t>(nblk(256 * nb, SC_TILE), nb) + 2};   // scans of the histogram and of per-element arrays
  }
  hipError_t alloc(Bufs& B, uint64_t cap) {
    const Sizes z = sizes(cap);
    hipError_t e;
    if ((e = B.get(&hist, z.hist)) != hipSuccess) return e;
    if ((e = B.get(&offs, z.offs)) != hipSuccess) return e;
    return B.get(&partial, z.partial);
  }
  void in_block(uint32_t* scratch, uint64_t cap) {
    const Sizes z = sizes(cap);
    hist = scratch;
    offs = scratch + z.hist;
    partial = scratch + z.hist + z.offs;
  }
};
inline uint64_t dev_sort_scratch(uint64_t n) { const SortScratch::Sizes z = SortScratch::sizes(n); return z.hist + z.offs + z.partial; }

// Stable LSD sort (k_rs_hist / k_rs_scatter over dev_scan_u32) of n 64-bit keys with their 64-bit payloads, one 8-bit digit per entry of `shifts`
// in ascending significance.  The sorted arrays end up in (*k0, *p0): the pointers are swapped after every pass.  scratch: dev_sort_scratch(n)
// entries of u32.
int dev_radix_sort(uint64_t** k0, uint64_t** p0, uint64_t** k1, uint64_t** p1, uint32_t n, const std::vector<uint32_t>& shifts, const SortScratch& S,
                   hipStream_t st, std::string& err);
inline int dev_radix_sort(uint64_t** k0, uint64_t** p0, uint64_t** k1, uint64_t** p1, uint32_t n, const std::vector<uint32_t>& shifts,
                          uint32_t* scratch, hipStream_t st, std::string& err) {
  SortScratch S;
  S.in_block(scratch, n);
  return dev_radix_sort(k0, p0, k1, p1, n, shifts, S, st, err);
}

}  // namespace herro
