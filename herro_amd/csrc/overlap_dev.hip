// overlap_dev.hip — minimizer seeding and chaining on the read store (overlap_dev.h; specification: DESIGN.md §10,
// tests/overlap_ref.py).  Stages:
//   k_sketch     a block per 256 k-mers of one read: f / r / hash per k-mer, window minima in LDS, every k-mer equal to the
//                minimum of a window it lies in is selected.  Run twice: count per tile, scan, write — so the output is in
//                (rid, pos) order without any atomic deciding a place.
//   radix sort   by hash, stable: the shared sort and scan of scan_sort_dev.h (dev_radix_sort, dev_scan_u32), as every sort and prefix below.
//   k_occ_census, k_occ_pick   occ_frac_ppm only: the histogram of the run lengths (LDS bins below 2048, the table beyond) and, in one workgroup, the
//                cut that leaves the given fraction of the distinct hashes above it; k_runs_occ reads it where k_occ_pick left it.
//   k_occ_place, k_rescue, k_resc_kind   the rescue of high-frequency minimizers only (OvlParams.occ_dist != 0): the run length of every minimizer put back
//                in (rid, pos) order, one wave64 per read over its streaks of minimizers above the cut, and the outcome back in hash order for
//                k_runs_resc / k_expand_resc (tests/rescue_ref.py).
//   k_runs       per hash run: length, frequency cut, anchors every occurrence has with the later reads of its run.
//   k_expand     the anchors of the targets of one chunk: A = tpos << 32 | qpos, B = (t - t_lo) << 33 | q << 1 | rel;
//                sorted by A carrying B, then by B carrying A (stable): order (t, q, rel, tpos, qpos).
//   k_chain      one wave64 per (t, q, rel) group: the 64 predecessors of an anchor are the 64 lanes.
//   k_chain_far  OvlParams.lookback = 64 R > 64 only: k_chain with R rounds a step, the R blocks in front of the current one in an LDS ring.
//   k_walk       back through the stored predecessors: first anchor, anchor count, coordinates.
//   k_sketch_part, k_occ16, k_part_cls, k_part_gather, k_part_runs, k_part_expand   OvlParams.index_kmers != 0 only (herro_set_index_params): the
//                occurrences of every minimizer's hash by hash range (the pick over 64-bit bins: k_occ_pick again), then the stages above per pair
//                of read blocks, a hash run judged by those occurrences ("an index in parts", below); host side: part_index, find_parts.
// The row table and the final order of the records of an index in parts are overlap_rows.hip.
// A core mask (one byte per read, non-zero: the read is a target) keeps k_runs / k_expand from creating an anchor between two non-core
// reads, so everything behind the anchors sees wanted pairs only; without a mask (CORE = false) the two kernels are what they were.
// Nothing an atomic orders reaches the output: the only atomics are integer sums (histograms, anchors per read).
#include "overlap_dev.h"
#include "index_plan.h"
#include "scan_sort_dev.h"

#include <algorithm>
#include <climits>
#include <type_traits>

namespace herro {
namespace {

constexpr uint64_t INF64 = 0xffffffffffffffffull;
constexpr int SK_T = 256;                    // k-mers (threads) of a sketch tile
constexpr int SK_H = SK_T + 2 * 63 + 2;      // hashes a tile needs: w - 1 <= 63 on either side

// ---- sketch -----------------------------------------------------------------------------------------------------------------
__device__ inline uint64_t hash64(uint64_t x, uint64_t m) {   // minimap2's invertible mix on 2k bits
  x = (~x + (x << 21)) & m;
  x ^= x >> 24;
  x = (x + (x << 3) + (x << 8)) & m;
  x ^= x >> 14;
  x = (x + (x << 2) + (x << 4)) & m;
  x ^= x >> 28;
  x = (x + (x << 31)) & m;
  return x;
}

// hash and strand of the k-mer that starts at base p of the read whose first word is w0
__device__ inline uint64_t kmer_hash(const uint64_t* __restrict__ words, uint64_t w0, uint32_t p, uint32_t k, uint64_t mask, uint32_t& strand) {
  const uint64_t wi = w0 + (p >> 5);
  const uint32_t sh = (p & 31u) * 2u;
  uint64_t v = words[wi] >> sh;
  if (sh + 2u * k > 64u) v |= words[wi + 1] << (64u - sh);   // (sh > 0 here)
  v &= mask;                                 // base p + i at bits 2i: this is the reverse complement's value once complemented
  const uint64_t r = ~v & mask;
  uint64_t x = __brevll(v);                  // base order reversed; the two bits of a base swapped back below
  x = ((x & 0x5555555555555555ull) << 1) | ((x >> 1) & 0x5555555555555555ull);
  const uint64_t f = x >> (64u - 2u * k);    // first base most significant
  strand = r < f ? 1u : 0u;
  if (f == r) return INF64;
  return hash64(f < r ? f : r, mask);
}

// The front of a sketch tile: block b of the store's tiles is 256 k-mers of one read among r_lo .. r_hi - 1 (tile_off[r]: first tile of read r;
// reads shorter than k + w - 1 have none).  Leaves the hashes the tile needs in sh, their strands in ss and the window minima in wm, all indexed
// from k-mer lo of the read on, and for the thread's own k-mer j its hash hj and sel: it equals the minimum of a window it lies in.
struct SketchTile { uint32_t rid, j, lo; uint64_t hj; bool sel; };
__device__ __forceinline__ SketchTile sketch_tile(const uint64_t* __restrict__ words, const uint64_t* __restrict__ word_off,
                                                  const uint64_t* __restrict__ base_off, const uint32_t* __restrict__ tile_off, uint32_t r_lo,
                                                  uint32_t r_hi, uint32_t b, uint32_t k, uint32_t w, uint64_t* sh, uint64_t* wm, uint8_t* ss) {
  const uint32_t tid = threadIdx.x;
  uint32_t lo_r = r_lo, hi_r = r_hi;          // largest r with tile_off[r] <= b
  while (hi_r - lo_r > 1) {
    const uint32_t mid = (lo_r + hi_r) >> 1;  // (no more than OVL_MAX_READS = 2^31 - 1 reads: the sum fits)
    if (tile_off[mid] <= b) lo_r = mid; else hi_r = mid;
  }
  const uint32_t rid = lo_r;
  const uint32_t len = (uint32_t)(base_off[rid + 1] - base_off[rid]);
  const uint32_t nk = len - k + 1;            // >= w (the read has tiles)
  const uint32_t base = (b - tile_off[rid]) * SK_T;
  const uint64_t w0 = word_off[rid];
  const uint64_t mask = (1ull << (2 * k)) - 1;
  const uint32_t lo = base >= w - 1 ? base - (w - 1) : 0u;
  const uint32_t hi = min(nk, base + SK_T + (w - 1));
  for (uint32_t i = lo + tid; i < hi; i += SK_T) {
    uint32_t s;
    sh[i - lo] = kmer_hash(words, w0, i, k, mask, s);
    ss[i - lo] = (uint8_t)s;
  }
  __syncthreads();
  const uint32_t s_hi = min(nk - w, base + SK_T - 1);   // last window start any k-mer of the tile lies in
  for (uint32_t s = lo + tid; s <= s_hi; s += SK_T) {
    uint64_t m = INF64;
    for (uint32_t o = 0; o < w; o++) { const uint64_t v = sh[s - lo + o]; m = v < m ? v : m; }
    wm[s - lo] = m;
  }
  __syncthreads();
  const uint32_t j = base + tid;
  bool sel = false;
  uint64_t hj = INF64;
  if (j < nk) {
    hj = sh[j - lo];
    if (hj != INF64) {
      const uint32_t s0 = j >= w - 1 ? j - (w - 1) : 0u, s1 = min(j, nk - w);
      for (uint32_t s = s0; s <= s1; s++) sel |= wm[s - lo] == hj;
    }
  }
  return SketchTile{rid, j, lo, hj, sel};
}

__global__ __launch_bounds__(SK_T) void k_sketch(const uint64_t* __restrict__ words, const uint64_t* __restrict__ word_off,
                                                 const uint64_t* __restrict__ base_off, const uint32_t* __restrict__ tile_off,
                                                 uint32_t n_reads, uint32_t k, uint32_t w, uint32_t* __restrict__ tile_cnt,
                                                 const uint32_t* __restrict__ tile_at, uint64_t* __restrict__ hash_out,
                                                 uint64_t* __restrict__ meta_out, int write) {
  __shared__ uint64_t sh[SK_H];
  __shared__ uint64_t wm[SK_H];
  __shared__ uint8_t ss[SK_H];
  __shared__ uint32_t wc[4];
  const uint32_t b = blockIdx.x, tid = threadIdx.x;
  const SketchTile t = sketch_tile(words, word_off, base_off, tile_off, 0, n_reads, b, k, w, sh, wm, ss);
  const uint64_t bal = __ballot(t.sel);
  const uint32_t lane = tid & 63, wave = tid >> 6;
  if (lane == 0) wc[wave] = (uint32_t)__popcll(bal);
  __syncthreads();
  uint32_t before = 0, total = 0;
  for (uint32_t i = 0; i < 4; i++) { if (i < wave) before += wc[i]; total += wc[i]; }
  if (!write) {
    if (tid == 0) tile_cnt[b] = total;
    return;
  }
  if (t.sel) {
    const uint32_t at = tile_at[b] + before + (uint32_t)__popcll(bal & ((1ull << lane) - 1));
    hash_out[at] = t.hj;
    meta_out[at] = ((uint64_t)t.rid << 32) | ((uint64_t)(t.j + k - 1) << 1) | ss[t.j - t.lo];
  }
}

// ---- runs of one hash, frequency cut, anchors per occurrence --------------------------------------------------------------
// cnt[x]: anchors occurrence x has as the target side = occurrences behind it in its run that lie in another (later) read;
// run_end[x]: end of its run.  Runs longer than max_occ (and single occurrences) keep cnt 0 (cleared before the launch).
// CORE: an occurrence in a non-core read counts only the later occurrences whose read is core — none of them is in its own read, which is
// not core.  An occurrence in a core read keeps the count above.  The frequency cut is the whole store's, whatever the mask.
// RESCUE ("Rescue of high-frequency minimizers"): a run with max_occ < c <= rmax is kept for its rescued occurrences.  kind[x]
// (k_resc_kind): 0 — x is in no such run, 1 — it is and is not rescued, 2 — it is rescued.  A rescued occurrence counts every later occurrence in
// another read, one that is not rescued counts the rescued ones; the core rule holds on top.  stat[2] sums the anchors of these runs.
template <bool CORE, bool RESCUE = false>
__device__ inline void runs_of_head(const uint64_t* __restrict__ hash, const uint64_t* __restrict__ meta, uint32_t n, uint32_t max_occ,
                                    uint32_t* __restrict__ cnt, uint32_t* __restrict__ run_end, unsigned long long* __restrict__ per_read,
                                    const uint8_t* __restrict__ core, uint32_t rmax = 0, const uint8_t* __restrict__ kind = nullptr,
                                    unsigned long long* __restrict__ stat = nullptr) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t h = hash[i];
  if (i > 0 && hash[i - 1] == h) return;       // the head of a run does the run
  uint32_t bound = max_occ;
  if constexpr (RESCUE) bound = max(max_occ, rmax);
  uint64_t e = i + 1;
  while (e < n && hash[e] == h && e - i <= bound) e++;
  const uint64_t c = e - i;
  if (c < 2 || c > bound) return;
  if constexpr (RESCUE) {
    if (c > max_occ) {
      // behind j: a = all occurrences, r = the rescued, c = those of core reads, cr = both; s*: the same of j's own read, which do not count
      uint32_t ta = 0, tr = 0, tc = 0, tcr = 0, sa = 0, sr = 0, sc = 0, scr = 0, rid_after = 0xffffffffu;
      unsigned long long sum = 0;
      for (uint64_t j = e; j-- > i;) {
        const uint32_t rid = (uint32_t)(meta[j] >> 32);
        if (rid != rid_after) sa = sr = sc = scr = 0;
        rid_after = rid;
        const bool resc = kind[j] == 2;
        bool is_core = true;
        if constexpr (CORE) is_core = core[rid] != 0;
        const uint32_t m = is_core ? (resc ? ta - sa : tr - sr) : (resc ? tc - sc : tcr - scr);
        cnt[j] = m;
        run_end[j] = (uint32_t)e;
        if (m) atomicAdd(&per_read[rid], (unsigned long long)m);
        sum += m;
        ta++; sa++;
        if (resc) { tr++; sr++; }
        if (is_core) { tc++; sc++; if (resc) { tcr++; scr++; } }
      }
      if (sum) atomicAdd(&stat[2], sum);
      return;
    }
  }
  uint64_t nxt = e;                            // first occurrence of the next read
  uint32_t rid_after = 0;
  uint32_t core_after = 0;                     // CORE: occurrences behind j whose read is core
  for (uint64_t j = e; j-- > i;) {
    const uint32_t rid = (uint32_t)(meta[j] >> 32);
    if (j + 1 < e && rid != rid_after) nxt = j + 1;
    rid_after = rid;
    uint32_t m = (uint32_t)(e - nxt);
    if constexpr (CORE) {
      const bool is_core = core[rid] != 0;
      if (!is_core) m = core_after;
      core_after += is_core ? 1u : 0u;
    }
    cnt[j] = m;
    run_end[j] = (uint32_t)e;
    if (m) atomicAdd(&per_read[rid], (unsigned long long)m);
  }
}

template <bool CORE>
__global__ __launch_bounds__(256) void k_runs(const uint64_t* __restrict__ hash, const uint64_t* __restrict__ meta, uint32_t n,
                                              uint32_t max_occ, uint32_t* __restrict__ cnt, uint32_t* __restrict__ run_end,
                                              unsigned long long* __restrict__ per_read, const uint8_t* __restrict__ core) {
  runs_of_head<CORE>(hash, meta, n, max_occ, cnt, run_end, per_read, core);
}

// ... with the cut k_occ_pick left in occ[0] (at most 65534: the walk to the end of a run stays bounded)
template <bool CORE>
__global__ __launch_bounds__(256) void k_runs_occ(const uint64_t* __restrict__ hash, const uint64_t* __restrict__ meta, uint32_t n,
                                                  const uint64_t* __restrict__ occ, uint32_t* __restrict__ cnt, uint32_t* __restrict__ run_end,
                                                  unsigned long long* __restrict__ per_read, const uint8_t* __restrict__ core) {
  runs_of_head<CORE>(hash, meta, n, (uint32_t)occ[0], cnt, run_end, per_read, core);
}

// ... with the rescue on; occ: where k_occ_pick left the cut, or NULL — the cut is max_occ
template <bool CORE>
__global__ __launch_bounds__(256) void k_runs_resc(const uint64_t* __restrict__ hash, const uint64_t* __restrict__ meta, uint32_t n, uint32_t max_occ,
                                                   const uint64_t* __restrict__ occ, uint32_t* __restrict__ cnt, uint32_t* __restrict__ run_end,
                                                   unsigned long long* __restrict__ per_read, const uint8_t* __restrict__ core, uint32_t rmax,
                                                   const uint8_t* __restrict__ kind, unsigned long long* __restrict__ stat) {
  runs_of_head<CORE, true>(hash, meta, n, occ ? (uint32_t)occ[0] : max_occ, cnt, run_end, per_read, core, rmax, kind, stat);
}

// ---- the cut as a fraction of the distinct hashes (occ_frac_ppm; DESIGN.md section 10, tests/occ_ref.py) -------------------------------------
constexpr uint32_t OCC_LDS_BINS = 2048;      // bins of the census a block keeps in LDS (8 KB); a longer run is rare and goes to the table itself
constexpr uint32_t OCC_GRID = 1024;          // blocks of the census at most: each flushes its LDS bins once

// the floor, the caller's ceiling (0: none), and never the last bin, whose runs have no known length
__host__ __device__ inline uint32_t occ_final_cut(uint32_t q, uint32_t max_occ) {
  uint32_t cut = q > OVL_OCC_FLOOR ? q : OVL_OCC_FLOOR;
  if (max_occ && cut > max_occ) cut = max_occ;
  return cut < OVL_OCC_BINS - 2 ? cut : OVL_OCC_BINS - 2;
}

// The census's bins: a block counts the runs of fewer than OCC_LDS_BINS members in LDS (h) and adds them to the table (hist, u32 or 64-bit bins)
// once, at its end; a longer run goes to the table itself.  256 threads.
__device__ inline void occ_bins_clear(uint32_t* h) {
  for (uint32_t b = threadIdx.x; b < OCC_LDS_BINS; b += 256) h[b] = 0;
  __syncthreads();
}
template <class Bin>
__device__ inline void occ_bins_add(uint32_t* h, Bin* __restrict__ hist, uint32_t c) {
  if (c < OCC_LDS_BINS) atomicAdd(&h[c], 1u);
  else atomicAdd(&hist[c], (Bin)1);
}
template <class Bin>
__device__ inline void occ_bins_flush(const uint32_t* h, Bin* __restrict__ hist) {
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < OCC_LDS_BINS; b += 256)
    if (h[b]) atomicAdd(&hist[b], (Bin)h[b]);
}

// hist[min(length, 65535)] += 1 for every hash run.  rstart[r]: first minimizer of run r (run_starts), rstart[*n_runs] = n: a run's length is a
// difference, no thread walks a run.
__global__ __launch_bounds__(256) void k_occ_census(const uint32_t* __restrict__ rstart, const uint32_t* __restrict__ n_runs,
                                                    uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[OCC_LDS_BINS];
  occ_bins_clear(h);
  const uint32_t nr = *n_runs;
  for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < nr; r += (uint64_t)gridDim.x * 256)
    occ_bins_add(h, hist, min(rstart[r + 1] - rstart[r], OVL_OCC_BINS - 1));
  occ_bins_flush(h, hist);
}

// One workgroup.  Thread t owns the 256 bins from 256 (255 - t) on, so `above`, the sum over the threads in front, is the runs in all higher bins.
// q = the least v with no more than drop runs above it; occ = {cut, distinct, runs above the cut, minimizers in them}; n: the store's minimizers.
// Bin: uint32_t (k_occ_census) or 64 bits (k_occ16: the singletons of a large store exceed 2^32); the sums are 64-bit for both.
template <class Bin>
__global__ __launch_bounds__(256) void k_occ_pick(const Bin* __restrict__ hist, uint64_t n, uint32_t ppm, uint32_t max_occ, uint64_t* __restrict__ occ) {
  __shared__ unsigned long long sums[256];
  __shared__ uint32_t s_q;
  __shared__ unsigned long long s_runs, s_kept;
  const uint32_t b0 = 256u * (255u - threadIdx.x);
  if (threadIdx.x == 0) { s_q = OVL_OCC_BINS - 1; s_runs = 0; s_kept = 0; }
  uint64_t s = 0;
  for (uint32_t b = 0; b < 256; b++) s += hist[b0 + b];
  sums[threadIdx.x] = s;
  __syncthreads();
  uint64_t above = 0, distinct = 0;             // above: the runs in all higher bins (the threads in front own them)
  for (uint32_t t = 0; t < 256; t++) { const uint64_t v = sums[t]; if (t < threadIdx.x) above += v; distinct += v; }
  const uint64_t drop = distinct * ppm / 1000000u;
  uint32_t q = OVL_OCC_BINS;
  for (uint32_t b = 256; b-- > 0 && above <= drop;) {
    q = b0 + b;
    above += hist[b0 + b];
  }
  if (q < OVL_OCC_BINS) atomicMin(&s_q, q);
  __syncthreads();
  const uint32_t cut = occ_final_cut(s_q, max_occ);
  uint64_t runs = 0, kept = 0;                   // kept: minimizers in runs of at most cut (<= 65534: the bin is the length)
  for (uint32_t b = 0; b < 256; b++) {
    const uint32_t v = b0 + b;
    const uint64_t c = hist[v];
    if (v > cut) runs += c; else kept += (uint64_t)v * c;
  }
  if (runs) atomicAdd(&s_runs, (unsigned long long)runs);
  if (kept) atomicAdd(&s_kept, (unsigned long long)kept);
  __syncthreads();
  if (threadIdx.x == 0) { occ[0] = cut; occ[1] = distinct; occ[2] = s_runs; occ[3] = n - s_kept; }
}

__global__ __launch_bounds__(256) void k_mask(const uint64_t* __restrict__ meta, const uint32_t* __restrict__ cnt, uint32_t n,
                                              uint32_t t_lo, uint32_t t_hi, uint32_t* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t rid = (uint32_t)(meta[i] >> 32);
  out[i] = rid >= t_lo && rid < t_hi ? cnt[i] : 0u;
}

// CORE: a non-core occurrence has its cntm[x] partners scattered over the rest of its run — the occurrences of core reads; it walks the
// run from itself on (at most max_occ steps) and skips the others, those of its own read among them.
// RESCUE: an occurrence of a rescued run that is not rescued itself (kind 1) has the rescued occurrences of the other reads behind it as partners,
// scattered likewise; the walk is bounded by the run's end, at most rescue_max_occ steps.
template <bool CORE, bool RESCUE>
__device__ inline void expand_one(const uint64_t* __restrict__ meta, const uint32_t* __restrict__ cntm, const uint32_t* __restrict__ run_end,
                                  const uint32_t* __restrict__ aoff, uint32_t n, const uint64_t* __restrict__ base_off, uint32_t k, uint32_t t_lo,
                                  uint64_t* __restrict__ A, uint64_t* __restrict__ B, const uint8_t* __restrict__ core,
                                  const uint8_t* __restrict__ kind) {
  const uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (x >= n) return;
  const uint32_t c = cntm[x];
  if (!c) return;
  const uint64_t mx = meta[x];
  const uint32_t t = (uint32_t)(mx >> 32), tpos = ((uint32_t)mx) >> 1, st = (uint32_t)mx & 1u;
  const uint32_t e = run_end[x];
  uint32_t at = aoff[x];
  bool sparse = false;
  if constexpr (CORE) sparse = core[t] == 0;
  bool rsparse = false;
  if constexpr (RESCUE) rsparse = kind[x] == 1;
  const uint32_t at_end = at + c;
  for (uint32_t y = sparse || rsparse ? (uint32_t)x + 1 : e - c; y < e; y++) {
    const uint64_t my = meta[y];
    const uint32_t q = (uint32_t)(my >> 32), qp = ((uint32_t)my) >> 1, rel = ((uint32_t)my & 1u) ^ st;
    if constexpr (CORE || RESCUE) {
      if (at == at_end) break;                              // (its c partners are written: nothing behind them is core)
    }
    if constexpr (CORE) {
      if (sparse && core[q] == 0) continue;
    }
    if constexpr (RESCUE) {
      if (rsparse && (q == t || kind[y] != 2)) continue;
    }
    const uint32_t qlen = (uint32_t)(base_off[q + 1] - base_off[q]);
    const uint32_t qpos = rel ? qlen - qp + k - 2 : qp;     // last base of the same k-mer on the query's reverse complement
    A[at] = ((uint64_t)tpos << 32) | qpos;
    B[at] = ((uint64_t)(t - t_lo) << 33) | ((uint64_t)q << 1) | rel;
    at++;
  }
}

template <bool CORE>
__global__ __launch_bounds__(256) void k_expand(const uint64_t* __restrict__ meta, const uint32_t* __restrict__ cntm,
                                                const uint32_t* __restrict__ run_end, const uint32_t* __restrict__ aoff, uint32_t n,
                                                const uint64_t* __restrict__ base_off, uint32_t k, uint32_t t_lo,
                                                uint64_t* __restrict__ A, uint64_t* __restrict__ B, const uint8_t* __restrict__ core) {
  expand_one<CORE, false>(meta, cntm, run_end, aoff, n, base_off, k, t_lo, A, B, core, nullptr);
}

template <bool CORE>
__global__ __launch_bounds__(256) void k_expand_resc(const uint64_t* __restrict__ meta, const uint32_t* __restrict__ cntm,
                                                     const uint32_t* __restrict__ run_end, const uint32_t* __restrict__ aoff, uint32_t n,
                                                     const uint64_t* __restrict__ base_off, uint32_t k, uint32_t t_lo,
                                                     uint64_t* __restrict__ A, uint64_t* __restrict__ B, const uint8_t* __restrict__ core,
                                                     const uint8_t* __restrict__ kind) {
  expand_one<CORE, true>(meta, cntm, run_end, aoff, n, base_off, k, t_lo, A, B, core, kind);
}

// ---- rescue of high-frequency minimizers (tests/rescue_ref.py) ------------------------------------------------------------
// first p with a[p] >= v
__device__ inline uint32_t lower_bound_u64(const uint64_t* __restrict__ a, uint32_t n, uint64_t v) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// From hash order back to (rid, pos) order: meta ascends with (rid, pos) and is unique, so the place of sorted element i is its rank in the
// unsorted copy meta_rp.  occ_rp[place] = the length of i's run (a difference of run starts: run_starts), perm[i] = place.
__global__ __launch_bounds__(256) void k_occ_place(const uint64_t* __restrict__ meta, const uint64_t* __restrict__ meta_rp,
                                                   const uint32_t* __restrict__ flag, const uint32_t* __restrict__ gidx,
                                                   const uint32_t* __restrict__ rstart, uint32_t n, uint32_t* __restrict__ occ_rp,
                                                   uint32_t* __restrict__ perm) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t r = gidx[i] + flag[i] - 1;
  const uint32_t p = lower_bound_u64(meta_rp, n, meta[i]);
  occ_rp[p] = rstart[r + 1] - rstart[r];
  perm[i] = p;
}

// One streak: the H minimizers (cut < occ <= rmax) of [s0, s1) in (rid, pos) order, `size` of them, no U among them; ps / pe: the positions that
// bound it.  Every argument is uniform over the wave.  Flags the m = (2 (pe - ps) + occ_dist) / (2 occ_dist) members with the least (occ, pos) —
// all of them if m >= size — and returns how many it flagged.  T, the m-th smallest occ, is found by bisection over the value, a ballot count
// per 64 members and step; then every occ < T is flagged and the first m - #(occ < T) of occ == T in position order.
__device__ inline uint32_t rescue_streak(const uint32_t* __restrict__ occ_rp, uint8_t* __restrict__ resc_rp, uint32_t s0, uint32_t s1,
                                         uint32_t size, uint32_t ps, uint32_t pe, uint32_t cut, uint32_t rmax, uint32_t occ_dist, uint32_t lane) {
  const uint64_t m64 = (2ull * (pe - ps) + occ_dist) / (2ull * occ_dist);
  if (!m64) return 0;
  uint32_t T = rmax, need = 0xffffffffu;
  if (m64 < size) {
    const uint32_t m = (uint32_t)m64;
    uint32_t lo = cut + 1, hi = rmax;          // the least T with #(cut < occ <= T) >= m
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      uint32_t le = 0;
      for (uint32_t b = s0; b < s1; b += 64) {
        const uint32_t c = b + lane < s1 ? occ_rp[b + lane] : 0u;
        le += (uint32_t)__popcll(__ballot(c > cut && c <= mid));
      }
      if (le >= m) hi = mid; else lo = mid + 1;
    }
    T = lo;
    uint32_t less = 0;
    for (uint32_t b = s0; b < s1; b += 64) {
      const uint32_t c = b + lane < s1 ? occ_rp[b + lane] : 0u;
      less += (uint32_t)__popcll(__ballot(c > cut && c < T));
    }
    need = m - less;
  }
  uint32_t taken = 0, flagged = 0;             // taken: members with occ == T in front of this block
  for (uint32_t b = s0; b < s1; b += 64) {
    const uint32_t c = b + lane < s1 ? occ_rp[b + lane] : 0u;
    const bool high = c > cut && c <= rmax, eq = high && c == T;
    const uint64_t beq = __ballot(eq);
    const bool f = high && (c < T || (eq && taken + (uint32_t)__popcll(beq & ((1ull << lane) - 1)) < need));
    if (f) resc_rp[b + lane] = 1;
    flagged += (uint32_t)__popcll(__ballot(f));
    taken += (uint32_t)__popcll(beq);
  }
  return flagged;
}

// One wave64 per read: its minimizers 64 at a time in ascending pos.  U = 2 <= occ <= cut, H = cut < occ <= rmax, the others are transparent.
// ps (the last U's pos, 0 at the start), the first member and the size of the open streak are uniform and carried from block to block; a U,
// or the read's end, closes the streak.  resc_rp is cleared before the launch; stat[0] += the H minimizers, stat[1] += the rescued.
__global__ __launch_bounds__(64) void k_rescue(const uint64_t* __restrict__ meta_rp, const uint32_t* __restrict__ occ_rp, uint32_t n,
                                               const uint64_t* __restrict__ base_off, uint32_t max_occ, const uint64_t* __restrict__ occ,
                                               uint32_t rmax, uint32_t occ_dist, uint8_t* __restrict__ resc_rp,
                                               unsigned long long* __restrict__ stat) {
  const uint32_t rid = blockIdx.x, lane = threadIdx.x;
  const uint32_t cut = occ ? (uint32_t)occ[0] : max_occ;
  if (rmax <= cut) return;
  const uint32_t r0 = lower_bound_u64(meta_rp, n, (uint64_t)rid << 32), r1 = lower_bound_u64(meta_rp, n, ((uint64_t)rid + 1) << 32);
  if (r0 == r1) return;
  const uint32_t len = (uint32_t)(base_off[rid + 1] - base_off[rid]);
  uint32_t ps = 0, s_begin = 0, s_size = 0, n_high = 0, n_resc = 0;
  for (uint32_t base = r0; base < r1; base += 64) {
    const bool valid = base + lane < r1;
    const uint32_t c = valid ? occ_rp[base + lane] : 0u;
    const uint32_t pos = valid ? ((uint32_t)meta_rp[base + lane]) >> 1 : 0u;
    const uint64_t mu = __ballot(c >= 2 && c <= cut), mh = __ballot(c > cut && c <= rmax);
    if (!mh && !s_size) {                       // no streak open, none begins: only the last U matters
      if (mu) ps = __shfl(pos, 63 - __clzll(mu), 64);
      continue;
    }
    n_high += (uint32_t)__popcll(mh);
    uint64_t rest = mu, seen = 0;               // seen: the lanes up to the last U handled
    while (rest) {
      const uint32_t l = (uint32_t)__builtin_ctzll(rest);
      rest &= rest - 1;
      const uint64_t hb = mh & ((1ull << l) - 1) & ~seen;
      if (hb) {
        if (!s_size) s_begin = base + (uint32_t)__builtin_ctzll(hb);
        s_size += (uint32_t)__popcll(hb);
      }
      const uint32_t pu = __shfl(pos, l, 64);
      if (s_size) {
        n_resc += rescue_streak(occ_rp, resc_rp, s_begin, base + l, s_size, ps, pu, cut, rmax, occ_dist, lane);
        s_size = 0;
      }
      ps = pu;
      seen = ((1ull << l) - 1) | (1ull << l);
    }
    const uint64_t hb = mh & ~seen;
    if (hb) {
      if (!s_size) s_begin = base + (uint32_t)__builtin_ctzll(hb);
      s_size += (uint32_t)__popcll(hb);
    }
  }
  if (s_size) n_resc += rescue_streak(occ_rp, resc_rp, s_begin, r1, s_size, ps, len, cut, rmax, occ_dist, lane);
  if (lane == 0) {
    if (n_high) atomicAdd(&stat[0], (unsigned long long)n_high);
    if (n_resc) atomicAdd(&stat[1], (unsigned long long)n_resc);
  }
}

// back in hash order: 0 — not in a rescued run, 1 — in one and not rescued, 2 — rescued
__global__ __launch_bounds__(256) void k_resc_kind(const uint32_t* __restrict__ perm, const uint32_t* __restrict__ occ_rp,
                                                   const uint8_t* __restrict__ resc_rp, uint32_t n, uint32_t max_occ,
                                                   const uint64_t* __restrict__ occ, uint32_t rmax, uint8_t* __restrict__ kind) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t cut = occ ? (uint32_t)occ[0] : max_occ;
  const uint32_t p = perm[i], c = occ_rp[p];
  kind[i] = c > cut && c <= rmax ? (resc_rp[p] ? 2 : 1) : 0;
}

// ---- groups -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_heads(const uint64_t* __restrict__ B, uint32_t n, uint32_t* __restrict__ flag) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) flag[i] = (i == 0 || B[i] != B[i - 1]) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_gstart(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ gidx, uint32_t n,
                                                uint32_t* __restrict__ gstart) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n && flag[i]) gstart[gidx[i]] = (uint32_t)i;
  if (i == 0) gstart[gidx[n]] = n;
}

__global__ __launch_bounds__(256) void k_gflag(const uint32_t* __restrict__ gstart, uint32_t ng, uint32_t min_anchors,
                                               uint32_t* __restrict__ gf) {
  const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (g < ng) gf[g] = gstart[g + 1] - gstart[g] >= min_anchors ? 1u : 0u;
}

// groups worth chaining, in group order: start, size; sort key = largest first, so that a launch does not end on one long group
__global__ __launch_bounds__(256) void k_gcompact(const uint32_t* __restrict__ gstart, const uint32_t* __restrict__ gf,
                                                  const uint32_t* __restrict__ cidx, uint32_t ng, uint32_t* __restrict__ cstart,
                                                  uint32_t* __restrict__ csize, uint64_t* __restrict__ ckey, uint64_t* __restrict__ cpay) {
  const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= ng || !gf[g]) return;
  const uint32_t c = cidx[g], s = gstart[g], sz = gstart[g + 1] - s;
  cstart[c] = s;
  csize[c] = sz;
  ckey[c] = 0xffffffffu - sz;
  cpay[c] = c;
}

// ---- chain ----------------------------------------------------------------------------------------------------------------------
__device__ inline int32_t wave_max_i32(int32_t v) {
  const int32_t ident = INT32_MIN;
  v = max(v, __builtin_amdgcn_update_dpp(ident, v, 0x111, 0xf, 0xf, false));   // row_shr:1
  v = max(v, __builtin_amdgcn_update_dpp(ident, v, 0x112, 0xf, 0xf, false));   // row_shr:2
  v = max(v, __builtin_amdgcn_update_dpp(ident, v, 0x114, 0xf, 0xf, false));   // row_shr:4
  v = max(v, __builtin_amdgcn_update_dpp(ident, v, 0x118, 0xf, 0xf, false));   // row_shr:8 -> lane 15 of a row holds the row
  v = max(v, __builtin_amdgcn_update_dpp(ident, v, 0x142, 0xa, 0xf, false));   // row_bcast:15 into rows 1 and 3
  v = max(v, __builtin_amdgcn_update_dpp(ident, v, 0x143, 0xc, 0xf, false));   // row_bcast:31 into rows 2 and 3
  return __builtin_amdgcn_readlane(v, 63);
}

struct ChainEnd { int32_t score; uint32_t last; };

// One wave per group.  Lane l holds anchor (i & 63) == l of the current block of 64 anchors (cur_*) and of the one before
// (prev_*), and in `fr` the f of the newest anchor with that residue: for anchor i = base + m the predecessor of lane l is
// base + l (l < m) or base - 64 + l (l >= m) — exactly i - 1 ... i - 64.
__global__ __launch_bounds__(64) void k_chain(const uint64_t* __restrict__ A, const uint64_t* __restrict__ order,
                                              const uint32_t* __restrict__ cstart, const uint32_t* __restrict__ csize,
                                              uint8_t* __restrict__ pred, ChainEnd* __restrict__ ends, int32_t k, int32_t bandwidth,
                                              int32_t max_gap) {
  const uint32_t c = (uint32_t)order[blockIdx.x];
  const uint32_t s0 = cstart[c], n = csize[c];
  const uint32_t lane = threadIdx.x;
  int32_t fr = 0, cur_t = 0, cur_q = 0, prev_t = 0, prev_q = 0;
  int32_t best_f = -1;
  uint32_t best_i = 0;
  for (uint32_t base = 0; base < n; base += 64) {
    prev_t = cur_t;
    prev_q = cur_q;
    if (base + lane < n) {
      const uint64_t a = A[(uint64_t)s0 + base + lane];
      cur_t = (int32_t)(a >> 32);
      cur_q = (int32_t)(uint32_t)a;
    }
    const uint32_t m_end = min(64u, n - base);
    uint32_t my_pd = 0;
    for (uint32_t m = 0; m < m_end; m++) {
      const int32_t ti = __builtin_amdgcn_readlane(cur_t, m), qi = __builtin_amdgcn_readlane(cur_q, m);
      const bool newer = lane < m;
      const int32_t tj = newer ? cur_t : prev_t, qj = newer ? cur_q : prev_q;
      const bool exists = newer || base >= 64;
      const int32_t dt = ti - tj, dq = qi - qj;
      const int32_t diff = dt - dq;
      const int32_t dd = diff < 0 ? -diff : diff;
      const bool ok = exists && dt > 0 && dq > 0 && dt <= max_gap && dq <= max_gap && dd <= bandwidth;
      int32_t sc = INT32_MIN;
      if (ok) {
        const int64_t cost = (((int64_t)dd * k) >> 6) + ((31 - __clz(dd + 1)) >> 1);
        const int64_t v = (int64_t)fr + min(k, min(dt, dq)) - cost;
        if (v > k) sc = (int32_t)v;
      }
      const int32_t mx = wave_max_i32(sc);
      int32_t f_i = k;
      uint32_t pd = 0;                          // distance to the chosen predecessor, 0: none
      if (mx > k) {
        const uint64_t hit = __ballot(sc == mx);
        const uint64_t low = hit & ((1ull << m) - 1);          // the nearest: the highest lane below m, else the highest of all
        const uint32_t lj = 63u - (uint32_t)__clzll(low ? low : hit);
        pd = lj < m ? m - lj : m - lj + 64u;
        f_i = mx;
      }
      if (lane == m) { fr = f_i; my_pd = pd; }
      if (f_i > best_f) { best_f = f_i; best_i = base + m; }    // strictly better: the smallest i wins ties
    }
    if (base + lane < n) pred[(uint64_t)s0 + base + lane] = (uint8_t)my_pd;
  }
  if (lane == 0) ends[c] = ChainEnd{best_f, best_i};
}

// The score of one predecessor (t_j, q_j, f_j) of anchor (t_i, q_i): k_chain's conditions and cost, INT32_MIN where it is no candidate.
// in_gap: the predecessor exists and dt <= max_gap — what the early stop of k_chain_far asks of a round.
__device__ inline int32_t chain_cand(int32_t ti, int32_t qi, int32_t tj, int32_t qj, int32_t fj, bool exists, int32_t k, int32_t bandwidth,
                                     int32_t max_gap, bool& in_gap) {
  const int32_t dt = ti - tj, dq = qi - qj;
  const int32_t diff = dt - dq;
  const int32_t dd = diff < 0 ? -diff : diff;
  in_gap = exists && dt <= max_gap;
  if (!(in_gap && dt > 0 && dq > 0 && dq <= max_gap && dd <= bandwidth)) return INT32_MIN;
  const int64_t cost = (((int64_t)dd * k) >> 6) + ((31 - __clz(dd + 1)) >> 1);
  const int64_t v = (int64_t)fj + min(k, min(dt, dq)) - cost;
  return v > k ? (int32_t)v : INT32_MIN;
}

// k_chain for a look-back of H = 64 R anchors, R = 2 .. 16 (OvlParams.lookback; DESIGN.md §10, "A longer look-back").  One wave per group.
// The current block of 64 anchors and the one before it sit in registers as in k_chain; (t, q, f) of the R finished blocks in front of the
// current one sit in a ring in LDS, 12 B per anchor, block b in slot b mod R at index slot * 64 + lane: a lane only ever reads what it wrote
// itself, so the ring needs no barrier.  For anchor i = base + m, round r = 0 .. R - 1 gives lane l the predecessor base + l - 64 r (l < m) or
// base + l - 64 (r + 1) (l >= m): the rounds together are exactly i - 1 ... i - H.  A lane keeps the best of its R candidates, a farther one only
// where it is strictly better, so the nearest wins the lane's ties; the wave's maximum and, among the lanes that hold it, the least distance
// are one reduction each.  The anchors ascend by tpos: a round in which no lane has an existing predecessor with dt <= max_gap ends the
// rounds of the step — every farther predecessor fails the same condition, or does not exist either.
__global__ __launch_bounds__(64) void k_chain_far(const uint64_t* __restrict__ A, const uint64_t* __restrict__ order,
                                                  const uint32_t* __restrict__ cstart, const uint32_t* __restrict__ csize,
                                                  uint16_t* __restrict__ pred, ChainEnd* __restrict__ ends, int32_t k, int32_t bandwidth,
                                                  int32_t max_gap, int32_t rounds) {
  extern __shared__ int32_t ring[];             // [3][rounds * 64]: t, q, f
  int32_t* const ring_t = ring;
  int32_t* const ring_q = ring + rounds * 64;
  int32_t* const ring_f = ring + rounds * 128;
  const uint32_t c = (uint32_t)order[blockIdx.x];
  const uint32_t s0 = cstart[c], n = csize[c];
  const uint32_t lane = threadIdx.x;
  int32_t fr = 0, cur_t = 0, cur_q = 0, prev_t = 0, prev_q = 0;
  int32_t best_f = -1;
  uint32_t best_i = 0;
  int32_t slot = 0, blk = 0;                    // the current block and its slot in the ring: blk mod rounds
  for (uint32_t base = 0; base < n; base += 64) {
    prev_t = cur_t;
    prev_q = cur_q;
    if (base + lane < n) {
      const uint64_t a = A[(uint64_t)s0 + base + lane];
      cur_t = (int32_t)(a >> 32);
      cur_q = (int32_t)(uint32_t)a;
    }
    const uint32_t m_end = min(64u, n - base);
    uint32_t my_pd = 0;
    for (uint32_t m = 0; m < m_end; m++) {
      const int32_t ti = __builtin_amdgcn_readlane(cur_t, m), qi = __builtin_amdgcn_readlane(cur_q, m);
      const bool newer = lane < m;
      const int32_t d0 = newer ? (int32_t)(m - lane) : (int32_t)(m - lane) + 64;      // the distance of the lane's predecessor in round 0
      bool in_gap;
      int32_t sc = chain_cand(ti, qi, newer ? cur_t : prev_t, newer ? cur_q : prev_q, fr, newer || base >= 64, k, bandwidth, max_gap, in_gap);
      int32_t dist = d0;
      const int32_t older = newer ? 0 : 1;      // blocks behind the round's own
      for (int32_t r = 1; r < rounds && __ballot(in_gap); r++) {
        int32_t s = slot - r - older;
        if (s < 0) s += rounds;
        const int32_t at = s * 64 + (int32_t)lane;
        const int32_t v = chain_cand(ti, qi, ring_t[at], ring_q[at], ring_f[at], blk - r - older >= 0, k, bandwidth, max_gap, in_gap);
        if (v > sc) { sc = v; dist = d0 + 64 * r; }            // strictly better: the nearer round wins ties
      }
      const int32_t mx = wave_max_i32(sc);
      int32_t f_i = k;
      uint32_t pd = 0;                          // distance to the chosen predecessor, 0: none
      if (mx > k) {
        pd = (uint32_t)-wave_max_i32(sc == mx ? -dist : INT32_MIN);      // the nearest of the lanes that hold the maximum
        f_i = mx;
      }
      if (lane == m) { fr = f_i; my_pd = pd; }
      if (f_i > best_f) { best_f = f_i; best_i = base + m; }    // strictly better: the smallest i wins ties
    }
    if (base + lane < n) pred[(uint64_t)s0 + base + lane] = (uint16_t)my_pd;
    const int32_t at = slot * 64 + (int32_t)lane;
    ring_t[at] = cur_t;
    ring_q[at] = cur_q;
    ring_f[at] = fr;
    blk++;
    if (++slot == rounds) slot = 0;
  }
  if (lane == 0) ends[c] = ChainEnd{best_f, best_i};
}

struct GroupOut { uint32_t t, q, rel, n_anchors; int32_t score; uint32_t tstart, tend, qstart, qend, kept; };

template <class Pred>   // uint8_t behind k_chain, uint16_t behind k_chain_far
__global__ __launch_bounds__(256) void k_walk(const uint64_t* __restrict__ A, const uint64_t* __restrict__ B,
                                              const uint32_t* __restrict__ cstart, const Pred* __restrict__ pred,
                                              const ChainEnd* __restrict__ ends, uint32_t nc, const uint64_t* __restrict__ base_off,
                                              uint32_t k, uint32_t t_lo, uint32_t min_score, uint32_t min_anchors,
                                              GroupOut* __restrict__ out) {
  const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= nc) return;
  const uint64_t s0 = cstart[c];
  const ChainEnd e = ends[c];
  uint32_t i = e.last, cnt = 1;
  for (uint32_t pd = pred[s0 + i]; pd; pd = pred[s0 + i]) { i -= pd; cnt++; }
  const uint64_t b = B[s0], a0 = A[s0 + i], a1 = A[s0 + e.last];
  GroupOut g;
  g.t = t_lo + (uint32_t)(b >> 33);
  g.q = (uint32_t)(b >> 1);
  g.rel = (uint32_t)b & 1u;
  g.n_anchors = cnt;
  g.score = e.score;
  g.tstart = (uint32_t)(a0 >> 32) - k + 1;
  g.tend = (uint32_t)(a1 >> 32) + 1;
  const uint32_t qs = (uint32_t)a0 - k + 1, qe = (uint32_t)a1 + 1;      // on the oriented query
  const uint32_t qlen = (uint32_t)(base_off[g.q + 1] - base_off[g.q]);
  g.qstart = g.rel ? qlen - qe : qs;
  g.qend = g.rel ? qlen - qs : qe;
  g.kept = ((int64_t)e.score >= (int64_t)min_score && cnt >= min_anchors) ? 1u : 0u;
  out[c] = g;
}

// ---- one overlap per pair (ovl_find_pairs) and the row table (ovl_row_table) -----------------------------------------------------------------
// A kept chain is its pair's overlap unless the kept chain of the other strand wins: the reverse strand with a strictly greater score, the
// forward strand with a greater or equal one (the forward strand on a tie).  The two are neighbours in g: ascending (t, q, rel).
__global__ __launch_bounds__(256) void k_pick(const GroupOut* __restrict__ g, uint32_t nc, uint32_t* __restrict__ sel) {
  const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= nc) return;
  const GroupOut x = g[c];
  uint32_t s = x.kept;
  if (s && x.rel == 0 && c + 1 < nc) {
    const GroupOut y = g[c + 1];
    if (y.kept && y.t == x.t && y.q == x.q && y.score > x.score) s = 0;
  } else if (s && x.rel != 0 && c > 0) {
    const GroupOut y = g[c - 1];
    if (y.kept && y.t == x.t && y.q == x.q && y.score >= x.score) s = 0;
  }
  sel[c] = s;
}

// the selected chains as records (query c.q on target c.t), in chain order, from out[0] on
__global__ __launch_bounds__(256) void k_prim_write(const GroupOut* __restrict__ g, const uint32_t* __restrict__ sel,
                                                    const uint32_t* __restrict__ soff, uint32_t nc, const uint64_t* __restrict__ base_off,
                                                    OvlRec* __restrict__ out) {
  const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= nc || !sel[c]) return;
  const GroupOut x = g[c];
  const uint32_t ql = (uint32_t)(base_off[x.q + 1] - base_off[x.q]), tl = (uint32_t)(base_off[x.t + 1] - base_off[x.t]);
  out[soff[c]] = OvlRec{x.q, ql, x.qstart, x.qend, x.rel, x.t, tl, x.tstart, x.tend, x.score};
}

// ---- an index in parts (OvlParams.index_kmers != 0; DESIGN.md section 10, "An index in parts"; tests/index_parts_ref.py) ------------------------
// Everything the finder takes from the whole store's index is occ(hash), the occurrences of a minimizer's hash in the store.  Pass A leaves
// occ16[ordinal] = min(occ, 65535) for every minimizer, its ordinal being its place in the store's (rid, pos) order; pass B runs the finder per
// pair of read blocks and judges every hash run by its members' occ16, never by its length inside the pair.  These kernels run only under the
// setting: the ones above are launched exactly as before.

// k_sketch over the tiles of one read block.  tile_off is the whole store's; u_at / f_at / cnt are the block's own slices, indexed by the tile
// inside the block.  The window minimum is taken over all hashes; a hash range only filters what is selected.
//   SKP_COUNT        cnt[tile] = the tile's minimizers
//   SKP_COUNT_RANGE  cnt[tile] = those with h_lo <= hash <= h_hi
//   SKP_WRITE_RANGE  the latter's hash and ordinal (ord_base + u_at[tile] + the rank in the tile), densely from out_base + f_at[tile] on
//   SKP_WRITE_BLOCK  hash, meta and occ = occ16[ordinal] of all of them from out_base + u_at[tile] on; meta_loc (or NULL): meta with the read id
//                    counted from the block's first read, which is what k_rescue is launched over
enum { SKP_COUNT = 0, SKP_COUNT_RANGE = 1, SKP_WRITE_RANGE = 2, SKP_WRITE_BLOCK = 3 };
struct SketchPart {
  const uint64_t *words, *word_off, *base_off;
  const uint32_t* tile_off;
  uint32_t r_lo, r_hi, tile0, k, w;
  uint64_t h_lo, h_hi;
  const uint32_t *u_at, *f_at;
  uint32_t* cnt;
  uint64_t ord_base;
  uint32_t out_base;
  uint64_t *hash_out, *meta_out, *ord_out, *meta_loc;
  uint32_t* occ_out;
  const uint16_t* occ16;
};

template <int MODE>
__global__ __launch_bounds__(SK_T) void k_sketch_part(const SketchPart a) {
  __shared__ uint64_t sh[SK_H];
  __shared__ uint64_t wm[SK_H];
  __shared__ uint8_t ss[SK_H];
  __shared__ uint32_t wc[2][4];
  const uint32_t lt = blockIdx.x, tid = threadIdx.x, k = a.k;
  const SketchTile t = sketch_tile(a.words, a.word_off, a.base_off, a.tile_off, a.r_lo, a.r_hi, a.tile0 + lt, k, a.w, sh, wm, ss);
  const bool in_range = t.sel && t.hj >= a.h_lo && t.hj <= a.h_hi;
  const uint64_t bal = __ballot(t.sel), bal_r = __ballot(in_range);
  const uint32_t lane = tid & 63, wave = tid >> 6;
  if (lane == 0) { wc[0][wave] = (uint32_t)__popcll(bal); wc[1][wave] = (uint32_t)__popcll(bal_r); }
  __syncthreads();
  uint32_t before = 0, total = 0, before_r = 0, total_r = 0;
  for (uint32_t i = 0; i < 4; i++) {
    if (i < wave) { before += wc[0][i]; before_r += wc[1][i]; }
    total += wc[0][i];
    total_r += wc[1][i];
  }
  if constexpr (MODE == SKP_COUNT) {
    if (tid == 0) a.cnt[lt] = total;
  } else if constexpr (MODE == SKP_COUNT_RANGE) {
    if (tid == 0) a.cnt[lt] = total_r;
  } else {
    const uint32_t urank = a.u_at[lt] + before + (uint32_t)__popcll(bal & ((1ull << lane) - 1));
    if constexpr (MODE == SKP_WRITE_RANGE) {
      if (in_range) {
        const uint32_t at = a.out_base + a.f_at[lt] + before_r + (uint32_t)__popcll(bal_r & ((1ull << lane) - 1));
        a.hash_out[at] = t.hj;
        a.ord_out[at] = a.ord_base + urank;
      }
    } else if (t.sel) {
      const uint32_t at = a.out_base + urank;
      const uint64_t low = ((uint64_t)(t.j + k - 1) << 1) | ss[t.j - t.lo];
      a.hash_out[at] = t.hj;
      a.meta_out[at] = ((uint64_t)t.rid << 32) | low;
      if (a.meta_loc) a.meta_loc[at] = ((uint64_t)(t.rid - a.r_lo) << 32) | low;
      a.occ_out[at] = a.occ16[a.ord_base + urank];
    }
  }
}

// Pass A, behind the sort of a hash range by hash (run_starts): every member's occ16 at its ordinal — a run lies in one range, so its length is the
// store's occ — and the run in the census, hist[min(length, 65535)] += 1, in 64-bit bins.
__global__ __launch_bounds__(256) void k_occ16(const uint64_t* __restrict__ ord, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ gidx,
                                               const uint32_t* __restrict__ rstart, uint32_t n, uint16_t* __restrict__ occ16,
                                               unsigned long long* __restrict__ hist) {
  __shared__ uint32_t h[OCC_LDS_BINS];
  occ_bins_clear(h);
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    const uint32_t f = flag[i], r = gidx[i] + f - 1;
    const uint32_t c = min(rstart[r + 1] - rstart[r], OVL_OCC_BINS - 1);
    occ16[ord[i]] = (uint16_t)c;
    if (f) occ_bins_add(h, hist, c);
  }
  occ_bins_flush(h, hist);
}

// Pass B.  The class of a minimizer of a block pair from its occ alone, in (rid, pos) order: 0 — its hash is not used (a singleton, above the cut
// and not rescuable), 1 — used (2 <= occ <= cut), 2 — cut < occ <= rmax and not rescued, 3 — rescued.  resc NULL / rmax 0: no rescue.  idx[p] = p,
// the payload of the sort by hash.  occ: where k_occ_pick left the cut, or NULL — the cut is max_occ.
__global__ __launch_bounds__(256) void k_part_cls(const uint32_t* __restrict__ occ_rp, const uint8_t* __restrict__ resc_rp, uint32_t n, uint32_t max_occ,
                                                  const uint64_t* __restrict__ occ, uint32_t rmax, uint8_t* __restrict__ cls, uint64_t* __restrict__ idx) {
  const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const uint32_t cut = occ ? (uint32_t)occ[0] : max_occ;
  const uint32_t c = occ_rp[p];
  uint8_t v = 0;
  if (c >= 2 && c <= cut) v = 1;
  else if (resc_rp && c > cut && c <= rmax) v = resc_rp[p] ? 3 : 2;
  cls[p] = v;
  idx[p] = p;
}

// behind the sort: meta and class in hash order
__global__ __launch_bounds__(256) void k_part_gather(const uint64_t* __restrict__ idx, const uint64_t* __restrict__ meta, const uint8_t* __restrict__ cls,
                                                     uint32_t n, uint64_t* __restrict__ meta_s, uint8_t* __restrict__ cls_s) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t p = idx[i];
  meta_s[i] = meta[p];
  cls_s[i] = cls[p];
}

// Does occurrence x (read t, class cx >= 1, t in front of `split` where split != 0) have an anchor with the later occurrence y of its run?
// The pair rule: y lies in another read — behind t, the run is in (rid, pos) order —; split != 0 (blocks i < j, split = block j's first read): y
// lies in block j; a run above the cut: one of the two is rescued; CORE: one of the two reads is core.
template <bool CORE>
__device__ inline bool part_pair_ok(uint32_t t, bool t_core, uint32_t cx, uint64_t my, uint32_t cy, uint32_t split, const uint8_t* __restrict__ core) {
  const uint32_t q = (uint32_t)(my >> 32);
  if (q == t || q < split) return false;
  if (cx >= 2 && cx != 3 && cy != 3) return false;
  if constexpr (CORE) {
    if (!t_core && core[q] == 0) return false;
  }
  return true;
}

// k_runs for a block pair, one thread per occurrence: it walks its run to the end — at most max(cut, rmax) steps: a used run has no more members
// in the whole store — and counts the partners the pair rule gives it.  cnt is cleared before the launch; per_read is indexed from read t0, the
// first of block i, where every target of the pair lies; stat[2] sums the anchors of the runs above the cut.
template <bool CORE>
__global__ __launch_bounds__(256) void k_part_runs(const uint64_t* __restrict__ hash, const uint64_t* __restrict__ meta, const uint8_t* __restrict__ cls,
                                                   uint32_t n, uint32_t split, uint32_t t0, uint32_t* __restrict__ cnt, uint32_t* __restrict__ run_end,
                                                   unsigned long long* __restrict__ per_read, const uint8_t* __restrict__ core,
                                                   unsigned long long* __restrict__ stat) {
  const uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (x >= n) return;
  const uint32_t cx = cls[x];
  if (!cx) return;
  const uint32_t t = (uint32_t)(meta[x] >> 32);
  if (split && t >= split) return;               // (block j's reads are queries only)
  bool t_core = true;
  if constexpr (CORE) t_core = core[t] != 0;
  const uint64_t h = hash[x];
  uint32_t m = 0;
  uint64_t y = x + 1;
  for (; y < n && hash[y] == h; y++) m += part_pair_ok<CORE>(t, t_core, cx, meta[y], cls[y], split, core) ? 1u : 0u;
  run_end[x] = (uint32_t)y;
  if (!m) return;
  cnt[x] = m;
  atomicAdd(&per_read[t - t0], (unsigned long long)m);
  if (cx >= 2) atomicAdd(&stat[2], (unsigned long long)m);
}

// k_expand for a block pair: the same walk writes the cntm[x] anchors of x from aoff[x] on
template <bool CORE>
__global__ __launch_bounds__(256) void k_part_expand(const uint64_t* __restrict__ meta, const uint8_t* __restrict__ cls, const uint32_t* __restrict__ cntm,
                                                     const uint32_t* __restrict__ run_end, const uint32_t* __restrict__ aoff, uint32_t n, uint32_t split,
                                                     const uint64_t* __restrict__ base_off, uint32_t k, uint32_t t_lo, uint64_t* __restrict__ A,
                                                     uint64_t* __restrict__ B, const uint8_t* __restrict__ core) {
  const uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (x >= n) return;
  const uint32_t c = cntm[x];
  if (!c) return;
  const uint64_t mx = meta[x];
  const uint32_t t = (uint32_t)(mx >> 32), tpos = ((uint32_t)mx) >> 1, st = (uint32_t)mx & 1u, cx = cls[x];
  bool t_core = true;
  if constexpr (CORE) t_core = core[t] != 0;
  const uint32_t e = run_end[x];
  uint32_t at = aoff[x];
  const uint32_t at_end = at + c;
  for (uint32_t y = (uint32_t)x + 1; y < e && at < at_end; y++) {
    const uint64_t my = meta[y];
    if (!part_pair_ok<CORE>(t, t_core, cx, my, cls[y], split, core)) continue;
    const uint32_t q = (uint32_t)(my >> 32), qp = ((uint32_t)my) >> 1, rel = ((uint32_t)my & 1u) ^ st;
    const uint32_t qlen = (uint32_t)(base_off[q + 1] - base_off[q]);
    const uint32_t qpos = rel ? qlen - qp + k - 2 : qp;
    A[at] = ((uint64_t)tpos << 32) | qpos;
    B[at] = ((uint64_t)(t - t_lo) << 33) | ((uint64_t)q << 1) | rel;
    at++;
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
// Run starts of the sorted keys[0 .. n), n >= 1, queued on st: flag[i] = 1 where a run begins; gidx [n + 1] its exclusive scan — element i lies in
// run gidx[i] + flag[i] - 1, gidx[n] is the number of runs —; rstart[r] the first element of run r, rstart[gidx[n]] = n.  partial: the scan's scratch.
int run_starts(const uint64_t* keys, uint32_t n, uint32_t* flag, uint32_t* gidx, uint32_t* rstart, uint32_t* partial, hipStream_t st, std::string& err) {
  k_heads<<<nblk(n), 256, 0, st>>>(keys, n, flag);
  if (int rc = dev_scan_u32(flag, n, gidx, partial, st, err)) return rc;
  k_gstart<<<nblk(n), 256, 0, st>>>(flag, gidx, n, rstart);
  OVL_TRY(hipGetLastError());
  return OVL_OK;
}

// f(std::true_type) with a core mask, f(std::false_type) without one: the launch of a kernel with a CORE variant is written once, in a generic
// lambda, as K<decltype(core)::value><<<...>>>(..., d_core) — d_core is NULL exactly where CORE is false.
template <class F>
void with_core(const uint8_t* d_core, F f) { d_core ? f(std::true_type{}) : f(std::false_type{}); }

// body(), and where it fails the stream is waited for before the scratch the body queued work on goes away
template <class F>
int synced_on_failure(hipStream_t st, F body) {
  const int rc = body();
  if (rc != OVL_OK) (void)hipStreamSynchronize(st);
  return rc;
}

// the digits of a hash: 2 k bits
std::vector<uint32_t> hash_shifts(uint32_t k) {
  std::vector<uint32_t> shifts;
  field_shifts(shifts, 0, 2 * k);
  return shifts;
}

uint32_t max_read_len(const OvlStore& S) { return S.n_reads ? *std::max_element(S.h_len, S.h_len + S.n_reads) : 0u; }

// The figures of a call without a census of its own: the cut is max_occ, or — occ_frac_ppm != 0, which then means fewer than two minimizers — the
// pick's over as many runs of one.
void stats_without_census(OvlStats& stats, uint64_t minimizers, const OvlParams& P) {
  const bool frac = P.occ_frac_ppm != 0;
  stats.occ_cut = frac ? occ_final_cut((uint32_t)minimizers, P.max_occ) : P.max_occ;
  stats.distinct = frac ? minimizers : 0;
  stats.cut_runs = stats.cut_minimizers = 0;
}

struct Sketch {            // device: minimizers in (rid, pos) order
  uint64_t* hash = nullptr;
  uint64_t* meta = nullptr;
  uint32_t n = 0;
  uint64_t kmers = 0;
};

int check_store(const OvlStore& S, std::string& err) {
  if (S.n_reads > OVL_MAX_READS) { err = "overlap finder: more than 2^31 - 1 reads"; return OVL_UNSUPPORTED; }
  for (uint32_t r = 0; r < S.n_reads; r++)
    if (S.h_len[r] > OVL_MAX_READ_LEN) { err = "overlap finder: read " + std::to_string(r) + " is longer than 2^31 - 1 bases"; return OVL_UNSUPPORTED; }
  return OVL_OK;
}

// tile_off [n_reads + 1]: the first sketch tile of every read, tile_off[n_reads] = the tiles of the store; a read has the k-mers index_read_kmers
// gives it (none if it is shorter than k + w - 1) in tiles of SK_T.  Returns the tiles in 64 bits and leaves the k-mers in `kmers`: the 32-bit
// entries hold only once the caller has found the totals within its limit.
uint64_t tile_table(const OvlStore& S, const OvlParams& P, std::vector<uint32_t>& tile_off, uint64_t& kmers) {
  tile_off.assign((size_t)S.n_reads + 1, 0);
  uint64_t tiles = 0;
  kmers = 0;
  for (uint32_t r = 0; r < S.n_reads; r++) {
    tile_off[r] = (uint32_t)tiles;
    const uint64_t nk = index_read_kmers(S.h_len[r], P.k, P.w);
    kmers += nk;
    tiles += (nk + SK_T - 1) / SK_T;
  }
  tile_off[S.n_reads] = (uint32_t)tiles;
  return tiles;
}

int sketch_dev(const OvlStore& S, const OvlParams& P, hipStream_t st, Bufs& B, Sketch& out, std::string& err) {
  if (int rc = check_store(S, err)) return rc;
  std::vector<uint32_t> tile_off;
  uint64_t kmers;
  const uint64_t tiles = tile_table(S, P, tile_off, kmers);
  if (kmers > OVL_MAX_KMERS) { err = "overlap finder: more than 2^32 k-mers in the read store"; return OVL_UNSUPPORTED; }
  out.kmers = kmers;
  out.n = 0;
  if (!tiles) return OVL_OK;
  const uint32_t nt = (uint32_t)tiles;
  uint32_t *d_tile_off, *d_cnt, *d_at, *d_partial;
  OVL_TRY(B.get(&d_tile_off, (uint64_t)S.n_reads + 1));
  OVL_TRY(B.get(&d_cnt, nt));
  OVL_TRY(B.get(&d_at, (uint64_t)nt + 1));
  OVL_TRY(B.get(&d_partial, nblk(nt, SC_TILE) + 2));
  OVL_TRY(hipMemcpyAsync(d_tile_off, tile_off.data(), 4ull * (S.n_reads + 1), hipMemcpyHostToDevice, st));
  k_sketch<<<nt, SK_T, 0, st>>>(S.d_words, S.d_word_off, S.d_base_off, d_tile_off, S.n_reads, P.k, P.w, d_cnt, nullptr, nullptr, nullptr, 0);
  OVL_TRY(hipGetLastError());
  if (int rc = dev_scan_u32(d_cnt, nt, d_at, d_partial, st, err)) return rc;
  uint32_t total = 0;
  OVL_TRY(hipMemcpyAsync(&total, d_at + nt, 4, hipMemcpyDeviceToHost, st));
  OVL_TRY(hipStreamSynchronize(st));           // (also keeps tile_off alive until its copy is done)
  out.n = total;
  OVL_TRY(B.get(&out.hash, total));
  OVL_TRY(B.get(&out.meta, total));
  if (total) {
    k_sketch<<<nt, SK_T, 0, st>>>(S.d_words, S.d_word_off, S.d_base_off, d_tile_off, S.n_reads, P.k, P.w, d_cnt, d_at, out.hash, out.meta, 1);
    OVL_TRY(hipGetLastError());
  }
  return OVL_OK;
}

}  // namespace

int ovl_sketch(const OvlStore& S, const OvlParams& P, hipStream_t st, std::vector<uint64_t>& hash, std::vector<uint64_t>& meta,
               std::string& err) {
  Bufs B;
  Sketch sk;
  if (int rc = sketch_dev(S, P, st, B, sk, err)) return rc;
  hash.resize(sk.n);
  meta.resize(sk.n);
  if (sk.n) {
    OVL_TRY(hipMemcpyAsync(hash.data(), sk.hash, 8ull * sk.n, hipMemcpyDeviceToHost, st));
    OVL_TRY(hipMemcpyAsync(meta.data(), sk.meta, 8ull * sk.n, hipMemcpyDeviceToHost, st));
  }
  OVL_TRY(hipStreamSynchronize(st));
  return OVL_OK;
}

namespace {
// The index of the whole store, queued on st — what ovl_find / ovl_find_pairs without index_kmers, ovl_occ_census and ovl_seed_rescue start from:
//   the sketch; with fewer than `least` minimizers that is all (built stays false: the caller's early return);
//   rescue: the copy of meta the rescue searches, taken while it is still in (rid, pos) order;
//   the sort by hash (stable: (rid, pos) order inside a hash); ms, the sort's scratch for sk.n elements, is the caller's to go on using;
//   census or rescue: the run starts of the sorted hashes, which serve both;
//   census: the histogram of the run lengths and the pick — d_occ = {cut, distinct, runs above the cut, minimizers in them}, d_hist;
//   rescue ("Rescue of high-frequency minimizers"): occ_rp and resc_rp in (rid, pos) order, kind in hash order and stat =
//   {H minimizers, rescued, 0}; k_rescue itself only with P.occ_dist != 0 (0 is the test hook with the setting off — the occurrences alone); the cut is
//   d_occ's, or, without a census, max_occ.  The selection is done before any chunk is cut and sees neither the core mask nor the scratch budget.
// flag [n] and gidx [n + 1] are allocated in every case: behind what is queued here they are free, and find_chunks' cntm and aoff.
struct StoreIndex {
  Sketch sk;
  bool built = false;
  SortScratch ms;
  uint32_t *flag = nullptr, *gidx = nullptr, *rstart = nullptr;
  uint32_t* d_hist = nullptr;
  uint64_t *d_occ = nullptr, *meta_rp = nullptr;
  uint32_t *occ_rp = nullptr, *perm = nullptr;
  uint8_t *resc_rp = nullptr, *kind = nullptr;
  unsigned long long* stat = nullptr;
};

int store_index(const OvlStore& S, const OvlParams& P, bool census, bool rescue, uint32_t least, hipStream_t st, Bufs& B, StoreIndex& X,
                std::string& err) {
  Sketch& sk = X.sk;
  if (int rc = sketch_dev(S, P, st, B, sk, err)) return rc;
  const uint32_t n = sk.n;
  if (n < least) return OVL_OK;
  X.built = true;
  if (rescue) {
    OVL_TRY(B.get(&X.meta_rp, n));
    OVL_TRY(hipMemcpyAsync(X.meta_rp, sk.meta, 8ull * n, hipMemcpyDeviceToDevice, st));
  }
  uint64_t *mk1, *mp1;
  OVL_TRY(B.get(&mk1, n));
  OVL_TRY(B.get(&mp1, n));
  OVL_TRY(X.ms.alloc(B, n));
  if (int rc = dev_radix_sort(&sk.hash, &sk.meta, &mk1, &mp1, n, hash_shifts(P.k), X.ms, st, err)) return rc;
  OVL_TRY(B.get(&X.flag, n));
  OVL_TRY(B.get(&X.gidx, (uint64_t)n + 1));
  if (!census && !rescue) return OVL_OK;
  OVL_TRY(B.get(&X.rstart, (uint64_t)n + 1));
  if (int rc = run_starts(sk.hash, n, X.flag, X.gidx, X.rstart, X.ms.partial, st, err)) return rc;
  if (census) {
    OVL_TRY(B.get(&X.d_hist, OVL_OCC_BINS));
    OVL_TRY(B.get(&X.d_occ, 4));
    OVL_TRY(hipMemsetAsync(X.d_hist, 0, 4ull * OVL_OCC_BINS, st));
    k_occ_census<<<std::min(nblk(n), OCC_GRID), 256, 0, st>>>(X.rstart, X.gidx + n, X.d_hist);
    k_occ_pick<<<1, 256, 0, st>>>(X.d_hist, n, P.occ_frac_ppm, P.max_occ, X.d_occ);
  }
  if (rescue) {
    OVL_TRY(B.get(&X.occ_rp, n));
    OVL_TRY(B.get(&X.perm, n));
    OVL_TRY(B.get(&X.resc_rp, n));
    OVL_TRY(B.get(&X.kind, n));
    OVL_TRY(B.get(&X.stat, 3));
    OVL_TRY(hipMemsetAsync(X.resc_rp, 0, n, st));
    OVL_TRY(hipMemsetAsync(X.stat, 0, 24, st));
    k_occ_place<<<nblk(n), 256, 0, st>>>(sk.meta, X.meta_rp, X.flag, X.gidx, X.rstart, n, X.occ_rp, X.perm);
    if (P.occ_dist)
      k_rescue<<<S.n_reads, 64, 0, st>>>(X.meta_rp, X.occ_rp, n, S.d_base_off, P.max_occ, X.d_occ, P.rescue_max_occ, P.occ_dist, X.resc_rp, X.stat);
    k_resc_kind<<<nblk(n), 256, 0, st>>>(X.perm, X.occ_rp, X.resc_rp, n, P.max_occ, X.d_occ, P.rescue_max_occ, X.kind);
  }
  OVL_TRY(hipGetLastError());
  return OVL_OK;
}

// The chain stage of a chunk, and all of ovl_chain_groups: the nc groups (cstart, csize; ck0 / cp0 as k_gcompact leaves them) ordered largest first,
// chained by k_chain (P.lookback == 64: pred8) or k_chain_far (pred16), walked back into gout.
struct ChainBufs {
  uint64_t *ck0, *cp0, *ck1, *cp1;
  uint32_t *cstart, *csize;
  uint8_t* pred8;
  uint16_t* pred16;
  ChainEnd* ends;
  GroupOut* gout;
};
int chain_and_walk(const uint64_t* A0, const uint64_t* B0, ChainBufs& C, uint32_t nc, const OvlParams& P, const uint64_t* d_base_off, uint32_t t_lo,
                   const SortScratch& as, hipStream_t st, std::string& err) {
  if (int rc = dev_radix_sort(&C.ck0, &C.cp0, &C.ck1, &C.cp1, nc, {0, 8, 16, 24}, as, st, err)) return rc;
  const int32_t bandwidth = (int32_t)std::min<uint32_t>(P.bandwidth, 0x3fffffffu), max_gap = (int32_t)std::min<uint32_t>(P.max_gap, 0x7fffffffu);
  if (P.lookback == OVL_LOOKBACK) {
    k_chain<<<nc, 64, 0, st>>>(A0, C.cp0, C.cstart, C.csize, C.pred8, C.ends, (int32_t)P.k, bandwidth, max_gap);
    k_walk<uint8_t><<<nblk(nc), 256, 0, st>>>(A0, B0, C.cstart, C.pred8, C.ends, nc, d_base_off, P.k, t_lo, P.min_score, P.min_anchors, C.gout);
  } else {
    k_chain_far<<<nc, 64, 12 * P.lookback, st>>>(A0, C.cp0, C.cstart, C.csize, C.pred16, C.ends, (int32_t)P.k, bandwidth, max_gap,
                                                 (int32_t)(P.lookback / 64));
    k_walk<uint16_t><<<nblk(nc), 256, 0, st>>>(A0, B0, C.cstart, C.pred16, C.ends, nc, d_base_off, P.k, t_lo, P.min_score, P.min_anchors, C.gout);
  }
  OVL_TRY(hipGetLastError());
  return OVL_OK;
}
bool lookback_ok(uint32_t h, std::string& err) {
  if (h >= OVL_LOOKBACK && h <= OVL_MAX_LOOKBACK && h % 64 == 0) return true;
  err = "overlap finder: the look-back is a multiple of 64 in 64 .. 1024";
  return false;
}

// What a run stage leaves for the chunk loop (chain_chunks, below): per occurrence in hash order its meta, the anchors it has as the target side
// (cnt) and the end of its run; cntm [nm], aoff [nm + 1] and scan_partial are scratch of the loop.  per_read (host): the anchors of the targets
// t0 .. t1 - 1, which are all the targets the occurrences have; max_len: the longest read of the store.
struct RunsOut {
  const uint64_t* meta;
  uint32_t nm;
  const uint32_t *cnt, *run_end;
  uint32_t *cntm, *aoff, *scan_partial;
  const unsigned long long* per_read;
  uint32_t t0, t1, max_len;
};
template <class Expand, class Take>
int chain_chunks(const OvlStore& S, const OvlParams& P, uint64_t budget_bytes, hipStream_t st, Bufs& B, const RunsOut& RO, OvlStats& stats, std::string& err,
                 Expand expand, Take take);

// The whole store's index, the run stage and the chunk loop of ovl_find and ovl_find_pairs.  Behind every chunk's k_walk, take(nc, gout, ccap, t_hi, B)
// gets the chunk's nc GroupOut records, still on the device, in ascending (t, q, rel): it takes what it wants before it returns or queues its kernels
// on st, in front of the next chunk's k_walk, which overwrites gout.  ccap: the most records any chunk has; t_hi: the targets done so far, this
// chunk's included; B: the call's scratch.  d_core: the core mask on the device (n_reads bytes) or NULL — every read is core.
template <class Take>
int find_chunks(const OvlStore& S, const OvlParams& P, const uint8_t* d_core, uint64_t budget_bytes, hipStream_t st, OvlStats& stats, std::string& err,
                Take take) {
  const bool frac = P.occ_frac_ppm != 0, rescue = P.occ_dist != 0;
  Bufs B;
  StoreIndex X;
  if (int rc = store_index(S, P, frac, rescue, 2, st, B, X, err)) return rc;
  const Sketch& sk = X.sk;
  const uint32_t nm = sk.n;
  stats.kmers = sk.kmers;
  stats.minimizers = nm;
  stats_without_census(stats, nm, P);
  if (!X.built) { OVL_TRY(hipStreamSynchronize(st)); return OVL_OK; }

  uint32_t *d_cnt, *d_run_end, *const d_cntm = X.flag, *const d_aoff = X.gidx;
  unsigned long long* d_per_read;
  OVL_TRY(B.get(&d_cnt, nm));
  OVL_TRY(B.get(&d_run_end, nm));
  OVL_TRY(B.get(&d_per_read, S.n_reads));
  OVL_TRY(hipMemsetAsync(d_cnt, 0, 4ull * nm, st));
  OVL_TRY(hipMemsetAsync(d_per_read, 0, 8ull * S.n_reads, st));
  // the census, the pick and the run kernel queue one behind the other: the cut stays on the device and comes back with per_read
  with_core(d_core, [&](auto core) {
    constexpr bool CORE = decltype(core)::value;
    if (rescue)
      k_runs_resc<CORE><<<nblk(nm), 256, 0, st>>>(sk.hash, sk.meta, nm, P.max_occ, X.d_occ, d_cnt, d_run_end, d_per_read, d_core, P.rescue_max_occ,
                                                  X.kind, X.stat);
    else if (frac) k_runs_occ<CORE><<<nblk(nm), 256, 0, st>>>(sk.hash, sk.meta, nm, X.d_occ, d_cnt, d_run_end, d_per_read, d_core);
    else k_runs<CORE><<<nblk(nm), 256, 0, st>>>(sk.hash, sk.meta, nm, P.max_occ, d_cnt, d_run_end, d_per_read, d_core);
  });
  OVL_TRY(hipGetLastError());
  uint64_t occ[4] = {0, 0, 0, 0};
  unsigned long long resc_stat[3] = {0, 0, 0};
  std::vector<unsigned long long> per_read(S.n_reads);
  OVL_TRY(hipMemcpyAsync(per_read.data(), d_per_read, 8ull * S.n_reads, hipMemcpyDeviceToHost, st));
  if (frac) OVL_TRY(hipMemcpyAsync(occ, X.d_occ, sizeof(occ), hipMemcpyDeviceToHost, st));
  if (rescue) OVL_TRY(hipMemcpyAsync(resc_stat, X.stat, sizeof(resc_stat), hipMemcpyDeviceToHost, st));
  OVL_TRY(hipStreamSynchronize(st));
  if (frac) { stats.occ_cut = occ[0]; stats.distinct = occ[1]; stats.cut_runs = occ[2]; stats.cut_minimizers = occ[3]; }
  if (rescue) { stats.resc_high = resc_stat[0]; stats.rescued = resc_stat[1]; stats.resc_anchors = resc_stat[2]; }

  const RunsOut RO{sk.meta, nm, d_cnt, d_run_end, d_cntm, d_aoff, X.ms.partial, per_read.data(), 0, S.n_reads, max_read_len(S)};
  return chain_chunks(S, P, budget_bytes, st, B, RO, stats, err, [&](uint32_t t_lo, uint64_t* A0, uint64_t* B0) {
    with_core(d_core, [&](auto core) {
      constexpr bool CORE = decltype(core)::value;
      if (rescue)
        k_expand_resc<CORE><<<nblk(nm), 256, 0, st>>>(sk.meta, d_cntm, d_run_end, d_aoff, nm, S.d_base_off, P.k, t_lo, A0, B0, d_core, X.kind);
      else k_expand<CORE><<<nblk(nm), 256, 0, st>>>(sk.meta, d_cntm, d_run_end, d_aoff, nm, S.d_base_off, P.k, t_lo, A0, B0, d_core);
    });
  }, take);
}

// The chunk loop of a run stage's outcome — all of a call, or one block pair of an index in parts: consecutive targets whose anchors fit the budget
// (a target with more runs alone), and per chunk k_mask, the scan, expand(t_lo, A0, B0) — the caller's expanding kernel over the occurrences —,
// the two sorts, the groups, the chains and take (find_chunks).  The figures are added to stats.
template <class Expand, class Take>
int chain_chunks(const OvlStore& S, const OvlParams& P, uint64_t budget_bytes, hipStream_t st, Bufs& B, const RunsOut& RO, OvlStats& stats, std::string& err,
                 Expand expand, Take take) {
  const uint32_t nm = RO.nm;
  const auto per_read_of = [&](uint32_t t) { return (uint64_t)RO.per_read[t - RO.t0]; };
  const bool far = P.lookback != OVL_LOOKBACK;      // (k_chain_far's predecessor distances take two bytes an anchor: one more than k_chain's)
  const uint64_t want = std::max<uint64_t>(budget_bytes / (OVL_ANCHOR_BYTES + (far ? 1 : 0)), 1);
  std::vector<uint32_t> cut{RO.t0};
  uint64_t cap = 0, total = 0;
  {
    uint64_t acc = 0;
    for (uint32_t t = RO.t0; t < RO.t1; t++) {
      if (per_read_of(t) > 0xfffff000ull) { err = "overlap finder: read " + std::to_string(t) + " has more than 2^32 anchors"; return OVL_UNSUPPORTED; }
      if (acc && acc + per_read_of(t) > want) { cut.push_back(t); acc = 0; }
      acc += per_read_of(t);
      total += per_read_of(t);
      cap = std::max(cap, acc);
    }
    cut.push_back(RO.t1);
  }
  stats.anchors += total;
  if (!total) return OVL_OK;
  if (cap > 0xfffff000ull) { err = "overlap finder: more than 2^32 anchors in one chunk (lower HERRO_OVL_SCRATCH_MB)"; return OVL_UNSUPPORTED; }

  uint64_t *A0, *B0, *A1, *B1;
  uint32_t *flag, *gidx, *gstart, *gf, *cidx;
  ChainBufs C{};
  OVL_TRY(B.get(&A0, cap)); OVL_TRY(B.get(&B0, cap)); OVL_TRY(B.get(&A1, cap)); OVL_TRY(B.get(&B1, cap));
  OVL_TRY(B.get(&flag, cap)); OVL_TRY(B.get(&gidx, cap + 1)); OVL_TRY(B.get(&gstart, cap + 1)); OVL_TRY(B.get(&gf, cap));
  OVL_TRY(B.get(&cidx, cap + 1)); OVL_TRY(B.get(&C.cstart, cap)); OVL_TRY(B.get(&C.csize, cap));
  const uint64_t ccap = cap / std::max(1u, P.min_anchors) + 1;     // groups of >= min_anchors anchors
  OVL_TRY(B.get(&C.ck0, ccap)); OVL_TRY(B.get(&C.cp0, ccap)); OVL_TRY(B.get(&C.ck1, ccap)); OVL_TRY(B.get(&C.cp1, ccap));
  if (far) OVL_TRY(B.get(&C.pred16, cap));
  else OVL_TRY(B.get(&C.pred8, cap));
  OVL_TRY(B.get(&C.ends, ccap));
  OVL_TRY(B.get(&C.gout, ccap));
  SortScratch as;
  OVL_TRY(as.alloc(B, cap));
  const uint32_t max_len = RO.max_len;

  for (size_t ch = 0; ch + 1 < cut.size(); ch++) {
    const uint32_t t_lo = cut[ch], t_hi = cut[ch + 1];
    uint64_t na64 = 0;
    for (uint32_t t = t_lo; t < t_hi; t++) na64 += per_read_of(t);
    if (!na64) continue;
    stats.chunks++;
    const uint32_t na = (uint32_t)na64;
    k_mask<<<nblk(nm), 256, 0, st>>>(RO.meta, RO.cnt, nm, t_lo, t_hi, RO.cntm);
    if (int rc = dev_scan_u32(RO.cntm, nm, RO.aoff, RO.scan_partial, st, err)) return rc;
    expand(t_lo, A0, B0);
    OVL_TRY(hipGetLastError());
    {
      std::vector<uint32_t> sa, sb;
      field_shifts(sa, 0, bits_of(max_len));
      field_shifts(sa, 32, bits_of(max_len));
      field_shifts(sb, 0, 1 + bits_of(S.n_reads - 1));
      field_shifts(sb, 33, bits_of(t_hi - t_lo - 1));
      if (int rc = dev_radix_sort(&A0, &B0, &A1, &B1, na, sa, as, st, err)) return rc;     // by (tpos, qpos)
      if (int rc = dev_radix_sort(&B0, &A0, &B1, &A1, na, sb, as, st, err)) return rc;     // then by (t, q, rel), stable
    }
    if (int rc = run_starts(B0, na, flag, gidx, gstart, as.partial, st, err)) return rc;     // the (t, q, rel) groups
    uint32_t ng = 0;
    OVL_TRY(hipMemcpyAsync(&ng, gidx + na, 4, hipMemcpyDeviceToHost, st));
    OVL_TRY(hipStreamSynchronize(st));
    stats.groups += ng;
    k_gflag<<<nblk(ng), 256, 0, st>>>(gstart, ng, P.min_anchors, gf);
    if (int rc = dev_scan_u32(gf, ng, cidx, as.partial, st, err)) return rc;
    uint32_t nc = 0;
    OVL_TRY(hipMemcpyAsync(&nc, cidx + ng, 4, hipMemcpyDeviceToHost, st));
    OVL_TRY(hipStreamSynchronize(st));
    if (!nc) continue;
    stats.chained += nc;
    k_gcompact<<<nblk(ng), 256, 0, st>>>(gstart, gf, cidx, ng, C.cstart, C.csize, C.ck0, C.cp0);
    OVL_TRY(hipGetLastError());
    if (int rc = chain_and_walk(A0, B0, C, nc, P, S.d_base_off, t_lo, as, st, err)) return rc;
    if (int rc = take(nc, C.gout, ccap, t_hi, B)) return rc;
  }
  return OVL_OK;
}

// ---- an index in parts: the host side ("An index in parts") -------------------------------------------------------------
constexpr uint64_t PART_MAX_MINIMIZERS = 0xfffff000ull;      // of one hash range or block pair: 32-bit places
constexpr uint64_t PART_RANGE_FLOOR = 65536;                 // minimizers a hash range may always hold, however small index_kmers is

// What pass A leaves, for the life of the call: the per-read and per-tile tables and occ16.  Block b is the reads cuts[b] .. cuts[b + 1] - 1, its
// tiles tile0[b] .. tile0[b + 1] - 1, its minimizers the ordinals ord0[b] .. ord0[b + 1] - 1; u_at + tile0[b] + b is its slice of the prefix of
// the minimizers per tile (tiles + 1 entries, from 0).
struct PartIndex {
  BufsPeak acct;                                // the bytes of B and of every part's scratch (OvlStats.peak_bytes)
  Bufs B{&acct};
  std::vector<uint64_t> cuts, ord0;
  std::vector<uint32_t> tile0;
  uint32_t n_blocks = 0, max_tiles = 0;
  uint64_t minimizers = 0;
  uint32_t *d_tile_off = nullptr, *d_u_at = nullptr, *d_cnt = nullptr, *d_partial = nullptr;
  uint16_t* d_occ16 = nullptr;
  unsigned long long* d_hist = nullptr;         // [OVL_OCC_BINS] the census of the whole store
  uint64_t* d_occ = nullptr;                    // occ_frac_ppm != 0: {cut, distinct, runs above the cut, minimizers in them} (k_occ_pick)
  uint32_t reads_of(uint32_t b) const { return (uint32_t)(cuts[b + 1] - cuts[b]); }
  uint32_t tiles_of(uint32_t b) const { return tile0[b + 1] - tile0[b]; }
  uint32_t minimizers_of(uint32_t b) const { return (uint32_t)(ord0[b + 1] - ord0[b]); }
};

SketchPart sketch_part_args(const OvlStore& S, const OvlParams& P, const PartIndex& X, uint32_t b) {
  SketchPart a{};
  a.words = S.d_words; a.word_off = S.d_word_off; a.base_off = S.d_base_off; a.tile_off = X.d_tile_off;
  a.r_lo = (uint32_t)X.cuts[b]; a.r_hi = (uint32_t)X.cuts[b + 1]; a.tile0 = X.tile0[b]; a.k = P.k; a.w = P.w;
  a.h_lo = 0; a.h_hi = INF64;
  a.u_at = X.d_u_at + X.tile0[b] + b;
  a.occ16 = X.d_occ16;
  return a;
}

// A count pass of pass A over every block: the minimizers per tile (MODE SKP_COUNT: all of them, SKP_COUNT_RANGE: those with a hash in
// [h_lo, h_hi]), their scan into the block's slice of the per-tile table `at` and, once the stream is synchronised here, tot[b], the block's total.
template <int MODE>
int part_count_pass(const OvlStore& S, const OvlParams& P, hipStream_t st, PartIndex& X, uint32_t* at, uint64_t h_lo, uint64_t h_hi,
                    std::vector<uint32_t>& tot, std::string& err) {
  tot.assign(X.n_blocks, 0);
  for (uint32_t b = 0; b < X.n_blocks; b++) {
    const uint32_t nt = X.tiles_of(b);
    if (!nt) continue;
    SketchPart a = sketch_part_args(S, P, X, b);
    a.h_lo = h_lo; a.h_hi = h_hi; a.cnt = X.d_cnt;
    k_sketch_part<MODE><<<nt, SK_T, 0, st>>>(a);
    OVL_TRY(hipGetLastError());
    if (int rc = dev_scan_u32(X.d_cnt, nt, at + X.tile0[b] + b, X.d_partial, st, err)) return rc;
    OVL_TRY(hipMemcpyAsync(&tot[b], at + X.tile0[b] + b + nt, 4, hipMemcpyDeviceToHost, st));
  }
  OVL_TRY(hipStreamSynchronize(st));
  return OVL_OK;
}

// One hash range [h_lo, h_hi] of pass A.  *n_out: its minimizers; with may_split and more than split_above of them nothing is written (the count
// pass says so first) and *n_out alone comes back.  f_at: a per-tile table like u_at, this range's.
int part_range(const OvlStore& S, const OvlParams& P, hipStream_t st, PartIndex& X, uint32_t* f_at, uint64_t h_lo, uint64_t h_hi, bool may_split,
               uint64_t split_above, uint64_t* n_out, std::string& err) {
  std::vector<uint32_t> ftot;
  if (int rc = part_count_pass<SKP_COUNT_RANGE>(S, P, st, X, f_at, h_lo, h_hi, ftot, err)) return rc;
  uint64_t n64 = 0;
  for (uint32_t v : ftot) n64 += v;
  *n_out = n64;
  if (!n64 || (may_split && n64 > split_above)) return OVL_OK;
  if (n64 > PART_MAX_MINIMIZERS) { err = "overlap finder: a hash range of the occurrence pass holds more than 2^32 - 4096 minimizers (more occ_ranges)"; return OVL_UNSUPPORTED; }
  const uint32_t n = (uint32_t)n64;
  Bufs RB(&X.acct);
  uint64_t *hk0, *hp0, *hk1, *hp1;
  uint32_t *flag, *gidx, *rstart;
  SortScratch ms;
  OVL_TRY(RB.get(&hk0, n)); OVL_TRY(RB.get(&hp0, n)); OVL_TRY(RB.get(&hk1, n)); OVL_TRY(RB.get(&hp1, n));
  OVL_TRY(RB.get(&flag, n)); OVL_TRY(RB.get(&gidx, (uint64_t)n + 1)); OVL_TRY(RB.get(&rstart, (uint64_t)n + 1));
  OVL_TRY(ms.alloc(RB, n));
  uint32_t at = 0;
  for (uint32_t b = 0; b < X.n_blocks; b++) {
    if (!ftot[b]) continue;
    SketchPart a = sketch_part_args(S, P, X, b);
    a.h_lo = h_lo; a.h_hi = h_hi;
    a.f_at = f_at + X.tile0[b] + b;
    a.ord_base = X.ord0[b];
    a.out_base = at;
    a.hash_out = hk0; a.ord_out = hp0;
    k_sketch_part<SKP_WRITE_RANGE><<<X.tiles_of(b), SK_T, 0, st>>>(a);
    at += ftot[b];
  }
  OVL_TRY(hipGetLastError());
  if (int rc = dev_radix_sort(&hk0, &hp0, &hk1, &hp1, n, hash_shifts(P.k), ms, st, err)) return rc;
  if (int rc = run_starts(hk0, n, flag, gidx, rstart, ms.partial, st, err)) return rc;
  k_occ16<<<std::min(nblk(n), OCC_GRID), 256, 0, st>>>(hp0, flag, gidx, rstart, n, X.d_occ16, X.d_hist);
  OVL_TRY(hipGetLastError());
  OVL_TRY(hipStreamSynchronize(st));           // (RB goes with the return)
  return OVL_OK;
}

// The plan and pass A.  stats gains kmers, minimizers, blocks, ranges and, with occ_frac_ppm, the census figures.
int part_index(const OvlStore& S, const OvlParams& P, hipStream_t st, PartIndex& X, OvlStats& stats, std::string& err) {
  if (int rc = check_store(S, err)) return rc;
  if (P.index_kmers > OVL_MAX_KMERS || P.occ_ranges > INDEX_MAX_RANGES) { err = "overlap finder: index_kmers <= 2^32 - 4096, occ_ranges <= 65536"; return OVL_UNSUPPORTED; }
  std::vector<uint64_t> bk;
  index_plan(S.n_reads, S.h_len, P.k, P.w, P.index_kmers, X.cuts, &bk);
  {
    uint64_t bi = 0, bj = 0;
    if (index_plan_overflow(bk, OVL_MAX_KMERS, bi, bj)) { err = index_plan_overflow_text(X.cuts, bi, bj); return OVL_UNSUPPORTED; }
  }
  X.n_blocks = (uint32_t)bk.size();
  stats.blocks = X.n_blocks;
  std::vector<uint32_t> tile_off;
  uint64_t kmers;
  const uint64_t tiles = tile_table(S, P, tile_off, kmers);
  if (tiles + X.n_blocks > 0xfffff000ull) { err = "overlap finder: more than 2^40 k-mers in the read store"; return OVL_UNSUPPORTED; }
  X.tile0.assign((size_t)X.n_blocks + 1, 0);
  for (uint32_t b = 0; b <= X.n_blocks; b++) X.tile0[b] = tile_off[X.cuts[b]];
  for (uint32_t b = 0; b < X.n_blocks; b++) X.max_tiles = std::max(X.max_tiles, X.tiles_of(b));
  stats.kmers = kmers;
  X.ord0.assign((size_t)X.n_blocks + 1, 0);
  if (!tiles) return OVL_OK;
  const uint32_t nt = (uint32_t)tiles;
  OVL_TRY(X.B.get(&X.d_tile_off, (uint64_t)S.n_reads + 1));
  OVL_TRY(X.B.get(&X.d_u_at, (uint64_t)nt + X.n_blocks + 1));
  OVL_TRY(X.B.get(&X.d_cnt, X.max_tiles));
  OVL_TRY(X.B.get(&X.d_partial, nblk(X.max_tiles, SC_TILE) + 2));
  OVL_TRY(X.B.get(&X.d_hist, OVL_OCC_BINS));
  OVL_TRY(X.B.get(&X.d_occ, 4));
  OVL_TRY(hipMemsetAsync(X.d_hist, 0, 8ull * OVL_OCC_BINS, st));
  OVL_TRY(hipMemcpyAsync(X.d_tile_off, tile_off.data(), 4ull * (S.n_reads + 1), hipMemcpyHostToDevice, st));
  std::vector<uint32_t> utot;                   // (the pass ends synchronised: tile_off's copy is done as well)
  if (int rc = part_count_pass<SKP_COUNT>(S, P, st, X, X.d_u_at, 0, INF64, utot, err)) return rc;
  for (uint32_t b = 0; b < X.n_blocks; b++) X.ord0[b + 1] = X.ord0[b] + utot[b];
  X.minimizers = X.ord0[X.n_blocks];
  stats.minimizers = X.minimizers;
  if (!X.minimizers) return OVL_OK;
  OVL_TRY(X.B.bytes(&X.d_occ16, 2 * X.minimizers + 64));

  // the hash ranges: occ_ranges as given, else as many as keep a range near the minimizers of index_kmers k-mers (two per w + 1), split where the
  // count pass finds more than twice that
  const uint64_t space = 1ull << (2 * P.k);     // hashes are below it (INF64 is never selected)
  const uint64_t per_range = std::max<uint64_t>(2 * P.index_kmers / (P.w + 1), PART_RANGE_FLOOR);
  const bool forced = P.occ_ranges != 0;
  const uint64_t R = forced ? P.occ_ranges : std::min<uint64_t>((X.minimizers + per_range - 1) / per_range, INDEX_MAX_RANGES);
  const uint64_t step = (space + R - 1) / R;
  std::vector<std::pair<uint64_t, uint64_t>> todo;
  for (uint64_t lo = 0; lo < space; lo += step) todo.emplace_back(lo, std::min(lo + step, space) - 1);
  uint32_t* f_at;
  OVL_TRY(X.B.get(&f_at, (uint64_t)nt + X.n_blocks + 1));
  while (!todo.empty()) {
    const std::pair<uint64_t, uint64_t> r = todo.back();
    todo.pop_back();
    uint64_t n = 0;
    const bool may_split = !forced && r.first < r.second;
    const uint64_t split_above = std::min<uint64_t>(2 * per_range, PART_MAX_MINIMIZERS);
    if (int rc = part_range(S, P, st, X, f_at, r.first, r.second, may_split, split_above, &n, err)) return rc;
    if (may_split && n > split_above) {
      const uint64_t mid = r.first + (r.second - r.first) / 2;
      todo.emplace_back(mid + 1, r.second);
      todo.emplace_back(r.first, mid);
      continue;
    }
    stats.ranges++;
  }
  if (P.occ_frac_ppm) {
    uint64_t occ[4];
    k_occ_pick<<<1, 256, 0, st>>>(X.d_hist, X.minimizers, P.occ_frac_ppm, P.max_occ, X.d_occ);
    OVL_TRY(hipGetLastError());
    OVL_TRY(hipMemcpyAsync(occ, X.d_occ, sizeof(occ), hipMemcpyDeviceToHost, st));
    OVL_TRY(hipStreamSynchronize(st));
    stats.occ_cut = occ[0]; stats.distinct = occ[1]; stats.cut_runs = occ[2]; stats.cut_minimizers = occ[3];
  } else {
    X.d_occ = nullptr;
  }
  return OVL_OK;
}

// The minimizers of block b behind those already at out_base, in (rid, pos) order, each with its occ from occ16; meta_loc: see k_sketch_part
struct PartSketch { uint64_t *hash, *meta, *meta_loc; uint32_t* occ; };
int part_sketch_block(const OvlStore& S, const OvlParams& P, hipStream_t st, const PartIndex& X, uint32_t b, uint32_t out_base, const PartSketch& K,
                      std::string& err) {
  if (!X.minimizers_of(b)) return OVL_OK;
  SketchPart a = sketch_part_args(S, P, X, b);
  a.ord_base = X.ord0[b];
  a.out_base = out_base;
  a.hash_out = K.hash; a.meta_out = K.meta; a.meta_loc = K.meta_loc; a.occ_out = K.occ;
  k_sketch_part<SKP_WRITE_BLOCK><<<X.tiles_of(b), SK_T, 0, st>>>(a);
  OVL_TRY(hipGetLastError());
  return OVL_OK;
}

// k_rescue over the reads of block b, whose minimizers begin at `at` of the pair's arrays: the kernel of the unpartitioned path, given the block's
// slice, its read ids counted from the block's first read and the offsets from there on.  occ_rp holds occ16's values: the classes and the order
// (occ, pos) among cut < occ <= rmax <= 65534 are those of the true counts.
void part_rescue_block(const OvlStore& S, const OvlParams& P, hipStream_t st, const PartIndex& X, uint32_t b, uint32_t at, const PartSketch& K,
                       uint8_t* resc, unsigned long long* stat) {
  const uint32_t n = X.minimizers_of(b);
  if (!n || !P.occ_dist) return;
  k_rescue<<<X.reads_of(b), 64, 0, st>>>(K.meta_loc + at, K.occ + at, n, S.d_base_off + X.cuts[b], P.max_occ, X.d_occ, P.rescue_max_occ, P.occ_dist,
                                         resc + at, stat);
}

// find_chunks with the index in parts.  reset() comes in front of every block pair: what take keeps in the scratch it is handed is gone by then.
template <class Reset, class Take>
int find_parts(const OvlStore& S, const OvlParams& P, const uint8_t* d_core, uint64_t budget_bytes, hipStream_t st, OvlStats& stats, std::string& err,
               Reset reset, Take take) {
  PartIndex X;
  const int rc_all = synced_on_failure(st, [&]() -> int {
    if (int rc = part_index(S, P, st, X, stats, err)) return rc;
    const bool frac = P.occ_frac_ppm != 0, rescue = P.occ_dist != 0;
    if (!frac || X.minimizers < 2) stats_without_census(stats, X.minimizers, P);     // (else part_index has left the pick's figures)
    if (X.minimizers < 2) return OVL_OK;
    const uint32_t max_len = max_read_len(S);
    std::vector<uint8_t> has_core(X.n_blocks, 1);
    if (d_core) {
      std::vector<uint8_t> core(S.n_reads);
      OVL_TRY(hipMemcpyAsync(core.data(), d_core, S.n_reads, hipMemcpyDeviceToHost, st));
      OVL_TRY(hipStreamSynchronize(st));
      for (uint32_t b = 0; b < X.n_blocks; b++) {
        has_core[b] = 0;
        for (uint64_t r = X.cuts[b]; r < X.cuts[b + 1] && !has_core[b]; r++) has_core[b] = core[r] != 0;
      }
    }
    for (uint32_t bi = 0; bi < X.n_blocks; bi++) {
      for (uint32_t bj = bi; bj < X.n_blocks; bj++) {
        // a pair of two blocks without a core read has no wanted anchor; a block with itself always runs: the rescue's figures are counted there
        if (bj > bi && !has_core[bi] && !has_core[bj]) continue;
        const uint32_t ni = X.minimizers_of(bi), nj = bj > bi ? X.minimizers_of(bj) : 0;
        if (!ni || (bj > bi && !nj)) continue;
        stats.block_pairs++;
        reset();
        const uint32_t nm = ni + nj;            // (the plan keeps the k-mers of a pair, so its minimizers, within 2^32 - 4096)
        const uint32_t t0 = (uint32_t)X.cuts[bi], t1 = (uint32_t)X.cuts[bi + 1], split = bj > bi ? (uint32_t)X.cuts[bj] : 0u;
        Bufs B(&X.acct);
        PartSketch K{};
        uint8_t *resc = nullptr, *cls, *cls_s;
        uint64_t *idx, *k1, *p1, *meta_s;
        uint32_t *d_cnt, *d_run_end, *d_cntm, *d_aoff;
        unsigned long long *d_per_read, *d_stat;
        SortScratch ms;
        OVL_TRY(B.get(&K.hash, nm)); OVL_TRY(B.get(&K.meta, nm)); OVL_TRY(B.get(&K.occ, nm));
        if (rescue) { OVL_TRY(B.get(&K.meta_loc, nm)); OVL_TRY(B.get(&resc, nm)); }
        OVL_TRY(B.get(&cls, nm)); OVL_TRY(B.get(&cls_s, nm)); OVL_TRY(B.get(&idx, nm)); OVL_TRY(B.get(&k1, nm)); OVL_TRY(B.get(&p1, nm));
        OVL_TRY(B.get(&meta_s, nm));
        OVL_TRY(B.get(&d_cnt, nm)); OVL_TRY(B.get(&d_run_end, nm)); OVL_TRY(B.get(&d_cntm, nm)); OVL_TRY(B.get(&d_aoff, (uint64_t)nm + 1));
        OVL_TRY(B.get(&d_per_read, t1 - t0));
        OVL_TRY(B.get(&d_stat, 6));             // {H minimizers, rescued, anchors of the runs above the cut}, and the same of a block counted before
        OVL_TRY(ms.alloc(B, nm));
        OVL_TRY(hipMemsetAsync(d_cnt, 0, 4ull * nm, st));
        OVL_TRY(hipMemsetAsync(d_per_read, 0, 8ull * (t1 - t0), st));
        OVL_TRY(hipMemsetAsync(d_stat, 0, 48, st));
        if (int rc = part_sketch_block(S, P, st, X, bi, 0, K, err)) return rc;
        if (bj > bi) if (int rc = part_sketch_block(S, P, st, X, bj, ni, K, err)) return rc;
        if (rescue) {
          OVL_TRY(hipMemsetAsync(resc, 0, nm, st));
          part_rescue_block(S, P, st, X, bi, 0, K, resc, bj == bi ? d_stat : d_stat + 3);
          if (bj > bi) part_rescue_block(S, P, st, X, bj, ni, K, resc, d_stat + 3);
        }
        k_part_cls<<<nblk(nm), 256, 0, st>>>(K.occ, resc, nm, P.max_occ, X.d_occ, rescue ? P.rescue_max_occ : 0u, cls, idx);
        OVL_TRY(hipGetLastError());
        if (int rc = dev_radix_sort(&K.hash, &idx, &k1, &p1, nm, hash_shifts(P.k), ms, st, err)) return rc;
        k_part_gather<<<nblk(nm), 256, 0, st>>>(idx, K.meta, cls, nm, meta_s, cls_s);
        with_core(d_core, [&](auto core) {
          k_part_runs<decltype(core)::value><<<nblk(nm), 256, 0, st>>>(K.hash, meta_s, cls_s, nm, split, t0, d_cnt, d_run_end, d_per_read, d_core, d_stat);
        });
        OVL_TRY(hipGetLastError());
        std::vector<unsigned long long> per_read(t1 - t0);
        unsigned long long resc_stat[3] = {0, 0, 0};
        OVL_TRY(hipMemcpyAsync(per_read.data(), d_per_read, 8ull * (t1 - t0), hipMemcpyDeviceToHost, st));
        OVL_TRY(hipMemcpyAsync(resc_stat, d_stat, sizeof(resc_stat), hipMemcpyDeviceToHost, st));
        OVL_TRY(hipStreamSynchronize(st));
        if (rescue) { stats.resc_high += resc_stat[0]; stats.rescued += resc_stat[1]; stats.resc_anchors += resc_stat[2]; }
        const RunsOut RO{meta_s, nm, d_cnt, d_run_end, d_cntm, d_aoff, ms.partial, per_read.data(), t0, t1, max_len};
        if (int rc = chain_chunks(S, P, budget_bytes, st, B, RO, stats, err, [&](uint32_t t_lo, uint64_t* A0, uint64_t* B0) {
          with_core(d_core, [&](auto core) {
            k_part_expand<decltype(core)::value><<<nblk(nm), 256, 0, st>>>(meta_s, cls_s, d_cntm, d_run_end, d_aoff, nm, split, S.d_base_off, P.k, t_lo, A0,
                                                                           B0, d_core);
          });
        }, take)) return rc;
        OVL_TRY(hipStreamSynchronize(st));     // (B goes with the pair: nothing of it is still read)
      }
    }
    return OVL_OK;
  });
  stats.peak_bytes = X.acct.peak;
  return rc_all;
}

// ovl_find and ovl_find_pairs behind their take: the whole store's index, or (index_kmers != 0) an index in parts, where reset() comes in front of
// every block pair.
template <class Reset, class Take>
int find_overlaps(const OvlStore& S, const OvlParams& P, const uint8_t* d_core, uint64_t budget_bytes, hipStream_t st, OvlStats& stats, std::string& err,
                  Reset reset, Take take) {
  stats = OvlStats{};
  if (!lookback_ok(P.lookback, err)) return OVL_UNSUPPORTED;
  if (!P.index_kmers) return find_chunks(S, P, d_core, budget_bytes, st, stats, err, take);
  return find_parts(S, P, d_core, budget_bytes, st, stats, err, reset, take);
}
}  // namespace

int ovl_occ_census(const OvlStore& S, const OvlParams& P, hipStream_t st, std::vector<uint32_t>* hist, uint64_t rec[4], std::string& err) {
  if (P.index_kmers) {                          // pass A alone; a bin beyond 32 bits is reported as 2^32 - 1
    PartIndex X;
    OvlStats stats;
    if (int rc = part_index(S, P, st, X, stats, err)) { (void)hipStreamSynchronize(st); return rc; }
    if (hist) hist->assign(OVL_OCC_BINS, 0);
    rec[0] = X.minimizers ? stats.occ_cut : occ_final_cut(0, P.max_occ);
    rec[1] = stats.distinct; rec[2] = stats.cut_runs; rec[3] = stats.cut_minimizers;
    if (hist && X.minimizers) {
      std::vector<unsigned long long> h64(OVL_OCC_BINS);
      OVL_TRY(hipMemcpyAsync(h64.data(), X.d_hist, 8ull * OVL_OCC_BINS, hipMemcpyDeviceToHost, st));
      OVL_TRY(hipStreamSynchronize(st));
      for (uint32_t b = 0; b < OVL_OCC_BINS; b++) (*hist)[b] = (uint32_t)std::min<unsigned long long>(h64[b], 0xffffffffull);
    }
    return OVL_OK;
  }
  Bufs B;
  StoreIndex X;
  if (int rc = store_index(S, P, true, false, 1, st, B, X, err)) return rc;
  if (hist) hist->assign(OVL_OCC_BINS, 0);
  rec[0] = occ_final_cut(0, P.max_occ);
  rec[1] = rec[2] = rec[3] = 0;
  if (!X.built) { OVL_TRY(hipStreamSynchronize(st)); return OVL_OK; }
  if (hist) OVL_TRY(hipMemcpyAsync(hist->data(), X.d_hist, 4ull * OVL_OCC_BINS, hipMemcpyDeviceToHost, st));
  OVL_TRY(hipMemcpyAsync(rec, X.d_occ, 32, hipMemcpyDeviceToHost, st));
  OVL_TRY(hipStreamSynchronize(st));
  return OVL_OK;
}

int ovl_seed_rescue(const OvlStore& S, const OvlParams& P, hipStream_t st, std::vector<uint32_t>& occ, std::vector<uint8_t>& rescued, std::string& err) {
  if (P.index_kmers) {                          // pass A, then block by block: its sketch, occ from occ16, k_rescue
    PartIndex X;
    OvlStats stats;
    return synced_on_failure(st, [&]() -> int {
      if (int rc = part_index(S, P, st, X, stats, err)) return rc;
      occ.assign(X.minimizers, 1);
      rescued.assign(X.minimizers, 0);
      for (uint32_t b = 0; b < X.n_blocks; b++) {
        const uint32_t n = X.minimizers_of(b);
        if (!n) continue;
        Bufs B(&X.acct);
        PartSketch K{};
        uint8_t* resc;
        unsigned long long* stat;
        OVL_TRY(B.get(&K.hash, n)); OVL_TRY(B.get(&K.meta, n)); OVL_TRY(B.get(&K.meta_loc, n)); OVL_TRY(B.get(&K.occ, n));
        OVL_TRY(B.get(&resc, n)); OVL_TRY(B.get(&stat, 3));
        OVL_TRY(hipMemsetAsync(resc, 0, n, st));
        OVL_TRY(hipMemsetAsync(stat, 0, 24, st));
        if (int rc = part_sketch_block(S, P, st, X, b, 0, K, err)) return rc;
        part_rescue_block(S, P, st, X, b, 0, K, resc, stat);
        OVL_TRY(hipGetLastError());
        OVL_TRY(hipMemcpyAsync(occ.data() + X.ord0[b], K.occ, 4ull * n, hipMemcpyDeviceToHost, st));
        OVL_TRY(hipMemcpyAsync(rescued.data() + X.ord0[b], resc, n, hipMemcpyDeviceToHost, st));
        OVL_TRY(hipStreamSynchronize(st));
      }
      return OVL_OK;
    });
  }
  Bufs B;
  StoreIndex X;
  if (int rc = store_index(S, P, P.occ_frac_ppm != 0, true, 2, st, B, X, err)) return rc;
  const uint32_t n = X.sk.n;
  occ.assign(n, 1);
  rescued.assign(n, 0);
  if (!X.built) { OVL_TRY(hipStreamSynchronize(st)); return OVL_OK; }
  OVL_TRY(hipMemcpyAsync(occ.data(), X.occ_rp, 4ull * n, hipMemcpyDeviceToHost, st));
  OVL_TRY(hipMemcpyAsync(rescued.data(), X.resc_rp, n, hipMemcpyDeviceToHost, st));
  OVL_TRY(hipStreamSynchronize(st));
  for (uint32_t& c : occ) c = std::min(c, OVL_OCC_BINS - 1);
  return OVL_OK;
}

int ovl_find(const OvlStore& S, const OvlParams& P, const uint8_t* d_core, uint64_t budget_bytes, hipStream_t st, std::vector<OvlPair>& out,
             OvlStats& stats, std::string& err) {
  out.clear();
  std::vector<GroupOut> h_out;
  const auto take = [&](uint32_t nc, const GroupOut* gout, uint64_t, uint32_t, Bufs&) -> int {
    h_out.resize(nc);
    OVL_TRY(hipMemcpyAsync(h_out.data(), gout, sizeof(GroupOut) * (uint64_t)nc, hipMemcpyDeviceToHost, st));
    OVL_TRY(hipStreamSynchronize(st));
    for (const GroupOut& g : h_out)
      if (g.kept) out.push_back(OvlPair{g.t, g.q, g.rel, g.n_anchors, g.score, g.tstart, g.tend, g.qstart, g.qend});
    return OVL_OK;
  };
  if (int rc = find_overlaps(S, P, d_core, budget_bytes, st, stats, err, [] {}, take)) return rc;
  // an index in parts of several blocks: a target's chains come pair by pair, (i, i), (i, i + 1), ... — in ascending q, every (t, q) in one pair; the
  // stable sort by t gives ascending (t, q, rel)
  if (stats.blocks > 1) std::stable_sort(out.begin(), out.end(), [](const OvlPair& a, const OvlPair& b) { return a.t < b.t; });
  return OVL_OK;
}

// The chain stage alone on the caller's groups (herro_debug_chain).  The keys k_walk decodes are those of target 0, query 0, forward strand, whose
// length it then does not ask for; it leaves the first anchor's coordinates, and the keys of a group are strictly ascending: its index is looked up.
int ovl_chain_groups(uint64_t n_groups, const uint64_t* group_off, const uint32_t* tpos, const uint32_t* qpos, const OvlParams& P, hipStream_t st,
                     int32_t* out, std::string& err) {
  if (!lookback_ok(P.lookback, err)) return OVL_UNSUPPORTED;
  if (!n_groups) return OVL_OK;
  const uint32_t nc = (uint32_t)n_groups;
  const uint64_t na = group_off[n_groups];
  std::vector<uint64_t> hA(na), key(nc), pay(nc);
  std::vector<uint32_t> start(nc), size(nc);
  for (uint64_t i = 0; i < na; i++) hA[i] = (uint64_t)tpos[i] << 32 | qpos[i];
  for (uint32_t g = 0; g < nc; g++) {           // (what k_gcompact leaves)
    start[g] = (uint32_t)group_off[g];
    size[g] = (uint32_t)(group_off[g + 1] - group_off[g]);
    key[g] = 0xffffffffu - size[g];
    pay[g] = g;
  }
  Bufs B;
  uint64_t *A0, *B0, *d_base_off;
  ChainBufs C{};
  OVL_TRY(B.get(&A0, na)); OVL_TRY(B.get(&B0, na)); OVL_TRY(B.get(&d_base_off, 2));
  OVL_TRY(B.get(&C.cstart, nc)); OVL_TRY(B.get(&C.csize, nc));
  OVL_TRY(B.get(&C.ck0, nc)); OVL_TRY(B.get(&C.cp0, nc)); OVL_TRY(B.get(&C.ck1, nc)); OVL_TRY(B.get(&C.cp1, nc));
  if (P.lookback != OVL_LOOKBACK) OVL_TRY(B.get(&C.pred16, na));
  else OVL_TRY(B.get(&C.pred8, na));
  OVL_TRY(B.get(&C.ends, nc));
  OVL_TRY(B.get(&C.gout, nc));
  SortScratch as;
  OVL_TRY(as.alloc(B, nc));
  OVL_TRY(hipMemcpyAsync(A0, hA.data(), 8 * na, hipMemcpyHostToDevice, st));
  OVL_TRY(hipMemsetAsync(B0, 0, 8 * na, st));
  OVL_TRY(hipMemsetAsync(d_base_off, 0, 16, st));
  OVL_TRY(hipMemcpyAsync(C.cstart, start.data(), 4ull * nc, hipMemcpyHostToDevice, st));
  OVL_TRY(hipMemcpyAsync(C.csize, size.data(), 4ull * nc, hipMemcpyHostToDevice, st));
  OVL_TRY(hipMemcpyAsync(C.ck0, key.data(), 8ull * nc, hipMemcpyHostToDevice, st));
  OVL_TRY(hipMemcpyAsync(C.cp0, pay.data(), 8ull * nc, hipMemcpyHostToDevice, st));
  if (int rc = chain_and_walk(A0, B0, C, nc, P, d_base_off, 0, as, st, err)) { (void)hipStreamSynchronize(st); return rc; }
  std::vector<GroupOut> h_out(nc);
  std::vector<ChainEnd> h_ends(nc);
  OVL_TRY(hipMemcpyAsync(h_out.data(), C.gout, sizeof(GroupOut) * (uint64_t)nc, hipMemcpyDeviceToHost, st));
  OVL_TRY(hipMemcpyAsync(h_ends.data(), C.ends, sizeof(ChainEnd) * (uint64_t)nc, hipMemcpyDeviceToHost, st));
  OVL_TRY(hipStreamSynchronize(st));
  for (uint32_t g = 0; g < nc; g++) {
    const GroupOut& o = h_out[g];
    const uint64_t first_key = (uint64_t)(o.tstart + P.k - 1) << 32 | (uint32_t)(o.qstart + P.k - 1);
    const uint64_t* a = hA.data() + start[g];
    out[4 * g] = o.score;
    out[4 * g + 1] = (int32_t)(std::lower_bound(a, a + size[g], first_key) - a);
    out[4 * g + 2] = (int32_t)h_ends[g].last;
    out[4 * g + 3] = (int32_t)o.n_anchors;
  }
  return OVL_OK;
}

// ---- one overlap per pair and the row table, on the device ("Pairs on the device") ---------------------------------------
int ovl_find_pairs(const OvlStore& S, const OvlParams& P, const uint8_t* d_core, uint64_t budget_bytes, hipStream_t st, OvlRecs& out, OvlStats& stats,
                   std::string& err) {
  out.release();
  uint32_t *sel = nullptr, *soff = nullptr, *part = nullptr;
  const auto take = [&](uint32_t nc, const GroupOut* gout, uint64_t ccap, uint32_t t_hi, Bufs& B) -> int {
    if (!sel) {
      OVL_TRY(B.get(&sel, ccap));
      OVL_TRY(B.get(&soff, ccap + 1));
      OVL_TRY(B.get(&part, (uint64_t)nblk(ccap, SC_TILE) + 2));
    }
    k_pick<<<nblk(nc), 256, 0, st>>>(gout, nc, sel);
    if (int rc2 = dev_scan_u32(sel, nc, soff, part, st, err)) return rc2;
    uint32_t ns = 0;
    OVL_TRY(hipMemcpyAsync(&ns, soff + nc, 4, hipMemcpyDeviceToHost, st));
    OVL_TRY(hipStreamSynchronize(st));
    if (!ns) return OVL_OK;
    if (out.n + ns > OVL_MAX_PAIRS) { err = "overlap finder: more than 2^31 - 1 overlapping read pairs"; return OVL_UNSUPPORTED; }
    // The array grows by chunks as the aligner's op store does: the first chunk's primaries per target, projected over all targets plus an eighth,
    // size it; a chunk that does not fit moves it to twice the projection (behind the synchronisation above: nothing is writing the old block).
    if (out.n + ns > out.cap) {
      const uint64_t proj = (out.n + ns) * (uint64_t)S.n_reads / std::max(t_hi, 1u);
      const uint64_t cap = std::max<uint64_t>(out.n + ns, (out.cap ? 2 : 1) * (proj + proj / 8)) + 1024;
      OvlRec* d = nullptr;
      OVL_TRY(hipMalloc((void**)&d, cap * sizeof(OvlRec)));
      OvlRec* const old = out.d;
      out.d = d; out.cap = cap;
      hipError_t e = out.n ? hipMemcpyAsync(d, old, out.n * sizeof(OvlRec), hipMemcpyDeviceToDevice, st) : hipSuccess;
      if (old) {
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        (void)hipFree(old);
      }
      OVL_TRY(e);
    }
    k_prim_write<<<nblk(nc), 256, 0, st>>>(gout, sel, soff, nc, S.d_base_off, out.d + out.n);
    OVL_TRY(hipGetLastError());
    out.n += ns;
    return OVL_OK;
  };
  // an index in parts: the scratch of a block pair goes with the pair, and so does what take keeps in it; the records of several blocks are then
  // put into target order
  if (int rc = find_overlaps(S, P, d_core, budget_bytes, st, stats, err, [&] { sel = soff = part = nullptr; }, take)) return rc;
  OVL_TRY(hipStreamSynchronize(st));
  return stats.blocks < 2 ? OVL_OK : ovl_sort_recs(out, S.n_reads, st, err);
}

}  // namespace herro
