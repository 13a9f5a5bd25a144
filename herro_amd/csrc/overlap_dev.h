// overlap_dev.h — which reads overlap, where, on which strand (overlap_dev.hip; the row table: overlap_rows.hip): the GPU counterpart of the seeding and chaining
// half of the `minimap2 -x ava-ont` run that `herro inference` starts without --read-alns (mm2.rs:15-30, overlaps.rs:340-344).
// Minimizer sketch of the resident 2-bit store, radix sort by hash, frequency cut, anchor expansion, radix sort by
// (t, q, rel, tpos, qpos), one wave64 per (t, q, rel) group for the chain.  The specification is DESIGN.md §10 and
// tests/overlap_ref.py; the kernels equal it bit for bit, whatever the scratch budget.
// The frequency cut is max_occ, or — occ_frac_ppm != 0, minimap2's -f — taken from the store's own index: the census of the run lengths
// and the pick of DESIGN.md §10, "The cut as a fraction" (tests/occ_ref.py), two kernels between the sort and k_runs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

namespace herro {

constexpr uint32_t OVL_LOOKBACK = 64;          // predecessors a chain step looks at: the lanes of a wave
constexpr uint32_t OVL_MAX_LOOKBACK = 1024;    // ... at most, in multiples of 64, where OvlParams.lookback asks for more (k_chain_far: 64 a round)
constexpr uint64_t OVL_ANCHOR_BYTES = 128;     // scratch the budget charges per anchor of a chunk (keys, payloads, both sort buffers, groups)
constexpr uint64_t OVL_MAX_KMERS = 0xfffff000ull;   // k-mers of the whole store (32-bit minimizer indices)
constexpr uint32_t OVL_MAX_READ_LEN = 0x7fffffffu;  // pos << 1 | strand is one 32-bit field
constexpr uint32_t OVL_MAX_READS = 0x7fffffffu;     // q << 1 | rel is one 33-bit field of the anchor key

// defaults already filled in.  occ_frac_ppm 0: runs longer than max_occ are dropped.  Else the cut is the census's (ovl_occ_census) and max_occ
// its ceiling, 0 = none.  With index_kmers != 0 ovl_occ_census, ovl_seed_rescue, ovl_find and ovl_find_pairs take the occurrences from a pass
// over hash ranges and run per pair of read blocks; what they return is what they return without it (ovl_sketch and ovl_chain_groups ignore it).
// occ_dist != 0: the rescue of high-frequency minimizers (minimap2's -e, mm2.rs:24) — of a stretch of a read whose minimizers all lie
// above the cut, the least frequent ones stay, about one per occ_dist bases, among those of at most rescue_max_occ occurrences (filled in: never 0).
// lookback: the predecessors a chain step looks at, a multiple of 64 in 64 .. OVL_MAX_LOOKBACK ("A longer look-back"); 64 runs
// k_chain and everything else as it was, any other value k_chain_far.
// index_kmers != 0: the index is built in parts ("An index in parts"; herro_set_index_params) — the most k-mers one index of the call
// covers, at most OVL_MAX_KMERS; occ_ranges: the hash ranges of the occurrence pass, 0 = chosen here.  0 runs everything as it was.
struct OvlParams {
  uint32_t k, w, max_occ, bandwidth, max_gap, min_score, min_anchors, occ_frac_ppm, occ_dist = 0, rescue_max_occ = 0, lookback = OVL_LOOKBACK;
  uint64_t index_kmers = 0;
  uint32_t occ_ranges = 0;
};

constexpr uint32_t OVL_OCC_BINS = 65536;       // census counts of a hash run: min(length, 65535)
constexpr uint32_t OVL_OCC_FLOOR = 10;         // the least cut the fraction may give (minimap2's min_mid_occ)

struct OvlStore {            // the context's read store
  const uint64_t* d_words;      // 2-bit codes, 32 bases per word (+ one pad word)
  const uint64_t* d_word_off;   // [n_reads + 1] first word of a read
  const uint64_t* d_base_off;   // [n_reads + 1] first base of a read (its length by difference)
  const uint32_t* h_len;        // host: read lengths
  uint32_t n_reads;
};

struct OvlPair {             // one kept chain, t < q, forward coordinates on both reads
  uint32_t t, q, rel, n_anchors;
  int32_t score;
  uint32_t tstart, tend, qstart, qend;
};

struct OvlStats {
  uint64_t kmers = 0, minimizers = 0, anchors = 0, groups = 0, chained = 0, chunks = 0;
  uint64_t occ_cut = 0;                                       // the cut the call used: max_occ, or the census's
  uint64_t distinct = 0, cut_runs = 0, cut_minimizers = 0;    // occ_frac_ppm != 0: hash runs of the index, those above the cut, their minimizers
  uint64_t resc_high = 0, rescued = 0, resc_anchors = 0;      // occ_dist != 0: minimizers between the cut and rescue_max_occ, the rescued, the anchors of their runs
  // index_kmers != 0: the read blocks, the block pairs run, the hash ranges run, the most device scratch the call held at once.  The figures above
  // are then the sums over the parts and equal the unpartitioned call's, chunks excepted.
  uint64_t blocks = 0, block_pairs = 0, ranges = 0, peak_bytes = 0;
};

enum { OVL_OK = 0, OVL_HIP = 1, OVL_UNSUPPORTED = 2 };   // (the scan and the sort the finder runs on are scan_sort_dev.h's: 0 / 1 there too)

// for the finder's own units (overlap_dev.hip, overlap_rows.hip): a failed HIP call ends the function with OVL_HIP and its text in `err`
#define OVL_TRY(expr)                                                                  \
  do {                                                                                 \
    const hipError_t _e = (expr);                                                      \
    if (_e != hipSuccess) {                                                            \
      err = std::string("overlap finder: " #expr ": ") + hipGetErrorString(_e);        \
      return OVL_HIP;                                                                  \
    }                                                                                  \
  } while (0)

// minimizers of the whole store sorted by (rid, pos): hash[i], meta[i] = rid << 32 | pos << 1 | strand (host vectors)
int ovl_sketch(const OvlStore& S, const OvlParams& P, hipStream_t st, std::vector<uint64_t>& hash, std::vector<uint64_t>& meta,
               std::string& err);

// The census and the pick alone (occ_frac_ppm != 0): rec = {cut, distinct hashes, runs above the cut, minimizers in them}; hist (or NULL): the
// OVL_OCC_BINS bins of min(run length, 65535).
int ovl_occ_census(const OvlStore& S, const OvlParams& P, hipStream_t st, std::vector<uint32_t>* hist, uint64_t rec[4], std::string& err);

// The rescue alone, for the minimizers in ovl_sketch's order: occ = min(occurrences of the hash in the store, 65535), rescued = 1 where the rule of
// DESIGN.md §10, "Rescue of high-frequency minimizers" (tests/rescue_ref.py) keeps a minimizer above the cut.  occ_dist 0: no flag is set.
int ovl_seed_rescue(const OvlStore& S, const OvlParams& P, hipStream_t st, std::vector<uint32_t>& occ, std::vector<uint8_t>& rescued, std::string& err);

// every kept (t, q) chain per strand, ascending (t, q, rel); the caller picks the strand and writes the dual records
// d_core (here and below): NULL — every read is a target — or the core mask on the device, n_reads bytes, non-zero = core (the PAF
// entries' `core`: overlaps.rs:154-159).  No anchor is created between two non-core reads (k_runs, k_expand), so the sorts, the chains and
// all behind them see only pairs with a core read; the frequency cut stays the whole store's, chains are independent per (t, q, rel), and the
// result is therefore the unmasked one restricted to those pairs.  OvlStats.anchors and the limits count the masked anchors.
int ovl_find(const OvlStore& S, const OvlParams& P, const uint8_t* d_core, uint64_t budget_bytes, hipStream_t st, std::vector<OvlPair>& out,
             OvlStats& stats, std::string& err);

// The chain stage alone on anchor groups the caller gives (herro_debug_chain): group g is tpos / qpos [group_off[g], group_off[g + 1]), not empty,
// strictly ascending by (tpos, qpos), coordinates below 2^31, fewer than 2^31 anchors in all (the caller has checked all that).  Runs what a
// chunk of ovl_find runs behind k_gcompact — the groups ordered largest first, k_chain or k_chain_far by P.lookback, k_walk — and leaves
// out[g] = {score, first anchor, last anchor, anchors in the chain}: tests/overlap_ref.py::chain.  Of P it reads k, bandwidth, max_gap, lookback.
int ovl_chain_groups(uint64_t n_groups, const uint64_t* group_off, const uint32_t* tpos, const uint32_t* qpos, const OvlParams& P, hipStream_t st,
                     int32_t* out, std::string& err);

// ---- one overlap per pair, left on the device ("Pairs on the device") -------------------------------------------------------
constexpr uint64_t OVL_MAX_PAIRS = 0x7fffffffull;   // the mirror's record limit; 2 P rows stay inside the sort's 32-bit count

struct OvlRec {              // one overlap in herro_alignment's field order (40 B): query q on target t, t < q
  uint32_t qid, qlen, qstart, qend, strand, tid, tlen, tstart, tend;
  int32_t score;                // chain score
};

struct OvlRecs {             // a device array of records; it owns its memory
  OvlRec* d = nullptr;
  uint64_t n = 0, cap = 0;
  OvlRecs() = default;
  OvlRecs(const OvlRecs&) = delete;
  OvlRecs& operator=(const OvlRecs&) = delete;
  void release() { if (d) (void)hipFree(d); d = nullptr; n = cap = 0; }
  ~OvlRecs() { release(); }
};

// ovl_find with the strand choice on the device: the better strand of every pair (forward on a tie) as one record, in ascending
// (t, q) order — the primaries of api.pair_rows over herro_find_overlaps' records.  The host reads one count per chunk.
int ovl_find_pairs(const OvlStore& S, const OvlParams& P, const uint8_t* d_core, uint64_t budget_bytes, hipStream_t st, OvlRecs& out,
                   OvlStats& stats, std::string& err);

// ---- overlap_rows.hip: what needs only the records and the shared scan and sort ------------------------------------------------------------------
// The records of all block pairs of an index in parts into target order, stably: ovl_find_pairs' last step there (n_reads bounds the target ids).
int ovl_sort_recs(OvlRecs& R, uint32_t n_reads, hipStream_t st, std::string& err);

// The 2 P rows herro_find_overlaps emits for P primaries — (t, q) and (q, t) of each, by (tid, qid) — as a table: rids / aln_off group
// them by target, rec_of_row[i] is p for the row that is primary p and P + p for its mirror.  Sorted and grouped on the device.
// With d_core only the rows whose target is core: one or two per primary, rec_of_row.size() <= 2 P.
int ovl_row_table(const OvlRecs& R, uint32_t n_reads, const uint8_t* d_core, hipStream_t st, std::vector<uint32_t>& rids,
                  std::vector<uint64_t>& aln_off, std::vector<uint32_t>& rec_of_row, std::string& err);

}  // namespace herro
