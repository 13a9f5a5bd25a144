// fasta_dev.h — the corrected reads of a job as FASTA text formed on the device (fasta_dev.hip; specification: DESIGN.md §15, tests/chop_ref.py,
// the rule and the byte counts in chop_plan.h).  It stands for two things at once: the host assembly of herro_job_fasta (consensus.rs:90-111 picks
// the corrected windows, lib.rs:282-317 names and writes the records) and scripts/postprocess_corrected.sh of the reference's workflow
// (`seqkit sliding -s 30000 -W 30000 -g`, then `seqkit seq -m 10000`): the records are segmented, chopped, filtered, named and written where the
// consensus kernel left the bases, and the host receives finished text.
//   record   '>' id [':' i] ["_sliding:" start+1 '-' end] ' ' [desc] '\n' bases ['\n' behind every line_width of them] '\n'
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <functional>
#include <string>
#include <vector>

#include "chop_plan.h"
#include "job_dev.h"

namespace herro {

constexpr uint64_t FASTA_MAX_ROW_ELEMS = 0xffffffffull;   // window slots of a job: base prefixes, piece counts and the scans under them are 32-bit
constexpr uint64_t FASTA_DEFAULT_CHUNK = 64ull << 20;     // text bytes of a chunk at the default budget (a sixteenth of HERRO_FASTA_SCRATCH_MB = 1024)

struct FastaNames {                   // what the headers are written from: target t's id is blob[off[2t], off[2t+1]), its description blob[off[2t+1], off[2t+2])
  std::string blob;
  std::vector<uint64_t> off;          // [2 * n_targets + 1]
  std::vector<uint8_t> present;       // [n_targets]: 0 = ids[t] was NULL, the target gives nothing
};

struct FastaStats {
  uint64_t records = 0, bases = 0, dropped = 0, bases_dropped = 0, segments = 0, targets = 0;   // herro_fasta_text_stats, in its order
  uint64_t n_targets = 0, bytes = 0, chunks = 0;
  double seg_ms = 0, piece_ms = 0, write_ms = 0;                                               // host clock around the stages (each ends in a wait)
};

enum { FASTA_OK = 0, FASTA_HIP = 1 };

// Where the call's memory comes from.  hipMalloc and hipHostMalloc synchronise the device and cost more than every kernel here together, so the
// caller hands out recycled blocks: dev(bytes) a device block (256-byte aligned; at most three per call), text(bytes) the pinned host block the
// text is copied into.  nullptr: out of memory.  The blocks are the caller's again when the call has returned (the stream is idle then).
struct FastaMem {
  std::function<void*(uint64_t)> dev;
  std::function<char*(uint64_t)> text;
};

// The text of the job's n_targets targets into *text = mem.text(*text_len), the end offset of every target's records into target_end (*text stays
// NULL for an empty text).  J: a job whose consensus pass is queued or done on st (cons_seq, cons_len, win_nkept, win); tgt_win_off: host,
// [n_targets + 1]; row_elems <= FASTA_MAX_ROW_ELEMS: the size of J.cons_seq.  chunk: text bytes formed at a time (a multiple of 16 is made of
// it) in one of two device halves, each copied to its place in the pinned block behind its kernel.  The bytes do not depend on it.  Returns
// when the text is on the host; FASTA_HIP: err names the call that failed, and the stream is idle.
int fasta_text_dev(const JobDev& J, uint64_t row_elems, const uint32_t* tgt_win_off, uint32_t n_targets, const FastaNames& names, const ChopRule& R,
                   uint64_t chunk, hipStream_t st, const FastaMem& mem, char** text, uint64_t* text_len, std::vector<uint64_t>& target_end,
                   FastaStats& stats, std::string& err);

// The 64-bit offset join of the pieces as fasta_text_dev runs it, on arrays of the caller's (the test hook herro_debug_offsets64): piece p has
// lo_in[p] + 2^32 hi_in[p] bytes; off[0 .. n] are the running sums, off[n] the total.  The low words are scanned modulo 2^32 into lo, a piece at
// which that prefix falls adds a carry to its hi_in (which is changed), the high words are scanned into hi, off joins them.  All on the device:
// lo_in, hi_in [n], lo, hi, off [n + 1], partial [dev_scan_partials(n)].  Exact while the total is below 2^64.  Queued on st; nothing is awaited.
int fasta_offsets64(uint32_t* lo_in, uint32_t* hi_in, uint32_t n, uint32_t* lo, uint32_t* hi, uint64_t* off, uint32_t* partial, hipStream_t st,
                    std::string& err);

}  // namespace herro
