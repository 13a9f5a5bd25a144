// paf_dev.h — PAF lines formed on the device (paf_dev.hip; specification: DESIGN.md §12, tests/paf_ref.py): the text the reference writes with
// `--write-alns` (AlnMode::Write, overlaps.rs:248-286) from ops that never left the device.  One line per row,
//   qname qlen qstart qend +|- tname tlen tstart tend mbases blocklen 255 cg:Z:<cigar>
// tab separated, '\n' behind it; a row without ops (a failed record) gives no line.  mbases = the summed lengths of the row's M ops and blocklen = those
// of all its ops, in 64 bits: NOT minimap2's residue matches and block length (the reference reads nine fields and the last one, overlaps.rs:135-172).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace herro {

constexpr uint64_t PAF_MAX_ROWS = 0x7fffffffull;      // rows of one call (32-bit row counts, one wave per row)
constexpr uint64_t PAF_MAX_CHUNK = 0xffffff00ull;     // text bytes of one chunk: its line offsets are a 32-bit scan
constexpr uint32_t PAF_LINE_TOO_LONG = 0xffffffffu;   // k_paf_len's byte count of a line that does not fit 32 bits

struct PafRow {              // one output row (48 B): where its ops lie in the store, and the nine fields of its herro_alignment
  uint64_t op_off;
  uint32_t n_ops;               // 0: no line
  uint32_t qid, qlen, qstart, qend, strand, tid, tlen, tstart, tend;
};

struct PafSums { uint64_t mbases, blocklen; };

// bytes of every row's line (0 for a row without ops, PAF_LINE_TOO_LONG beyond 32 bits) and its two sums; name_off: [n_reads + 1] into the names
void launch_paf_len(const PafRow* rows, const uint32_t* ops, const uint64_t* name_off, uint32_t n, uint32_t* line_bytes, PafSums* sums, hipStream_t st);

// the lines of rows [0, n) at text + line_off[row]; line_off has n + 1 entries (an exclusive scan of line_bytes) and line_off[n] <= cap
void launch_paf_write(const PafRow* rows, const uint32_t* ops, const char* names, const uint64_t* name_off, const uint32_t* line_off,
                      const PafSums* sums, uint32_t n, char* text, uint64_t cap, hipStream_t st);

}  // namespace herro
