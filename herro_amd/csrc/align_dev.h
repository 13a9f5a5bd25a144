// align_dev.h — base-level alignment of overlaps given by coordinates only (align_dev.hip): the GPU counterpart of the
// `minimap2 -c` step that `herro inference` runs without --read-alns (mm2.rs:15-30), followed by the reference's
// fix_cigar normalisation (aligners.rs:138-250).  One wave64 per record; the specification is DESIGN.md §9.
// Before it, the ends-free extension of an overlap's two ends (k_extend: one wave64 per record and side).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace herro {

constexpr int ALIGN_W = 128;                      // == HERRO_ALIGN_BAND: band cells per anti-diagonal
constexpr uint32_t ALIGN_MAX_CELLS = 1u << 25;    // n + m above this: refused (the -inf sentinel needs the headroom)

struct AlignIn {          // one record (40 B)
  uint64_t t_woff, q_woff;   // first 2-bit word of the target / query read in the store
  uint64_t scr_off;          // byte offset of the record's scratch (align_scratch_bytes)
  uint32_t t0, m;            // T = target bases [t0, t0 + m)
  uint32_t q0, n;            // query bases [q0, q0 + n) as stored; strand 1 reads them reversed and complemented
  uint32_t strand, pad;
};

struct AlignOut {         // (32 B)
  int32_t score;             // INT32_MIN: failed
  uint32_t n_ops, ops_off;   // final ops: dense[ops_off .. ops_off + n_ops), each len << 2 | (0 M, 1 I, 2 D)
  uint32_t failed;
  uint32_t tdrop0, qdrop0;   // bases the dropped leading indel consumed
  uint32_t tdrop1, qdrop1;   // ... and the dropped trailing one
};

// per record: traceback rows (64 B per anti-diagonal: 4 bits per band cell), the band's lo per anti-diagonal, the op list
inline uint64_t align_scratch_bytes(uint32_t n, uint32_t m) {
  const uint64_t nd = (uint64_t)n + m + 1;
  return (nd * (64 + 4 + 4) + 255) & ~(uint64_t)255;
}

void launch_align(const uint64_t* d_words, const AlignIn* d_in, AlignOut* d_out, uint8_t* d_scr, uint32_t* d_dense,
                  uint32_t* d_count, uint32_t n_rec, hipStream_t st);

// ---- mirrored records (k_mirror): the alignment of (q, t) derived from the final ops of (t, q) -------------------------
struct MirrorIn {         // one record (64 B): AlignIn's sequence fields with the roles exchanged, and where its ops are
  uint64_t t_woff, q_woff;   // first 2-bit word of the source's QUERY read (the mirror's target) / of its TARGET read
  uint64_t src_off, dst_off; // first op of the source record / of the mirror's c reserved slots in the store
  uint32_t t0, m;            // T' = the source's query bases [qstart, qend), forward
  uint32_t q0, n;            // Q' = the source's target bases [tstart, tend); strand 1 reads them reversed and complemented
  uint32_t strand, c;        // c: the source's op count (0: a failed source)
  int32_t score;             // the source's score
  uint32_t pad;
};

// d_out[r]: score, n_ops (<= c, in store[dst_off ..)), failed and the four drop lengths; ops_off is not used (0)
void launch_mirror(const uint64_t* d_words, const MirrorIn* d_in, AlignOut* d_out, uint32_t* d_store, uint32_t n_rec, hipStream_t st);

// ---- ends-free extension of an overlap's two ends (k_extend) --------------------------------------------
constexpr uint32_t EXTEND_ZDROP = 400;            // herro_extend_params.zdrop = 0
constexpr uint32_t EXTEND_MAX_EXT = 2048;         // herro_extend_params.max_ext = 0
constexpr uint32_t EXTEND_MAX_EXT_LIMIT = 1u << 20;

struct ExtIn {            // one side of one record (40 B); side 2r is the left, 2r + 1 the right side of record r
  uint64_t t_woff, q_woff;   // first 2-bit word of the target / query read in the store
  uint32_t t0, m;            // T' = stored target bases [t0, t0 + m), read downwards and complemented when trev
  uint32_t q0, n;            // Q' = stored query bases [q0, q0 + n), read downwards and complemented when qrev
  uint32_t trev, qrev;
};

struct ExtOut {           // (32 B)
  int32_t score;             // H of the best cell; 0 with i = j = 0: no extension
  uint32_t i, j;             // bases of Q' / T' the extension takes
  uint32_t d_stop;           // the last anti-diagonal computed
  uint32_t pad[4];
};

void launch_extend(const uint64_t* d_words, const ExtIn* d_in, ExtOut* d_out, uint32_t zdrop, uint32_t n_sides, hipStream_t st);

// The same for records that are on the device (OvlRec, overlap_dev.h): k_ext_sides writes the two sides of d_rec[0 .. n_rec) — herro_extend_overlaps'
// formulas, lengths from d_base_off — to d_sides[2 n_rec] for launch_extend; k_ext_fold applies its 2 n_rec results to the records' coordinates and
// writes d_ext[n_rec][4] (t_left, q_left, t_right, q_right) and d_scores[n_rec][2].
struct OvlRec;
void launch_ext_sides(const OvlRec* d_rec, uint32_t n_rec, const uint64_t* d_word_off, const uint64_t* d_base_off, uint32_t max_ext, ExtIn* d_sides,
                      hipStream_t st);
void launch_ext_fold(OvlRec* d_rec, uint32_t n_rec, const ExtOut* d_res, uint32_t* d_ext, int32_t* d_scores, hipStream_t st);

}  // namespace herro
