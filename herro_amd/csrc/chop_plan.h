// chop_plan.h — the host-only half of herro_job_fasta_dev (include/herro_amd.h, "corrected reads chopped for the assembler"; DESIGN.md §15,
// tests/chop_ref.py): what the call asks of its parameters, the piece rule and the byte count of a record.  Plain C++17 over integers: no HIP
// call, no context.  The rule and the counts are also what the kernels of fasta_dev.hip run (CHOP_HD), so the plan, the byte counts and the
// text cannot disagree; herro_chop_plan in fastx.cpp is chop_plan behind the C ABI, and tools/chop_plan_check.cpp drives it in a sanitizer build.
// The step stands for scripts/postprocess_corrected.sh of the reference's workflow: `seqkit sliding -s C -W C -g`, then `seqkit seq -m M`
// (C = 30000, M = 10000 there).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/herro_amd.h"
#include "trim_plan.h"   // herro_trim: the handle herro_chop_plan fills

#if defined(__HIPCC__)
#define CHOP_HD __host__ __device__
#else
#define CHOP_HD
#endif

namespace herro {

constexpr uint64_t CHOP_MAX_PARAM = 0x7fffffffull;    // chop_len, line_width
constexpr uint64_t CHOP_MAX_COUNT = 0xffffffffull;    // bases of a sequence, sequences and pieces of a call

struct ChopRule { uint32_t C, min_len, L; };          // chop_len, min_length, line_width (0 = off)

CHOP_HD inline uint32_t chop_digits(uint64_t v) {
  uint32_t k = 1;
  while (v >= 10) { v /= 10; k++; }
  return k;
}

// The pieces of a sequence of n bases: `full` of exactly C bases, then the remainder `rem` (C == 0: no full piece, the remainder is the sequence,
// and an empty sequence still gives its one piece).  Only the remainder can be shorter than C, so what the filter keeps is arithmetic.
struct ChopCount { uint64_t full, rem; bool has_rem, full_kept, rem_kept; };
CHOP_HD inline ChopCount chop_count(uint64_t n, const ChopRule& R) {
  ChopCount c;
  c.full = R.C ? n / R.C : 0;
  c.rem = R.C ? n % R.C : n;
  c.has_rem = R.C ? c.rem > 0 : true;
  c.full_kept = R.C >= R.min_len;
  c.rem_kept = c.has_rem && c.rem >= R.min_len;
  return c;
}
CHOP_HD inline uint64_t chop_n_pieces(const ChopCount& c) { return c.full + (c.has_rem ? 1 : 0); }
CHOP_HD inline uint64_t chop_n_kept(const ChopCount& c) { return (c.full_kept ? c.full : 0) + (c.rem_kept ? 1 : 0); }
// kept piece j (ascending) -> its number k among all pieces of the sequence
CHOP_HD inline uint64_t chop_kept_index(const ChopCount& c, uint64_t j) { return c.full_kept ? j : c.full; }
CHOP_HD inline void chop_bounds(uint64_t n, const ChopRule& R, uint64_t k, uint64_t* start, uint64_t* end) {
  if (!R.C) { *start = 0; *end = n; return; }
  *start = k * R.C;
  *end = (k + 1) * R.C < n ? (k + 1) * R.C : n;
}

// '>' id [':' i] ["_sliding:" start+1 '-' end] ' ' [desc] '\n'
CHOP_HD inline uint64_t chop_head_bytes(uint64_t id_len, uint64_t desc_len, uint32_t n_seg, uint32_t seg, const ChopRule& R, uint64_t start, uint64_t end) {
  return 1 + id_len + (n_seg > 1 ? 1 + chop_digits(seg) : 0) + (R.C ? 9 + chop_digits(start + 1) + 1 + chop_digits(end) : 0) + 1 + desc_len + 1;
}
// the bases, a '\n' behind every L of them except at the end, and the '\n' that ends the record
CHOP_HD inline uint64_t chop_body_bytes(uint64_t len, const ChopRule& R) { return len + (R.L && len ? (len - 1) / R.L : 0) + 1; }

// HERRO_OK and the rule, or HERRO_E_INVALID and why.  params == NULL: all zero.
inline int chop_check(const char* who, const herro_chop_params* params, ChopRule& R, std::string& why) {
  const std::string pre = std::string(who) + ": ";
  R = ChopRule{0, 0, 0};
  if (!params) return HERRO_OK;
  if (params->reserved[0] || params->reserved[1] || params->reserved[2] || params->reserved[3]) { why = pre + "reserved fields must be 0"; return HERRO_E_INVALID; }
  if (params->flags) { why = pre + "unknown flag"; return HERRO_E_INVALID; }
  if (params->chop_len > CHOP_MAX_PARAM) { why = pre + "chop_len = " + std::to_string(params->chop_len) + ": at most 2^31 - 1"; return HERRO_E_INVALID; }
  if (params->line_width > CHOP_MAX_PARAM) { why = pre + "line_width = " + std::to_string(params->line_width) + ": at most 2^31 - 1"; return HERRO_E_INVALID; }
  R = ChopRule{params->chop_len, params->min_length, params->line_width};
  return HERRO_OK;
}

// The kept pieces of n_seqs sequences, grouped by sequence; T.stats: pieces kept, pieces dropped, bases kept, bases dropped.
inline int chop_plan(uint64_t n_seqs, const uint64_t* len, const herro_chop_params* params, herro_trim& T, std::string& why) {
  const char* const who = "herro_chop_plan";
  const std::string pre = std::string(who) + ": ";
  if (n_seqs && !len) { why = pre + "null argument"; return HERRO_E_INVALID; }
  ChopRule R;
  if (const int rc = chop_check(who, params, R, why)) return rc;
  if (n_seqs > CHOP_MAX_COUNT) { why = pre + "more than 2^32 - 1 sequences"; return HERRO_E_UNSUPPORTED; }
  uint64_t all = 0, kept = 0;
  for (uint64_t s = 0; s < n_seqs; s++) {
    if (len[s] > CHOP_MAX_COUNT) { why = pre + "sequence " + std::to_string(s) + ": " + std::to_string(len[s]) + " bases, 2^32 or more"; return HERRO_E_UNSUPPORTED; }
    const ChopCount c = chop_count(len[s], R);
    all += chop_n_pieces(c);
    kept += chop_n_kept(c);
    if (all > CHOP_MAX_COUNT) { why = pre + "more than 2^32 - 1 pieces"; return HERRO_E_UNSUPPORTED; }
  }
  T.pieces.clear();
  T.pieces.reserve(kept);
  T.piece_off.assign((size_t)n_seqs + 1, 0);
  for (uint64_t& x : T.stats) x = 0;
  T.stats[1] = all - kept;
  for (uint64_t s = 0; s < n_seqs; s++) {
    const ChopCount c = chop_count(len[s], R);
    const uint64_t nk = chop_n_kept(c);
    uint64_t bases = 0;
    for (uint64_t j = 0; j < nk; j++) {
      uint64_t a, b;
      chop_bounds(len[s], R, chop_kept_index(c, j), &a, &b);
      T.pieces.push_back(herro_piece{(uint32_t)s, (uint32_t)a, (uint32_t)b});
      bases += b - a;
    }
    T.stats[0] += nk;
    T.stats[2] += bases;
    T.stats[3] += len[s] - bases;
    T.piece_off[s + 1] = T.pieces.size();
  }
  return HERRO_OK;
}

}  // namespace herro
