// trim_plan.h — which pieces of every read stay, from a table of adapter hits; host only (plain C++17 over integer arrays: no HIP call, no context).
// The rule is include/herro_amd.h's, "herro_trim_plan" (tests/adapter_ref.py); herro_trim_plan in fastx.cpp is this function behind the
// C ABI, and tools/trim_plan_check.cpp drives it over generated hit tables in a sanitizer build.
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../../include/herro_amd.h"

struct herro_trim {
  std::vector<herro_piece> pieces;     // grouped by read, ascending inside a read
  std::vector<uint64_t> piece_off;     // [n_reads + 1]
  uint64_t stats[4] = {0, 0, 0, 0};    // reads trimmed, reads split, reads dropped, bases removed
};

namespace herro {

// 0 in a field: its default
inline herro_trim_params trim_defaults(const herro_trim_params* in) {
  herro_trim_params p = in ? *in : herro_trim_params{};
  if (!p.end_window) p.end_window = 150;
  if (!p.end_max_err_pm) p.end_max_err_pm = 250;
  if (!p.mid_max_err_pm) p.mid_max_err_pm = 100;
  return p;
}

// HERRO_OK and the plan in T, or HERRO_E_INVALID and why
inline int trim_plan(uint32_t n_reads, const uint32_t* read_len, uint32_t n_adapters, const uint32_t* adapter_len, const herro_adapter_hit* hits,
                     const uint64_t* hits_off, const herro_trim_params* params, herro_trim& T, std::string& why) {
  const char* const who = "herro_trim_plan: ";
  if ((n_reads && !read_len) || (n_adapters && !adapter_len) || !hits_off) { why = std::string(who) + "null argument"; return HERRO_E_INVALID; }
  if (params && (params->reserved[0] || params->reserved[1] || params->reserved[2])) { why = std::string(who) + "reserved fields must be 0"; return HERRO_E_INVALID; }
  if (params && (params->flags & ~HERRO_TRIM_DISCARD_CHIMERAS)) { why = std::string(who) + "unknown flag"; return HERRO_E_INVALID; }
  const herro_trim_params P = trim_defaults(params);
  if (hits_off[0] != 0) { why = std::string(who) + "hits_off[0] = " + std::to_string(hits_off[0]) + ": hits_off must ascend from 0"; return HERRO_E_INVALID; }
  for (uint32_t r = 0; r < n_reads; r++)
    if (hits_off[r + 1] < hits_off[r]) { why = std::string(who) + "hits_off[" + std::to_string(r + 1) + "] = " + std::to_string(hits_off[r + 1]) + ": hits_off must ascend from 0"; return HERRO_E_INVALID; }
  if (hits_off[n_reads] && !hits) { why = std::string(who) + "null argument"; return HERRO_E_INVALID; }
  T.pieces.clear();
  T.piece_off.assign((size_t)n_reads + 1, 0);
  for (uint64_t& s : T.stats) s = 0;
  std::vector<std::pair<uint32_t, uint32_t>> mid;
  for (uint32_t r = 0; r < n_reads; r++) {
    const uint32_t L = read_len[r];
    uint32_t lo = 0, hi = L;
    bool any_mid = false;
    mid.clear();
    for (uint64_t x = hits_off[r]; x < hits_off[r + 1]; x++) {
      const herro_adapter_hit& h = hits[x];
      const char* bad = h.rid != r ? "its rid is not the read of its group" : h.start > h.end ? "start > end" : h.end > L ? "outside its read" :
                        h.adapter >= n_adapters ? "adapter index out of range" : nullptr;
      if (bad) { why = std::string(who) + "hit " + std::to_string(x) + ": " + bad; return HERRO_E_INVALID; }
      const uint64_t m = adapter_len[h.adapter];
      const uint64_t k_end = m * P.end_max_err_pm / 1000, k_mid = m * P.mid_max_err_pm / 1000;
      if (h.start < P.end_window && h.errors <= k_end) lo = std::max(lo, h.end);
      else if ((uint64_t)h.end + P.end_window > L && h.errors <= k_end) hi = std::min(hi, h.start);
      else if (h.errors <= k_mid) { any_mid = true; mid.emplace_back(h.start, h.end); }
    }
    const size_t first = T.pieces.size();
    if (lo < hi && !(any_mid && (P.flags & HERRO_TRIM_DISCARD_CHIMERAS))) {
      std::sort(mid.begin(), mid.end());
      const uint32_t least = std::max(P.min_length, 1u);
      uint32_t at = lo;                                   // everything below `at` is a piece already or cut away
      auto piece = [&](uint32_t a, uint32_t b) { if (b > a && b - a >= least) T.pieces.push_back(herro_piece{r, a, b}); };
      for (const auto& c : mid) {
        const uint32_t a = std::max(c.first, lo), b = std::min(c.second, hi);
        if (a >= b) continue;                             // nothing of the hit lies inside [lo, hi)
        if (a > at) piece(at, a);                         // (a <= at: it overlaps or touches the cut before it)
        at = std::max(at, b);
      }
      piece(at, hi);
    }
    const size_t n = T.pieces.size() - first;
    uint64_t kept = 0;
    for (size_t i = first; i < T.pieces.size(); i++) kept += T.pieces[i].end - T.pieces[i].start;
    T.stats[0] += lo > 0 || hi < L;
    T.stats[1] += n > 1;
    T.stats[2] += n == 0;
    T.stats[3] += L - kept;
    T.piece_off[r + 1] = T.pieces.size();
  }
  return HERRO_OK;
}

}  // namespace herro
