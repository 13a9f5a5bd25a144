// index_plan.h — the read blocks of an index built in parts (herro_set_index_params; DESIGN.md §10, "An index in parts").  Host code only: the
// finder (overlap_dev.hip) cuts its store with it, herro_index_plan in frontend_api.hip is this function behind the C ABI, and
// tools/index_plan_check.cpp drives it in a sanitizer build.  All integer.
//   nk[r]  = len[r] - k + 1 if len[r] >= k + w - 1, else 0 (the read has no window and no minimizer)
//   cap    = max(max_kmers / 2, 1): two blocks meet in every index, so a block gets half of what one index may cover
//   blocks   reads in ascending id, acc = 0: a new block opens in front of read r iff nk[r] > 0, acc > 0 and acc + nk[r] > cap — acc starts
//            again at 0 there —, then acc += nk[r].  A read with more than cap k-mers is a block alone; reads without k-mers never open a
//            block; a non-empty store has at least one block, an empty one none.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

namespace herro {

constexpr uint64_t INDEX_MAX_KMERS = 0xfffff000ull;   // OVL_MAX_KMERS (overlap_dev.h): the k-mers one index may cover at most
constexpr uint32_t INDEX_MAX_RANGES = 65536;          // hash ranges of the occurrence pass at most

inline uint64_t index_read_kmers(uint64_t len, uint32_t k, uint32_t w) { return len >= (uint64_t)k + w - 1 ? len - k + 1 : 0; }
inline uint64_t index_block_cap(uint64_t max_kmers) { return max_kmers / 2 > 1 ? max_kmers / 2 : 1; }

// cuts [n_blocks + 1]: block b is the reads cuts[b] .. cuts[b + 1] - 1; kmers [n_blocks] (or NULL): the k-mers of each block
inline void index_plan(uint64_t n_reads, const uint32_t* len, uint32_t k, uint32_t w, uint64_t max_kmers, std::vector<uint64_t>& cuts,
                       std::vector<uint64_t>* kmers = nullptr) {
  cuts.assign(1, 0);
  if (kmers) kmers->clear();
  if (!n_reads) return;
  const uint64_t cap = index_block_cap(max_kmers);
  uint64_t acc = 0;
  for (uint64_t r = 0; r < n_reads; r++) {
    const uint64_t nk = index_read_kmers(len[r], k, w);
    if (nk && acc && acc + nk > cap) {
      cuts.push_back(r);
      if (kmers) kmers->push_back(acc);
      acc = 0;
    }
    acc += nk;
  }
  cuts.push_back(n_reads);
  if (kmers) kmers->push_back(acc);
}

// The first block pair (i <= j, ascending (i, j)) whose k-mers together exceed `limit`: false if there is none.  Only a block that is one read
// of more than cap k-mers can be part of one.
inline bool index_plan_overflow(const std::vector<uint64_t>& kmers, uint64_t limit, uint64_t& bi, uint64_t& bj) {
  // the largest block and the second largest decide whether any pair overflows; then the first such pair is looked for
  uint64_t m0 = 0, m1 = 0;
  for (uint64_t v : kmers) { if (v > m0) { m1 = m0; m0 = v; } else if (v > m1) m1 = v; }
  if (m0 <= limit && m0 + m1 <= limit) return false;
  for (uint64_t i = 0; i < kmers.size(); i++) {
    if (kmers[i] > limit) { bi = bj = i; return true; }
    if (kmers[i] + m0 <= limit) continue;
    for (uint64_t j = i + 1; j < kmers.size(); j++)
      if (kmers[i] + kmers[j] > limit) { bi = i; bj = j; return true; }
  }
  return false;
}

inline std::string index_plan_overflow_text(const std::vector<uint64_t>& cuts, uint64_t bi, uint64_t bj) {
  return "overlap finder: the index blocks that begin at reads " + std::to_string(cuts[bi]) + " and " + std::to_string(cuts[bj]) +
         " hold more than 2^32 k-mers together";
}

}  // namespace herro
