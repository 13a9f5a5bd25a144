// index_plan_check — the block rule of an index in parts (herro_amd/csrc/index_plan.h) on the CPU, meant for a sanitizer build: hand-made tables,
// seeded random ones against the rule worked out again with a plain loop, a fabricated 100-Gbase length table (lengths only, no bases) on which
// every block pair must stay within INDEX_MAX_KMERS, and the overflow cases with their message.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o /tmp/index_plan_check tools/index_plan_check.cpp && /tmp/index_plan_check
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../herro_amd/csrc/index_plan.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s: %s (line %d)\n", what.c_str(), #c, __LINE__); return 1; } } while (0)

using Cuts = std::vector<uint64_t>;

static Cuts plan(const std::vector<uint32_t>& len, uint32_t k, uint32_t w, uint64_t max_kmers, std::vector<uint64_t>* kmers = nullptr) {
  Cuts c;
  herro::index_plan(len.size(), len.data(), k, w, max_kmers, c, kmers);
  return c;
}

int main(int argc, char** argv) {
  const int n_tables = argc > 1 ? std::atoi(argv[1]) : 20000;
  std::string what = "hand-made tables";
  const uint32_t k = 25, w = 17;                 // a read has k-mers from 41 bases on; 124 bases are 100 k-mers
  CHECK(plan({}, k, w, 1000) == Cuts({0}));
  CHECK(plan({40, 10}, k, w, 1000) == Cuts({0, 2}));
  CHECK(plan({100, 5000, 100, 100}, k, w, 1000) == Cuts({0, 1, 2, 4}));                 // a read longer than cap is a block alone
  CHECK(plan({5000}, k, w, 2) == Cuts({0, 1}));
  CHECK(plan({30, 40, 124, 40, 30, 124, 124, 40, 40}, k, w, 200) == Cuts({0, 5, 6, 9}));   // reads without k-mers never open a block
  CHECK(plan({30, 124, 40}, k, w, 1) == Cuts({0, 3}));
  CHECK(plan({124, 40, 124}, k, w, 0) == Cuts({0, 2, 3}));                              // max_kmers 0 is cap 1
  CHECK(plan({124, 124, 124, 124}, k, w, 400) == Cuts({0, 2, 4}));                      // acc + nk == cap stays in the block
  CHECK(plan({124, 124, 124, 124}, k, w, 399) == Cuts({0, 1, 2, 3, 4}));

  what = "random tables";
  std::mt19937_64 rng(1357);
  auto pick = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); };
  const uint32_t len_pool[] = {0, 1, 40, 41, 42, 100, 124, 125, 1000, 65536, 1u << 20};
  size_t blocks_seen = 0;
  for (int table = 0; table < n_tables; table++) {
    what = "random table " + std::to_string(table);
    const uint32_t kk = (uint32_t)pick(5, 31), ww = (uint32_t)pick(1, 64);
    std::vector<uint32_t> len(pick(0, 40));
    for (auto& x : len) x = table % 3 ? len_pool[pick(0, 10)] : (uint32_t)pick(0, 400);
    const uint64_t max_kmers = table % 5 ? pick(0, 3000) : pick(0, 1ull << 22);
    std::vector<uint64_t> kmers;
    const Cuts c = plan(len, kk, ww, max_kmers, &kmers);
    // the rule with a plain loop
    Cuts want{0};
    std::vector<uint64_t> want_k;
    const uint64_t cap = std::max<uint64_t>(max_kmers / 2, 1);
    uint64_t acc = 0;
    for (size_t r = 0; r < len.size(); r++) {
      const uint64_t nk = (uint64_t)len[r] >= (uint64_t)kk + ww - 1 ? (uint64_t)len[r] - kk + 1 : 0;
      if (nk > 0 && acc > 0 && acc + nk > cap) { want.push_back(r); want_k.push_back(acc); acc = 0; }
      acc += nk;
    }
    if (!len.empty()) { want.push_back(len.size()); want_k.push_back(acc); }
    CHECK(c == want && kmers == want_k);
    CHECK(c.size() == kmers.size() + 1 && (len.empty() ? c.size() == 1 : c.back() == len.size()));
    for (size_t b = 0; b + 1 < c.size(); b++) {
      CHECK(c[b] < c[b + 1]);
      uint64_t with = 0;
      for (uint64_t r = c[b]; r < c[b + 1]; r++) with += herro::index_read_kmers(len[r], kk, ww) ? 1 : 0;
      CHECK(kmers[b] <= cap || with == 1);           // past cap only as a single read with k-mers
      if (b) CHECK(herro::index_read_kmers(len[c[b]], kk, ww) > 0);      // a block opens at a read with k-mers
    }
    uint64_t bi = 0, bj = 0;
    CHECK(!herro::index_plan_overflow(kmers, herro::INDEX_MAX_KMERS, bi, bj));
    blocks_seen += kmers.size();
  }

  what = "a 100-Gbase length table";
  {
    std::vector<uint32_t> len(5000000);
    std::lognormal_distribution<double> d(9.7, 0.6);
    uint64_t bases = 0;
    for (size_t r = 0; r < len.size(); r++) {
      len[r] = r % 100000 == 0 ? (uint32_t)pick(0, 39) : (uint32_t)std::min(d(rng), 2.0e6);
      bases += len[r];
    }
    CHECK(bases > 95000000000ull && bases < 130000000000ull);
    std::vector<uint64_t> kmers;
    const Cuts c = plan(len, k, w, herro::INDEX_MAX_KMERS, &kmers);
    uint64_t bi = 0, bj = 0, total = 0;
    CHECK(!herro::index_plan_overflow(kmers, herro::INDEX_MAX_KMERS, bi, bj));
    for (size_t i = 0; i < kmers.size(); i++) {
      total += kmers[i];
      for (size_t j = i + 1; j < kmers.size(); j++) CHECK(kmers[i] + kmers[j] <= herro::INDEX_MAX_KMERS);
    }
    CHECK(total > (1ull << 32) && kmers.size() > 40 && kmers.size() < 80);
    std::printf("100-Gbase table: %llu bases, %llu k-mers, %zu blocks, %zu block pairs\n", (unsigned long long)bases, (unsigned long long)total,
                kmers.size(), kmers.size() * (kmers.size() + 1) / 2);
  }

  what = "overflow";
  {
    std::vector<uint64_t> kmers;
    const Cuts c = plan({1000, 0x7fffffffu, 500, 0x7fffffffu, 100}, k, w, 1u << 20, &kmers);
    CHECK(c == Cuts({0, 1, 2, 3, 4, 5}));           // (a read past cap is a block alone: the reads behind each of them open a block)
    uint64_t bi = 0, bj = 0;
    CHECK(herro::index_plan_overflow(kmers, herro::INDEX_MAX_KMERS, bi, bj) && bi == 1 && bj == 3);
    CHECK(herro::index_plan_overflow_text(c, bi, bj) == "overlap finder: the index blocks that begin at reads 1 and 3 hold more than 2^32 k-mers together");
    // one such read is fine: 2^31 - 25 k-mers and a block of at most cap beside it
    std::vector<uint64_t> k1;
    plan({1000, 0x7fffffffu, 500}, k, w, herro::INDEX_MAX_KMERS, &k1);
    CHECK(!herro::index_plan_overflow(k1, herro::INDEX_MAX_KMERS, bi, bj));
    // exactly at the limit is within it
    std::vector<uint64_t> edge{herro::INDEX_MAX_KMERS - 5, 5, 6};
    CHECK(herro::index_plan_overflow(edge, herro::INDEX_MAX_KMERS, bi, bj) && bi == 0 && bj == 2);
    edge = {herro::INDEX_MAX_KMERS - 5, 5, 5};
    CHECK(!herro::index_plan_overflow(edge, herro::INDEX_MAX_KMERS, bi, bj));
  }
  std::printf("index_plan_check: %d random tables, %zu blocks: ok\n", n_tables, blocks_seen);
  return 0;
}
