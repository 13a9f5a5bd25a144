// trim_plan_check — seeded random hit tables through herro::trim_plan (herro_amd/csrc/trim_plan.h) on the CPU, meant for a sanitizer build.  Every plan is
// compared with the rule worked out base by base on a mask of the read, and checked for what must hold of any plan: pieces grouped by read, ascending,
// disjoint, inside their read and not shorter than the least length; the statistics add up; a damaged table is refused with a message.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o /tmp/trim_plan_check tools/trim_plan_check.cpp && /tmp/trim_plan_check
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../herro_amd/csrc/trim_plan.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "table %d: %s (line %d)\n", table, #c, __LINE__); return 1; } } while (0)

int main(int argc, char** argv) {
  const int n_tables = argc > 1 ? std::atoi(argv[1]) : 5000;
  std::mt19937 rng(4321);
  auto pick = [&](uint32_t lo, uint32_t hi) { return lo + (uint32_t)(rng() % (hi - lo + 1)); };
  const uint32_t len_pool[] = {0, 1, 2, 29, 30, 149, 150, 151, 299, 300, 301, 1000, 5000};
  const uint32_t win_pool[] = {0, 1, 30, 150, 151, 2000};
  const uint32_t pm_pool[] = {0, 1, 100, 250, 500, 1000};
  const uint32_t least_pool[] = {0, 1, 2, 30, 299, 300, 301};
  size_t n_pieces = 0, n_refused = 0;
  for (int table = 0; table < n_tables; table++) {
    const uint32_t n_reads = pick(0, 6), n_adapters = pick(1, 4);
    std::vector<uint32_t> read_len(n_reads), adapter_len(n_adapters);
    for (auto& l : read_len) l = len_pool[pick(0, 12)];
    for (auto& m : adapter_len) m = pick(8, 64);
    std::vector<herro_adapter_hit> hits;
    std::vector<uint64_t> off(n_reads + 1, 0);
    for (uint32_t r = 0; r < n_reads; r++) {
      for (uint32_t x = read_len[r] ? pick(0, 8) : 0; x > 0; x--) {
        const uint32_t s = pick(0, read_len[r] - 1), e = std::min(read_len[r], s + pick(0, 90));
        hits.push_back(herro_adapter_hit{r, s, e, (uint16_t)pick(0, n_adapters - 1), (uint8_t)pick(0, 1), (uint8_t)pick(0, 20)});
      }
      off[r + 1] = hits.size();
    }
    herro_trim_params P{win_pool[pick(0, 5)], pm_pool[pick(0, 5)], pm_pool[pick(0, 5)], least_pool[pick(0, 6)], pick(0, 1), {0, 0, 0}};
    herro_trim T;
    std::string why;
    const bool defaults = table % 7 == 0;
    CHECK(herro::trim_plan(n_reads, read_len.data(), n_adapters, adapter_len.data(), hits.data(), off.data(), defaults ? nullptr : &P, T, why) == HERRO_OK);
    const herro_trim_params Q = herro::trim_defaults(defaults ? nullptr : &P);
    // ---- the rule base by base
    uint64_t st[4] = {0, 0, 0, 0};
    std::vector<herro_piece> want;
    for (uint32_t r = 0; r < n_reads; r++) {
      const uint32_t L = read_len[r];
      uint32_t lo = 0, hi = L;
      bool any_mid = false;
      std::vector<char> cut(L, 0);
      for (uint64_t x = off[r]; x < off[r + 1]; x++) {
        const herro_adapter_hit& h = hits[x];
        const uint64_t m = adapter_len[h.adapter];
        if (h.start < Q.end_window && h.errors <= m * Q.end_max_err_pm / 1000) lo = std::max(lo, h.end);
        else if ((uint64_t)h.end + Q.end_window > L && h.errors <= m * Q.end_max_err_pm / 1000) hi = std::min(hi, h.start);
        else if (h.errors <= m * Q.mid_max_err_pm / 1000) { any_mid = true; for (uint32_t i = h.start; i < h.end; i++) cut[i] = 1; }
      }
      const bool none = lo >= hi || (any_mid && (Q.flags & HERRO_TRIM_DISCARD_CHIMERAS));
      size_t mine = 0;
      uint64_t kept = 0;
      for (uint32_t i = 0; i < L && !none;) {
        if (i < lo || i >= hi || cut[i]) { i++; continue; }
        uint32_t j = i;
        while (j < hi && !cut[j]) j++;
        if (j - i >= std::max(Q.min_length, 1u)) { want.push_back(herro_piece{r, i, j}); mine++; kept += j - i; }
        i = j;
      }
      st[0] += lo > 0 || hi < L; st[1] += mine > 1; st[2] += mine == 0; st[3] += L - kept;
      CHECK(T.piece_off[r + 1] == want.size());
    }
    CHECK(T.pieces.size() == want.size() && T.piece_off.size() == (size_t)n_reads + 1 && T.piece_off[0] == 0);
    for (size_t i = 0; i < want.size(); i++) {
      const herro_piece &a = T.pieces[i], &b = want[i];
      CHECK(a.rid == b.rid && a.start == b.start && a.end == b.end);
      CHECK(a.start < a.end && a.end <= read_len[a.rid] && a.end - a.start >= std::max(Q.min_length, 1u));
      if (i && T.pieces[i - 1].rid == a.rid) CHECK(T.pieces[i - 1].end < a.start);   // (touching pieces would be one piece)
      else if (i) CHECK(T.pieces[i - 1].rid < a.rid);
    }
    for (int i = 0; i < 4; i++) CHECK(T.stats[i] == st[i]);
    n_pieces += want.size();
    // ---- one damaged copy of the table: refused, with a message
    if (!hits.empty()) {
      std::vector<herro_adapter_hit> bad = hits;
      std::vector<uint64_t> bad_off = off;
      herro_trim_params BP = P;
      const size_t x = pick(0, (uint32_t)hits.size() - 1);
      switch (table % 6) {
        case 0: bad[x].end = read_len[bad[x].rid] + 1 + pick(0, 5); break;
        case 1: bad[x].start = bad[x].end + 1; break;
        case 2: bad[x].adapter = (uint16_t)(n_adapters + pick(0, 3)); break;
        case 3: bad_off[pick(0, n_reads - 1)] = hits.size() + 1; break;
        case 4: BP.reserved[pick(0, 2)] = 1; break;
        default: bad[x].rid = bad[x].rid + 1; break;
      }
      herro_trim B;
      why.clear();
      CHECK(herro::trim_plan(n_reads, read_len.data(), n_adapters, adapter_len.data(), bad.data(), bad_off.data(), &BP, B, why) == HERRO_E_INVALID);
      CHECK(why.rfind("herro_trim_plan: ", 0) == 0 && why.size() > 20);
      n_refused++;
    }
  }
  std::printf("trim_plan_check: %d tables, %zu pieces, %zu damaged tables refused: ok\n", n_tables, n_pieces, n_refused);
  return 0;
}
