// chop_plan_check — seeded random lengths and parameters through herro::chop_plan and the byte counts of herro_amd/csrc/chop_plan.h on the CPU, meant
// for a sanitizer build.  Every accepted plan is checked for what must hold of any plan: the pieces of a sequence ascend, are those of the rule worked
// out again with a plain loop, kept and dropped pieces and bases add up to the input; a record assembled byte by byte has the bytes chop_head_bytes
// and chop_body_bytes count; a refused call has the code and the message the header promises.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o /tmp/chop_plan_check tools/chop_plan_check.cpp && /tmp/chop_plan_check
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../herro_amd/csrc/chop_plan.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "table %d: %s (line %d): %s\n", table, #c, __LINE__, why.c_str()); return 1; } } while (0)

int main(int argc, char** argv) {
  const int n_tables = argc > 1 ? std::atoi(argv[1]) : 5000;
  std::mt19937_64 rng(2468);
  auto pick = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); };
  const uint64_t len_pool[] = {0, 1, 2, 9, 10, 11, 99, 100, 999, 1000, 1001, 29999, 30000, 30001, 65536};
  const uint32_t c_pool[] = {0, 0, 1, 2, 3, 7, 10, 16, 100, 999, 1000, 30000, 0x7fffffffu};
  size_t n_pieces_seen = 0, n_refused = 0;
  for (int table = 0; table < n_tables; table++) {
    std::string why;
    const uint64_t n = pick(0, 12);
    std::vector<uint64_t> len(n);
    for (auto& x : len) x = table % 3 ? len_pool[pick(0, 14)] : pick(0, 300);
    herro_chop_params P{c_pool[pick(0, 12)], (uint32_t)(table % 4 ? pick(0, 40) : pick(0, 31000)), (uint32_t)(table % 2 ? pick(0, 80) : 0), 0, {0, 0, 0, 0}};
    if (P.chop_len) for (auto& x : len) x = std::min<uint64_t>(x, 300ull * P.chop_len);   // (keeps the tables small: at most 300 pieces per sequence)
    herro_trim T;
    const bool no_params = table % 17 == 0;
    int rc = herro::chop_plan(n, len.data(), no_params ? nullptr : &P, T, why);
    CHECK(rc == HERRO_OK);
    const herro::ChopRule R = no_params ? herro::ChopRule{0, 0, 0} : herro::ChopRule{P.chop_len, P.min_length, P.line_width};
    uint64_t kept = 0, dropped = 0, bk = 0, bd = 0, at = 0;
    CHECK(T.piece_off.size() == n + 1 && T.piece_off[0] == 0);
    for (uint64_t s = 0; s < n; s++) {
      // the rule with a plain loop
      std::vector<std::pair<uint64_t, uint64_t>> all;
      if (!R.C) all.emplace_back(0, len[s]);
      else for (uint64_t a = 0; a < len[s]; a += R.C) all.emplace_back(a, std::min<uint64_t>(a + R.C, len[s]));
      for (const auto& p : all) {
        if (p.second - p.first >= R.min_len) {
          CHECK(at < T.pieces.size() && T.pieces[at].rid == s && T.pieces[at].start == p.first && T.pieces[at].end == p.second);
          at++; kept++; bk += p.second - p.first;
          // a record of this piece, byte by byte: the counts are its size
          const uint32_t n_seg = (uint32_t)pick(1, 12), seg = (uint32_t)pick(0, n_seg - 1);
          const std::string id(pick(0, 5), 'i'), desc(pick(0, 3), 'd');
          std::string rec = ">" + id;
          if (n_seg > 1) rec += ":" + std::to_string(seg);
          if (R.C) rec += "_sliding:" + std::to_string(p.first + 1) + "-" + std::to_string(p.second);
          rec += " " + desc + "\n";
          CHECK(rec.size() == herro::chop_head_bytes(id.size(), desc.size(), n_seg, seg, R, p.first, p.second));
          if (p.second - p.first <= 3000) {
            std::string body;
            for (uint64_t i = p.first; i < p.second; i++) { if (R.L && i > p.first && (i - p.first) % R.L == 0) body += '\n'; body += 'A'; }
            body += '\n';
            CHECK(body.size() == herro::chop_body_bytes(p.second - p.first, R));
          }
        } else { dropped++; bd += p.second - p.first; }
      }
      CHECK(T.piece_off[s + 1] == at);
      const herro::ChopCount c = herro::chop_count(len[s], R);
      CHECK(herro::chop_n_pieces(c) == all.size());
    }
    CHECK(at == T.pieces.size() && T.stats[0] == kept && T.stats[1] == dropped && T.stats[2] == bk && T.stats[3] == bd);
    n_pieces_seen += kept;
    // ---- one refused copy
    herro_chop_params B = P;
    std::vector<uint64_t> bl = len;
    int want = HERRO_E_INVALID;
    std::string needle;
    switch (table % 6) {
      case 0: B.reserved[pick(0, 3)] = 1; needle = "reserved"; break;
      case 1: B.flags = (uint32_t)pick(1, 9); needle = "unknown flag"; break;
      case 2: B.chop_len = 0x80000000u + (uint32_t)pick(0, 9); needle = "chop_len = "; break;
      case 3: B.line_width = 0x80000000u + (uint32_t)pick(0, 9); needle = "line_width = "; break;
      case 4: if (!n) continue; { const uint64_t s = pick(0, n - 1); bl[s] = 0x100000000ull + pick(0, 9); for (uint64_t x = 0; x < s; x++) bl[x] = std::min<uint64_t>(bl[x], 100); needle = "sequence " + std::to_string(s) + ": "; want = HERRO_E_UNSUPPORTED; B.chop_len = 0; } break;
      default: bl.assign(2, 0xffffffffull); B.chop_len = 1; needle = "more than 2^32 - 1 pieces"; want = HERRO_E_UNSUPPORTED; break;
    }
    why.clear();
    herro_trim T2;
    rc = herro::chop_plan(bl.size(), bl.data(), &B, T2, why);
    CHECK(rc == want && why.find(needle) != std::string::npos && why.rfind("herro_chop_plan: ", 0) == 0);
    n_refused++;
    if (table % 50 == 0) { why.clear(); CHECK(herro::chop_plan(3, nullptr, nullptr, T2, why) == HERRO_E_INVALID && why == "herro_chop_plan: null argument"); }
  }
  std::printf("chop_plan_check: %d tables, %zu pieces checked, %zu refusals: ok\n", n_tables, n_pieces_seen, n_refused);
  return 0;
}
