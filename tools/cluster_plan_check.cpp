// cluster_plan_check — seeded random arguments through herro::cluster_check and herro::cluster_part (herro_amd/csrc/cluster_plan.h) on the CPU, meant for a
// sanitizer build.  Every accepted table is cut by the part rule and checked for what must hold of any cut: parts ascend along the order, stay below
// k, the weights of the parts add up to T, and |weight(p) - T / k| < max w; a damaged table is refused with the code and the index the header promises.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o /tmp/cluster_plan_check tools/cluster_plan_check.cpp && /tmp/cluster_plan_check
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../herro_amd/csrc/cluster_plan.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "table %d: %s (line %d): %s\n", table, #c, __LINE__, why.c_str()); return 1; } } while (0)

int main(int argc, char** argv) {
  const int n_tables = argc > 1 ? std::atoi(argv[1]) : 20000;
  std::mt19937_64 rng(9876);
  auto pick = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); };
  const uint32_t k_pool[] = {1, 2, 3, 7, 8, 64, 1000, 65535};
  const uint32_t w_pool[] = {0, 0, 1, 1, 2, 5, 63, 4096, 1000000, 400000000};
  size_t n_parts_seen = 0, n_refused = 0;
  for (int table = 0; table < n_tables; table++) {
    std::string why;
    const uint32_t n = (uint32_t)pick(0, 40), E = n >= 2 ? (uint32_t)pick(0, 60) : 0;
    const bool unit = table % 5 == 0;
    std::vector<uint32_t> w(n), a(E), b(E);
    for (auto& x : w) x = w_pool[pick(0, 9)];
    for (uint32_t e = 0; e < E; e++) { a[e] = (uint32_t)pick(0, n - 1); do b[e] = (uint32_t)pick(0, n - 1); while (b[e] == a[e]); }
    herro_cluster_params P{k_pool[pick(0, 7)], (uint32_t)pick(0, 5000), {0, 0}};
    uint64_t T = ~0ull;
    const int rc = herro::cluster_check("check", n, unit ? nullptr : w.data(), E, a.data(), b.data(), &P, &T, why);
    uint64_t sum = 0, wmax = 0;
    for (uint32_t v = 0; v < n; v++) { const uint64_t x = unit ? 1 : w[v]; sum += x; wmax = std::max(wmax, x); }
    if (sum >> 32) { CHECK(rc == HERRO_E_UNSUPPORTED && why.find("below 2^32") != std::string::npos); n_refused++; continue; }
    CHECK(rc == HERRO_OK && T == sum);
    // ---- the cut of the order 0 .. n - 1
    const uint32_t k = P.n_parts;
    std::vector<uint64_t> weight(k, 0);
    uint64_t S = 0;
    uint32_t last = 0;
    for (uint32_t v = 0; v < n; v++) {
      const uint32_t p = herro::cluster_part(S, T, k);
      CHECK(p < k && p >= last && (T != 0 || p == 0));
      last = p;
      const uint64_t x = unit ? 1 : w[v];
      weight[p] += x;
      S += x;
    }
    CHECK(S == T);
    for (uint32_t p = 0; p < k; p++) {      // |weight(p) - T / k| < max w, in integers; T == 0 and n == 0: everything is 0
      const int64_t d = (int64_t)(weight[p] * k) - (int64_t)T;
      CHECK(n == 0 || T == 0 || (d < 0 ? -d : d) < (int64_t)(wmax * k));
      n_parts_seen += weight[p] != 0;
    }
    // ---- one damaged copy: refused, with a message that names the entry
    herro_cluster_params B = P;
    std::vector<uint32_t> ba = a, bb = b;
    int want = HERRO_E_INVALID;
    std::string needle;
    uint64_t bn = n, bE = E;
    switch (table % 6) {
      case 0: B.n_parts = table % 12 ? 0 : 65536; needle = "n_parts = "; break;
      case 1: B.reserved[pick(0, 1)] = 1; needle = "reserved"; break;
      case 2: if (!E) continue; { const uint32_t e = (uint32_t)pick(0, E - 1); bb[e] = ba[e]; needle = "edge " + std::to_string(e) + ": a == b"; for (uint32_t x = 0; x < e; x++) if (ba[x] == bb[x]) needle.clear(); } break;
      case 3: if (!E) continue; { const uint32_t e = (uint32_t)pick(0, E - 1); ba[e] = n + (uint32_t)pick(0, 3); needle = "edge " + std::to_string(e) + ": read id"; } break;
      case 4: bn = 0x80000000ull + pick(0, 9); bE = 0; want = HERRO_E_UNSUPPORTED; needle = "reads"; break;
      default: why.clear(); CHECK(herro::cluster_check("check", n, nullptr, E, a.data(), b.data(), nullptr, nullptr, why) == HERRO_E_INVALID && why.find("params is NULL") != std::string::npos); n_refused++; continue;
    }
    why.clear();
    CHECK(herro::cluster_check("check", bn, table % 6 == 4 ? nullptr : (unit ? nullptr : w.data()), bE, ba.data(), bb.data(), &B, nullptr, why) == want);
    CHECK(why.rfind("check: ", 0) == 0 && (needle.empty() || why.find(needle) != std::string::npos));
    n_refused++;
  }
  std::printf("cluster_plan_check: %d tables, %zu non-empty parts, %zu damaged tables refused: ok\n", n_tables, n_parts_seen, n_refused);
  return 0;
}
