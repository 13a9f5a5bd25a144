// infer_plan_check — seeded random jobs through plan_batches, group_batches and build_launch (herro_amd/csrc/infer_plan.h) on the CPU, meant for a
// sanitizer build; it also checks what must hold of any plan: every informative window sits in exactly one launch, the token prefix matches the row
// counts, no tile exceeds its size and every array of the image starts on 16 bytes; and of the front end's plan of each launch (front_end_plan).
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o /tmp/infer_plan_check tools/infer_plan_check.cpp && /tmp/infer_plan_check
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../herro_amd/csrc/infer_plan.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "job %d: %s (line %d)\n", job, #c, __LINE__); return 1; } } while (0)

template <class T>
static std::vector<T> image_get(const std::vector<unsigned char>& image, size_t off, size_t n) {
  std::vector<T> v(n);
  if (n) std::memcpy(v.data(), image.data() + off, n * sizeof(T));
  return v;
}

int main(int argc, char** argv) {
  const int n_jobs = argc > 1 ? std::atoi(argv[1]) : 2000;
  std::mt19937 rng(12345);
  auto pick = [&](uint32_t lo, uint32_t hi) { return lo + (uint32_t)(rng() % (hi - lo + 1)); };
  const uint32_t rows_pool[] = {0, 0, 1, 2, 7, 15, 31, 32, 33, 63, 64, 65, 200, 511, 512, 513, 900, 30000, 70000};
  const uint32_t bs_pool[] = {1, 2, 3, 4, 7, 64};
  size_t launches = 0;
  for (int job = 0; job < n_jobs; job++) {
    const uint32_t n = pick(0, 40), n_targets = pick(0, 5);
    std::vector<uint32_t> nsup(n), Lf(n), two(n_targets + 1, 0);
    for (uint32_t w = 0; w < n; w++) { nsup[w] = job % 3 ? rows_pool[pick(0, 18)] : pick(0, 40); Lf[w] = pick(1, 5000); }
    for (uint32_t t = 1; t < n_targets; t++) two[t] = pick(0, n);
    if (n_targets) { two[n_targets] = n; std::sort(two.begin(), two.end()); } else { nsup.clear(); Lf.clear(); }
    const uint32_t bs = bs_pool[pick(0, 5)];
    const int mode = (int)pick(0, 1);
    const LaunchCfg cfg{pick(0, 3) != 0, pick(0, 1) ? 64u : 512u, pick(0, 1) != 0, (int)pick(0, 2), pick(0, 1) ? 8u : 256u, pick(0, 1) != 0};
    const std::vector<BatchPlan> batches = plan_batches(nsup, Lf, two, bs, mode);
    std::vector<unsigned char> image;
    std::vector<LaunchOffs> offs;
    std::vector<PlanWin> wins;
    uint64_t grouped_tok = 0;
    for (const LaunchGroup& g : group_batches(batches)) {
      CHECK(g.b1 > g.b0 && (g.b1 == g.b0 + 1 || g.n_tok <= LAUNCH_TOK_CAP));
      grouped_tok += g.n_tok;
      wins.clear(); wins.reserve(g.n_win);
      for (size_t bi = g.b0; bi < g.b1; bi++)
        for (uint32_t w : batches[bi].wins) wins.push_back(PlanWin{nsup[w], 1, Lf[w], batches[bi].lmax, 2, 3, w, (uint64_t)w + 100});
      CHECK(wins.size() == g.n_win);
      build_launch(wins, cfg, image, offs);
    }
    std::vector<uint32_t> hits(nsup.size(), 0);
    uint64_t launched_tok = 0;
    for (const LaunchOffs& o : offs) {
      for (size_t off : {o.plane_off, o.plane_ld, o.len, o.lmax, o.tok_off, o.sup_off, o.out_off, o.tiles, o.tiles_q, o.tiles_b, o.grp}) CHECK(off % 16 == 0 && off <= image.size());
      CHECK((o.rf_base == NO_ARRAY) == !cfg.with_rf_base);
      const auto out_off = image_get<uint64_t>(image, o.out_off, o.n_win);
      const auto tok_off = image_get<uint32_t>(image, o.tok_off, o.n_win + 1);
      const auto lmax = image_get<uint32_t>(image, o.lmax, o.n_win), len = image_get<uint32_t>(image, o.len, o.n_win);
      uint32_t most = 0;
      for (uint32_t k = 0; k < o.n_win; k++) {
        const uint64_t w = out_off[k];
        CHECK(w < nsup.size() && nsup[w] > 0);
        hits[w]++;
        CHECK(tok_off[k + 1] - tok_off[k] == nsup[w] && len[k] == Lf[w] && lmax[k] >= Lf[w]);
        CHECK(o.tiled == (cfg.fused && nsup[w] <= cfg.fused_rows));
        if (cfg.with_rf_base) CHECK(image_get<uint64_t>(image, o.rf_base, o.n_win)[k] == w + 100);
        most = std::max(most, nsup[w]);
      }
      CHECK(tok_off[0] == 0 && tok_off[o.n_win] == o.n_tok && most == o.max_win_tok);
      launched_tok += o.n_tok;
      if (!o.tiled) { CHECK(o.n_tiles + o.n_tiles_q + o.n_tiles_b == 0); continue; }
      // the tiles cover the token stream in order: sibling tiles, 64-token tiles, 32-token tiles
      const auto tb = image_get<uint32_t>(image, o.tiles_b, o.n_tiles_b ? o.n_tiles_b + 1 : 0), t64 = image_get<uint32_t>(image, o.tiles, o.n_tiles ? o.n_tiles + 1 : 0),
                 t32 = image_get<uint32_t>(image, o.tiles_q, o.n_tiles_q ? o.n_tiles_q + 1 : 0);
      uint32_t at = 0;
      for (const auto* t : {&tb, &t64}) for (size_t k = 0; k + 1 < t->size(); k++) { CHECK((*t)[k] == at && (*t)[k + 1] > at && (*t)[k + 1] - at <= FUSED_MAX_TOK); at = (*t)[k + 1]; }
      for (size_t k = 0; k + 1 < t32.size(); k++) { CHECK(t32[k] == at && t32[k + 1] > at && t32[k + 1] - at <= FUSED_HALF_TOK); at = t32[k + 1]; }
      CHECK(at == o.n_tok);
    }
    for (size_t w = 0; w < nsup.size(); w++) CHECK(hits[w] == (nsup[w] > 0 && (mode == 1 || (n_targets && w >= two[0])) ? 1u : 0u));
    CHECK(launched_tok == grouped_tok);
    // the front end of each launch (front_end_plan): tiles and units cover the tokens, grids within their caps, and chunks of a launch add up to it
    const uint32_t cu_pool[] = {1, 2, 3, 4, 8, 64, 256, 304};
    for (const LaunchOffs& o : offs) {
      const uint32_t n = o.n_tok, cu = cu_pool[pick(0, 7)];
      const int fmode = (int)pick(0, 2) - 1;
      const FrontEndPlan p = front_end_plan(n, cu, fmode);
      CHECK(p.fc_grid >= 1 && (uint64_t)p.fc_grid * p.fc_rows >= n && (uint64_t)(p.fc_grid - 1) * p.fc_rows < n);
      if (p.fused) { CHECK(fmode != 0 && p.fc_rows == FRONT_FUSED_TILE && p.conv_grid == 0 && p.conv_units == 0 && (fmode > 0 || conv_fc_faster(n, cu, FRONT_FUSED_TILE))); continue; }
      CHECK(fmode <= 0 && p.fc_rows % 16 == 0 && p.fc_rows >= 64 && p.fc_rows <= 128 && p.fc_rows == 16 * fc_tile_blocks(n, cu));
      CHECK(p.conv_units == ((uint64_t)n * FRONT_ROWS + 15) / 16);
      CHECK(p.conv_grid >= 1 && p.conv_grid <= 3 * cu && (uint64_t)(p.conv_grid - 1) * 4 < p.conv_units && (p.conv_grid == 3 * cu || 4ull * p.conv_grid >= p.conv_units));
      const uint32_t chunk = 16 * pick(1, 64);
      uint32_t units = 0;
      for (uint32_t t0 = 0; t0 < n; t0 += chunk) {
        const FrontEndPlan c = front_end_plan(std::min(n, t0 + chunk) - t0, cu, 0, 4 + pick(0, 4), t0);
        CHECK(!c.fused && c.conv_units > 0 && c.conv_grid >= 1 && c.conv_grid <= 3 * cu && (uint64_t)c.fc_grid * c.fc_rows >= std::min(n, t0 + chunk) - t0);
        CHECK(t0 / 16 * FRONT_ROWS == units);   // a chunk opens the unit behind the last one of the chunk before it
        units += c.conv_units;
      }
      CHECK(units == p.conv_units);
      CHECK(conv_w_grid(n, cu) >= 1 && conv_w_grid(n, cu) <= std::min(n, 2 * cu));
    }
    launches += offs.size();
  }
  std::printf("%d jobs, %zu launches: ok\n", n_jobs, launches);
  return 0;
}
