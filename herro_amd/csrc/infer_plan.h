// infer_plan.h — the launch plan of a model pass, host only (plain C++17 over integer arrays: no HIP call, no context): which windows form a batch
// (plan_batches), which batches share a set of launches (group_batches), and per group the fused / unfused split, the token-tile plan, the window order and
// the descriptor image the kernels read (build_launch: herro_job_infer and herro_model_forward); and, at the end, what the front end of a launch makes of its
// tokens and the compute units of the device (front_end_plan).  Tested without a device through herro_debug_launch_plan and herro_debug_front_end_plan.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

// Tiles of whole windows for the fused transformer stack: consecutive windows packed greedily into at
// most `cap` tokens.  Returns the first token of each tile (+ end) for windows [w0, w1) of the token stream.  Callers pass
// windows of <= FUSED_MAX_TOK informative rows only (larger windows run layer by layer, see build_launch).
static constexpr uint32_t FUSED_MAX_TOK = 64;
static constexpr uint32_t FUSED_HALF_TOK = 32;   // tile of k_layers_p<., 2> (the short last round of a launch)
static std::vector<uint32_t> token_tiles(const std::vector<uint32_t>& tok_off, size_t w0 = 0, size_t w1 = ~size_t(0), uint32_t cap = FUSED_MAX_TOK) {
  w1 = std::min(w1, tok_off.size() - 1);
  if (w0 >= w1) return std::vector<uint32_t>();
  std::vector<uint32_t> t(1, tok_off[w0]);
  for (size_t w = w0; w < w1; w++) {
    if (tok_off[w + 1] - t.back() > cap) t.push_back(tok_off[w]);
  }
  if (tok_off[w1] > t.back()) t.push_back(tok_off[w1]);
  return t.size() > 1 ? t : std::vector<uint32_t>();
}

// Order in which the windows of a launch enter the token stream so that token_tiles' consecutive packing comes out as
// best-fit-decreasing bins: every tile of the fused stack costs the same whatever it holds (the MFMAs run over all its token
// slots), so the launch time is the NUMBER of tiles.  A tile is opened with the largest window left and filled with the
// largest window that still fits, repeatedly; the window that opens the next tile is the largest one left, which did not fit
// (or it would have been taken), so the greedy split of token_tiles falls exactly on these bins.  cnt[i] in 1..cap; the indices
// appended to `order` are those of `idx` (all windows when idx is null).
// At the bench workload (informative rows per window 4..30, mean 15.2): 999 tiles of 64 instead of 1098 for 4096 windows
// (ideal 975), which is 4 rounds of 256 compute units instead of 5.
static void tile_pack_bins(const std::vector<uint32_t>& cnt, std::vector<std::vector<uint32_t>>& by, size_t left, uint32_t cap, std::vector<uint32_t>& order) {
  uint32_t top = cap;                  // no window above `top` is left
  while (top && by[top].empty()) top--;
  while (left && top) {
    uint32_t room = cap, s = top;
    while (room) {
      s = std::min(s, room);
      while (s && by[s].empty()) s--;
      if (!s) break;
      order.push_back(by[s].back());
      by[s].pop_back();
      room -= s;
      left--;
    }
    while (top && by[top].empty()) top--;
  }
}
static std::vector<uint32_t> tile_pack_order(const std::vector<uint32_t>& cnt) {
  std::vector<std::vector<uint32_t>> by(FUSED_MAX_TOK + 1);
  for (size_t i = cnt.size(); i-- > 0;) by[std::min(cnt[i], FUSED_MAX_TOK)].push_back((uint32_t)i);  // pop_back: ascending index
  std::vector<uint32_t> order;
  order.reserve(cnt.size());
  for (uint32_t i : by[0]) order.push_back(i);   // (not produced by the planner: windows without informative rows are skipped)
  tile_pack_bins(cnt, by, cnt.size() - by[0].size(), FUSED_MAX_TOK, order);
  return order;
}

// The token stream of one fused launch: `order[k]` = index (into cnt) of its k-th window, `tiles` the 64-token tiles at its
// head (first tokens + end), `tiles_q` the 32-token tiles behind them (k_layers_p<., 2>; empty when qmode = 0).
// A launch of the fused stack runs in rounds of one 64-token tile per compute unit; a 32-token tile costs about half a round
// (half the MFMAs and LDS traffic for the same weight stream).
// qmode 1 (default with the f16 stack): when the LAST round would fill at most half of the compute units, the windows of its
// tiles go into 32-token tiles instead, one per compute unit (2560 windows of the bench: 625 tiles = 2 rounds + 113 -> 2 rounds
// + 226 half tiles).  qmode 2 (A/B): every window of <= 32 rows goes into 32-token tiles; a window of 33..64 opens a 64-token
// tile and takes the best-fitting small windows along.  Without `pack` the windows keep their batch order inside each class.
// Windows above 64 rows (the caller admits them up to 64 * FUSED_MAX_SIB of api_job.h, f16 stack only) come FIRST in the stream, each one alone
// on ceil(rows / 64) consecutive tiles (`tiles_b`; grp[t] = first tile of the window's group | tiles in it << 20 | its tokens in the last tile << 24);
// small windows may share that last tile.
struct TilePlan { std::vector<uint32_t> order, tiles, tiles_q, tiles_b, grp; };
static TilePlan plan_tiles_small(const std::vector<uint32_t>& cnt, bool pack, int qmode, uint32_t n_cu, uint32_t n_busy = 0);
static TilePlan plan_tiles(const std::vector<uint32_t>& cnt, bool pack, int qmode, uint32_t n_cu) {
  std::vector<uint32_t> big, small;
  for (size_t i = 0; i < cnt.size(); i++) (cnt[i] > FUSED_MAX_TOK ? big : small).push_back((uint32_t)i);
  if (big.empty()) return plan_tiles_small(cnt, pack, qmode, n_cu);
  // the head of the stream: every large window, its last (partial) tile filled with the best-fitting small windows (pack only) — the
  // sibling code masks a tile's own block by window id like any tile, and the other siblings see only its first `nbig` tokens
  std::vector<std::vector<uint32_t>> by(FUSED_MAX_TOK + 1);
  if (pack) for (size_t k = small.size(); k-- > 0;) by[cnt[small[k]]].push_back(small[k]);   // pop_back: ascending index
  std::vector<uint32_t> head, tiles_b(1, 0), grp;
  std::vector<char> taken(cnt.size(), 0);
  uint32_t tok = 0;
  for (uint32_t i : big) {
    const uint32_t k = (cnt[i] + FUSED_MAX_TOK - 1) / FUSED_MAX_TOK, g0 = (uint32_t)grp.size(), last = cnt[i] - (k - 1) * FUSED_MAX_TOK;
    head.push_back(i);
    for (uint32_t j = 0; j + 1 < k; j++) tiles_b.push_back(tok + (j + 1) * FUSED_MAX_TOK);
    tok += cnt[i];
    uint32_t room = FUSED_MAX_TOK - last, f = room;
    while (room) {
      f = std::min(f, room);
      while (f && by[f].empty()) f--;
      if (!f) break;
      const uint32_t w = by[f].back();
      by[f].pop_back();
      head.push_back(w);
      taken[w] = 1;
      tok += f;
      room -= f;
    }
    tiles_b.push_back(tok);
    for (uint32_t j = 0; j < k; j++) grp.push_back(g0 | (k << 20) | (last << 24));   // first tile | tiles (<= 15) | the window's tokens in its last tile
  }
  std::vector<uint32_t> rest, rest_cnt;
  for (uint32_t i : small) if (!taken[i]) { rest.push_back(i); rest_cnt.push_back(cnt[i]); }
  TilePlan P = plan_tiles_small(rest_cnt, pack, qmode, n_cu, (uint32_t)grp.size());   // the sibling tiles share the grid of the 64-token tiles: they count in its rounds
  for (uint32_t& o : P.order) o = rest[o];
  for (uint32_t& t : P.tiles) t += tok;
  for (uint32_t& t : P.tiles_q) t += tok;
  P.order.insert(P.order.begin(), head.begin(), head.end());
  P.tiles_b.swap(tiles_b);
  P.grp.swap(grp);
  return P;
}
static TilePlan plan_tiles_small(const std::vector<uint32_t>& cnt, bool pack, int qmode, uint32_t n_cu, uint32_t n_busy) {
  TilePlan P;
  const size_t n = cnt.size();
  std::vector<uint32_t> tok_off(1, 0);
  auto finish = [&](size_t n_head) {   // n_head windows in 64-token tiles
    tok_off.assign(1, 0);
    for (size_t k = 0; k < n; k++) tok_off.push_back(tok_off.back() + cnt[P.order[k]]);
    P.tiles = token_tiles(tok_off, 0, n_head, FUSED_MAX_TOK);
    P.tiles_q.clear();
    if (n_head < n) P.tiles_q = token_tiles(tok_off, n_head, n, FUSED_HALF_TOK);
  };
  if (qmode != 2) {
    if (pack) P.order = tile_pack_order(cnt);
    else { P.order.resize(n); for (size_t i = 0; i < n; i++) P.order[i] = (uint32_t)i; }
    finish(n);
    const size_t n64 = P.tiles.empty() ? 0 : P.tiles.size() - 1;
    const size_t rr = n_cu ? (n64 + n_busy) % n_cu : 0;   // tiles of the last round (n_busy: sibling tiles at the head of the same grid)
    if (qmode == 0 || rr == 0 || 2 * rr > n_cu) return P;
    const size_t r = std::min(rr, n64);
    if (r == 0) return P;
    // windows of the last r tiles: the small ones leave for 32-token tiles, a large one stays (in front of them)
    const uint32_t cut_tok = P.tiles[n64 - r];
    size_t k0 = 0;
    while (tok_off[k0] < cut_tok) k0++;
    std::vector<uint32_t> keep, tail;
    for (size_t k = k0; k < n; k++) (cnt[P.order[k]] > FUSED_HALF_TOK ? keep : tail).push_back(P.order[k]);
    if (tail.empty()) return P;
    if (pack) {  // best-fit-decreasing into bins of 32
      std::vector<std::vector<uint32_t>> by(FUSED_HALF_TOK + 1);
      for (size_t i = tail.size(); i-- > 0;) by[cnt[tail[i]]].push_back(tail[i]);
      std::vector<uint32_t> t2;
      for (uint32_t i : by[0]) t2.push_back(i);
      tile_pack_bins(cnt, by, tail.size() - by[0].size(), FUSED_HALF_TOK, t2);
      tail.swap(t2);
    }
    P.order.resize(k0);
    P.order.insert(P.order.end(), keep.begin(), keep.end());
    const size_t n_head = P.order.size();
    P.order.insert(P.order.end(), tail.begin(), tail.end());
    finish(n_head);
    return P;
  }
  P.order.reserve(n);
  if (!pack) {
    for (size_t i = 0; i < n; i++) if (cnt[i] > FUSED_HALF_TOK) P.order.push_back((uint32_t)i);
    const size_t n_head = P.order.size();
    for (size_t i = 0; i < n; i++) if (cnt[i] <= FUSED_HALF_TOK) P.order.push_back((uint32_t)i);
    finish(n_head);
    return P;
  }
  std::vector<std::vector<uint32_t>> by(FUSED_MAX_TOK + 1);
  for (size_t i = n; i-- > 0;) by[std::min(cnt[i], FUSED_MAX_TOK)].push_back((uint32_t)i);
  size_t small_left = 0;
  for (uint32_t s = 0; s <= FUSED_HALF_TOK; s++) small_left += by[s].size();
  for (uint32_t s = FUSED_MAX_TOK; s > FUSED_HALF_TOK; s--)
    while (!by[s].empty()) {   // a 64-token tile: one large window + the small ones that fit best
      P.order.push_back(by[s].back());
      by[s].pop_back();
      uint32_t room = FUSED_MAX_TOK - s, f = room;
      while (room) {
        f = std::min(f, room);
        while (f && by[f].empty()) f--;
        if (!f) break;
        P.order.push_back(by[f].back());
        by[f].pop_back();
        room -= f;
        small_left--;
      }
    }
  const size_t n_head = P.order.size();
  for (uint32_t i : by[0]) { P.order.push_back(i); small_left--; }
  tile_pack_bins(cnt, by, small_left, FUSED_HALF_TOK, P.order);
  finish(n_head);
  return P;
}

// ---- batches (prepare_examples, inference.rs:241-250; flush rule features.rs:884-893) -----------------------------------
// A batch only matters through its padding length lmax, the longest window in it, which travels with each of its windows.
// batch_mode 0: per target, the windows with informative rows are collected; a flush follows every batch_size windows SEEN, informative or
// not (InferenceOutput::update), and the target's end (InferenceOutput::emit).  batch_mode 1: chunks of batch_size informative windows
// across the job.  A flush that finds nothing collected makes no batch.
struct BatchPlan { std::vector<uint32_t> wins; uint32_t n_tok = 0, lmax = 0; };   // job window indices, their informative rows, the longest L' among them
static std::vector<BatchPlan> plan_batches(const std::vector<uint32_t>& nsup, const std::vector<uint32_t>& Lf, const std::vector<uint32_t>& tgt_win_off, uint32_t batch_size, int batch_mode) {
  std::vector<BatchPlan> batches;
  std::vector<uint32_t> cur;
  auto flush = [&] {
    if (cur.empty()) return;
    BatchPlan bp;
    for (uint32_t w : cur) { bp.n_tok += nsup[w]; bp.lmax = std::max(bp.lmax, Lf[w]); }
    bp.wins = cur;
    batches.push_back(std::move(bp));
    cur.clear();   // (keeps its room)
  };
  if (batch_mode == 0) {
    for (size_t t = 0; t + 1 < tgt_win_off.size(); t++) {
      uint32_t seen = 0;
      for (uint32_t w = tgt_win_off[t]; w < tgt_win_off[t + 1]; w++) {
        if (nsup[w] > 0) cur.push_back(w);
        if (++seen == batch_size) { flush(); seen = 0; }
      }
      flush();
    }
  } else {
    for (uint32_t w = 0; w < nsup.size(); w++) {
      if (nsup[w] == 0) continue;
      cur.push_back(w);
      if (cur.size() == batch_size) flush();
    }
    flush();
  }
  return batches;
}

// ---- launch groups: all batches of a job go through ONE set of launches, cut only where the tokens of whole batches would pass
// LAUNCH_TOK_CAP (it bounds the activation scratch).  A single batch above the cap forms a group alone.
static constexpr uint32_t LAUNCH_TOK_CAP = 1u << 16;
struct LaunchGroup { size_t b0, b1; uint32_t n_win, n_tok; };   // batches [b0, b1)
static std::vector<LaunchGroup> group_batches(const std::vector<BatchPlan>& batches, uint32_t tok_cap_launch = LAUNCH_TOK_CAP) {
  std::vector<LaunchGroup> groups;
  for (size_t bi = 0; bi < batches.size();) {
    LaunchGroup g{bi, bi, 0, 0};
    while (g.b1 < batches.size() && (g.b1 == g.b0 || g.n_tok + batches[g.b1].n_tok <= tok_cap_launch)) { g.n_win += (uint32_t)batches[g.b1].wins.size(); g.n_tok += batches[g.b1++].n_tok; }
    groups.push_back(g);
    bi = g.b1;
  }
  return groups;
}

// ---- one group -> its launches.  Fused stacks (precision 1, 4, 5 ...) take tiles of whole windows of at most `fused_rows` informative
// rows; a window above that does not make the group fall off the fused path: the group is split into part 0, the windows that fit (all
// of them in the unfused modes), and part 1, the rest (layer-by-layer kernels).  A window's place in a launch is free — its planes, padding
// length and output slots travel with it — so part 0 of a fused mode takes its windows in the order that packs the fewest tiles (plan_tiles).
struct PlanWin {
  uint32_t n_tok, plane_ld, len, lmax;        // informative rows, plane stride, L', padding length (that of the window's BATCH, whichever launch it runs in)
  uint64_t plane_off, sup_off, out_off, rf_base;
};
struct LaunchCfg {
  bool fused; uint32_t fused_rows;       // the precision runs a fused stack; most informative rows of a window on it
  bool pack; int qmode; uint32_t n_cu;   // plan_tiles
  bool with_rf_base;                     // PlanWin::rf_base is meant (else the image carries none and the kernels take out_off)
};
static constexpr size_t NO_ARRAY = ~size_t(0);
// Byte offsets of one launch's arrays in the image (each 16-byte aligned) and its counts: everything a BatchDev needs besides the job's own buffers.
struct LaunchOffs {
  size_t plane_off, plane_ld, len, lmax, tok_off, sup_off, out_off, rf_base, tiles, tiles_q, tiles_b, grp;   // rf_base: NO_ARRAY without one
  uint32_t n_tiles, n_tiles_q, n_tiles_b, n_win, n_tok, max_win_tok;
  bool tiled;   // part 0 of a fused mode
};
template <class T>
static size_t image_put(std::vector<unsigned char>& image, const std::vector<T>& v) {
  const size_t o = (image.size() + 15) & ~size_t(15);
  image.resize(o + v.size() * sizeof(T));
  if (!v.empty()) std::memcpy(image.data() + o, v.data(), v.size() * sizeof(T));
  return o;
}
// Appends the arrays of the (at most two) launches over `wins` to `image` and their offsets to `out`.
static void build_launch(const std::vector<PlanWin>& wins, const LaunchCfg& c, std::vector<unsigned char>& image, std::vector<LaunchOffs>& out) {
  for (int part = 0; part < 2; part++) {
    std::vector<uint32_t> sel, sel_cnt;
    sel.reserve(wins.size()); sel_cnt.reserve(wins.size());
    for (size_t i = 0; i < wins.size(); i++)
      if ((int)(c.fused && wins[i].n_tok > c.fused_rows) == part) { sel.push_back((uint32_t)i); sel_cnt.push_back(wins[i].n_tok); }
    const size_t B = sel.size();
    if (B == 0) continue;
    LaunchOffs o;
    o.tiled = c.fused && part == 0;
    const TilePlan plan = o.tiled ? plan_tiles(sel_cnt, c.pack, c.qmode, c.n_cu) : TilePlan();
    std::vector<uint64_t> plane_off(B), sup_off(B), out_off(B), rf_base(c.with_rf_base ? B : 0);
    std::vector<uint32_t> ld(B), len(B), lmax(B), tok_off(B + 1, 0);
    for (size_t k = 0; k < B; k++) {
      const PlanWin& w = wins[sel[plan.order.empty() ? k : plan.order[k]]];
      plane_off[k] = w.plane_off; ld[k] = w.plane_ld; len[k] = w.len; lmax[k] = w.lmax; tok_off[k + 1] = tok_off[k] + w.n_tok;
      sup_off[k] = w.sup_off; out_off[k] = w.out_off;
      if (c.with_rf_base) rf_base[k] = w.rf_base;
    }
    o.n_win = (uint32_t)B; o.n_tok = tok_off.back(); o.max_win_tok = *std::max_element(sel_cnt.begin(), sel_cnt.end());
    o.plane_off = image_put(image, plane_off); o.plane_ld = image_put(image, ld); o.len = image_put(image, len); o.lmax = image_put(image, lmax);
    o.tok_off = image_put(image, tok_off); o.sup_off = image_put(image, sup_off); o.out_off = image_put(image, out_off);
    o.rf_base = c.with_rf_base ? image_put(image, rf_base) : NO_ARRAY;
    o.n_tiles = plan.tiles.empty() ? 0u : (uint32_t)plan.tiles.size() - 1; o.tiles = image_put(image, plan.tiles);
    o.n_tiles_q = plan.tiles_q.empty() ? 0u : (uint32_t)plan.tiles_q.size() - 1; o.tiles_q = image_put(image, plan.tiles_q);
    o.n_tiles_b = (uint32_t)plan.grp.size(); o.tiles_b = image_put(image, plan.tiles_b); o.grp = image_put(image, plan.grp);
    out.push_back(o);
  }
}

// ---- the front end of one launch (conv stack + FC projection: launch_model_h of model_h.hip, launch_front_generic of model.hip) --------------------------
// Everything the front end decides from the launch's tokens and the compute units of the device, in one place: which kernels, their grids, the FC tile height.
static constexpr uint32_t FRONT_ROWS = 31;         // read rows of a token (HERRO_ROWS)
static constexpr uint32_t FRONT_FUSED_TILE = 128;  // tokens of a k_conv_fc tile (CF_TM)

// The front end of a launch of n_tok tokens: true — k_conv_fc (tiles of `tile` tokens, one workgroup per compute unit); false — k_conv_m, then k_fc_r.
// From profiles/conv_fc_ab.txt (one MI355X, 256 compute units, both paths in one call), not from an estimate:
//     launch                    k_conv_m + k_fc_r    k_conv_fc               step
//     1792 windows, 27 k rows        157 - 160 us    133 us (212 tiles)      - 6.6 %   (measured with the rule below in force: it confirmed its one-round range)
//     2560 windows, 38.7 k rows      230 - 234 us    238 us (303 tiles)      no gain (inside the parent's spread)
//     4096 windows, 62 k rows        341 - 348 us    265 - 266 us (484)      - 7.4 %
// The fused kernel runs in ROUNDS of one tile per compute unit and a round costs the same whether 47 or 228 units take part in it — 119 us per round at
// the smaller launch, 133 at the larger (every unit streaming the FC weights) —, while the two kernels' time follows the rows: the line through the two
// launches above is 44 us + 4.85 us per 1000 rows.  The fused kernel is chosen where rounds x 133 us stays below 85 % of that line, a margin several times
// the run-to-run spread of the table: 265 against 293 at 4096 windows (taken), 266 against 197 at 2560 (two kernels, as measured); in between, where nothing
// was measured, the rule amounts to a last round that is about 70 % full (23.2 - 32.7 k rows, 55.5 - 65.5 k, 87.7 - 98.3 k ...).  Both times scale with the compute units of the device.
inline bool conv_fc_faster(uint32_t n_tok, uint32_t n_cu, uint32_t tile) {
  const uint32_t tiles = (n_tok + tile - 1) / tile, rounds = (tiles + n_cu - 1) / n_cu;
  const double t_fused = 133.0 * rounds * ((double)tile / FRONT_FUSED_TILE);
  const double t_two = 44.0 + 4.85e-3 * n_tok * (256.0 / n_cu);
  return t_fused <= 0.85 * t_two;
}

// k_conv_m takes blocks ("units") of 16 (token, read row) pairs, one per wave and trip of its grid-stride loop, four waves per workgroup, three workgroups
// per compute unit; k_conv_w of the generic front end takes one tile per workgroup and trip, two workgroups per compute unit.
inline uint32_t conv_m_grid(uint32_t n_units, uint32_t n_cu) { return std::min<uint32_t>((n_units + 3) / 4, 3 * n_cu); }
inline uint32_t conv_w_grid(uint32_t n_tiles, uint32_t n_cu) { return std::min<uint32_t>(n_tiles, 2 * n_cu); }

// fused: k_conv_fc on fc_grid tiles of fc_rows (= FRONT_FUSED_TILE) tokens, conv_grid 0.  Otherwise k_conv_m on conv_grid workgroups over conv_units units,
// then k_fc_r<fc_rows / 16> on fc_grid workgroups.  (The generic front end reports its k_conv_w launch in conv_grid / conv_units and leaves the rest 0.)
struct FrontEndPlan { bool fused; uint32_t fc_rows, fc_grid, conv_grid, conv_units; };
// FC tile height (16-row blocks, 4 .. 8) of k_fc_r over n tokens: the one that leaves the busiest compute unit the fewest rows — two workgroups fit a unit, a third
// would wait for a slot —, the taller one on a tie (every workgroup streams the whole weight matrix: fewer of them, less L2 traffic).
inline uint32_t fc_tile_blocks(uint32_t n, uint32_t n_cu) {
  auto busiest = [&](uint32_t rows) { const uint32_t wg = (n + rows - 1) / rows; return (uint64_t)((wg + n_cu - 1) / n_cu) * rows + (wg > 2 * n_cu ? 1u << 20 : 0u); };
  uint32_t nb = 8;
  for (uint32_t b = 7; b >= 4; b--) if (busiest(16u * b) < busiest(16u * nb)) nb = b;
  return nb;
}
// Tokens [t0, t0 + n_tok) of a launch, t0 a multiple of 16 (so that its first pair opens a unit; 0 but for the chunked A/B runs).  mode: -1 the rule
// (conv_fc_faster), 0 the two kernels, 1 k_conv_fc; force_nb: a tile height that replaces the chosen one (A/B builds), 0 none.
inline FrontEndPlan front_end_plan(uint32_t n_tok, uint32_t n_cu, int mode = -1, uint32_t force_nb = 0, uint32_t t0 = 0) {
  n_cu = std::max(n_cu, 1u);
  if (mode > 0 || (mode < 0 && conv_fc_faster(n_tok, n_cu, FRONT_FUSED_TILE)))
    return FrontEndPlan{true, FRONT_FUSED_TILE, (n_tok + FRONT_FUSED_TILE - 1) / FRONT_FUSED_TILE, 0, 0};
  const uint32_t nb = force_nb ? force_nb : fc_tile_blocks(n_tok, n_cu);
  const uint32_t units = (uint32_t)(((uint64_t)(t0 + n_tok) * FRONT_ROWS + 15) / 16) - t0 / 16 * FRONT_ROWS;
  return FrontEndPlan{false, 16 * nb, (n_tok + 16 * nb - 1) / (16 * nb), conv_m_grid(units, n_cu), units};
}
