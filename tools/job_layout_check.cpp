// job_layout_check — the block layouts of job creation (herro_amd/csrc/job_layout.h) on the CPU, meant for a sanitizer build.
// (a) Seeded random counts, zeros among them, through every layout: each piece starts on 256 bytes, the pieces lie in the order of their enum without
//     overlap, each has room for its elements, the totals are the end of the last piece, the descriptor head is one set of offsets for the pinned and the
//     device arena, and the bind functions point where the layout says.
// (b) A table of fixed inputs with the block sizes (and a few inner offsets) the inline arithmetic of herro_api.hip gave before the layouts were stated
//     here (commit 17fba03): the same bytes as before, the edge cases of (a) among them.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -o /tmp/job_layout_check tools/job_layout_check.cpp && /tmp/job_layout_check
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../herro_amd/csrc/job_layout.h"

using namespace herro;

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "case %d: %s (line %d)\n", id, #c, __LINE__); return 1; } } while (0)

struct Input {
  uint64_t n_aln; uint32_t n_targets, n_win; uint64_t txt, cuts, ops; bool try_dev;   // scan block
  JobTotals tot; uint32_t W;                                                          // job blocks
  uint64_t logit_cap;                                                                 // logits block
};

// pieces [0, n) of one block that ends at `end`: 256-byte starts, ascending without overlap, room for what each needs
static int check_pieces(int id, const Piece* p, int n, uint64_t begin, uint64_t end) {
  uint64_t at = begin;
  for (int i = 0; i < n; i++) {
    CHECK(p[i].off % 256 == 0);
    CHECK(p[i].off >= at);
    const uint64_t next = i + 1 < n ? p[i + 1].off : end;
    CHECK(p[i].off + p[i].bytes <= next);
    at = p[i].off + p[i].bytes;
  }
  CHECK(at <= end);
  return 0;
}

static int check_input(int id, const Input& in, ScanLayout& S, JobLayout& L, LogitsLayout& G) {
  // ---- scan block
  S = scan_layout(in.n_aln, in.n_targets, in.n_win, in.txt, in.cuts, in.ops, in.try_dev);
  if (check_pieces(id, S.p, SP_STAGED_N, 0, S.blk_bytes) || check_pieces(id, S.p + SP_STAGED_N, SP_N - SP_STAGED_N, S.blk_bytes, S.dev_blk_bytes)) return 1;
  CHECK(S.at(SP_TEXT) == 0 && S.at(SP_HEAD) == S.blk_bytes && S.blk_bytes == S.at(SP_TOTALS) + 256 && S.blk_bytes % 256 == 0 && S.dev_blk_bytes % 256 == 0);
  CHECK(S.ops_bytes % 256 == 0 && S.ops_bytes >= in.ops * 4 && S.ops_bytes < in.ops * 4 + 256);
  CHECK(S.p[SP_TEXT].bytes == in.txt + 16 && S.p[SP_IN].bytes == in.n_aln * sizeof(CigIn) && S.p[SP_OUT].bytes == in.n_aln * sizeof(CigOut));
  CHECK(S.p[SP_CUTS].bytes == in.cuts * sizeof(CigCut) && S.p[SP_TOTALS].bytes == sizeof(BuildTotals));
  if (in.try_dev) {
    CHECK(S.p[SP_ALN_META].bytes == in.n_aln * sizeof(AlnMeta) && S.p[SP_TGT_META].bytes == in.n_targets * sizeof(TgtMeta) && S.p[SP_WIN_TGT].bytes == (uint64_t)in.n_win * 4);
    CHECK(S.p[SP_HEAD].bytes == in.n_aln * sizeof(AlnHead) && S.p[SP_HOW].bytes == in.cuts * sizeof(HowRec) && S.p[SP_WACC].bytes == in.n_win * sizeof(WinAcc));
    CHECK(S.p[SP_OW_BEGIN].bytes == ((uint64_t)in.n_win + 1) * 4);
    for (int i : {SP_EV_OFF, SP_TILE_OFF, SP_ROW_OFF}) CHECK(S.p[i].bytes == ((uint64_t)in.n_win + 1) * 8);
  } else {   // the pieces of the device build are absent: nothing lies between their neighbours
    CHECK(S.at(SP_OUT) == S.at(SP_ALN_META) && S.dev_blk_bytes == S.blk_bytes);
    for (int i : {SP_ALN_META, SP_TGT_META, SP_WIN_TGT, SP_HEAD, SP_HOW, SP_WACC, SP_OW_BEGIN, SP_EV_OFF, SP_TILE_OFF, SP_ROW_OFF}) CHECK(S.p[i].bytes == 0);
  }
  // an empty piece takes nothing
  for (int i = SP_IN; i + 1 < SP_N; i++) if (S.p[i].bytes == 0) CHECK(S.p[i + 1].off == S.p[i].off);
  {
    unsigned char* const host = (unsigned char*)0x10000, * const arena = (unsigned char*)0x40000000;   // never dereferenced
    const ScanView H = bind_scan_host(host, S), D = bind_scan_dev(arena, S);
    CHECK(H.text == host && (unsigned char*)H.in == host + S.at(SP_IN) && (unsigned char*)H.tot == host + S.at(SP_TOTALS) && !H.ops && !H.head && !H.row_off);
    unsigned char* const blk = arena + S.ops_bytes;
    CHECK((unsigned char*)D.ops == arena && D.text == blk && (unsigned char*)D.am == blk + S.at(SP_ALN_META) && (unsigned char*)D.tm == blk + S.at(SP_TGT_META));
    CHECK((unsigned char*)D.win_tgt == blk + S.at(SP_WIN_TGT) && (unsigned char*)D.out == blk + S.at(SP_OUT) && (unsigned char*)D.cuts == blk + S.at(SP_CUTS));
    CHECK((unsigned char*)D.head == blk + S.at(SP_HEAD) && (unsigned char*)D.how == blk + S.at(SP_HOW) && (unsigned char*)D.wacc == blk + S.at(SP_WACC));
    CHECK((unsigned char*)D.ow_begin == blk + S.at(SP_OW_BEGIN) && (unsigned char*)D.ev_off == blk + S.at(SP_EV_OFF) && (unsigned char*)D.tile_off == blk + S.at(SP_TILE_OFF));
    CHECK((unsigned char*)D.row_off == blk + S.at(SP_ROW_OFF));
    BuildDev B{};
    bind_build_scan(B, D);
    CHECK(B.in == D.in && B.out == D.out && B.cuts == D.cuts && B.am == D.am && B.tm == D.tm && B.win_tgt == D.win_tgt && B.head == D.head && B.how == D.how);
    CHECK(B.wacc == D.wacc && B.tot == D.tot && B.ow_begin == D.ow_begin && B.ev_off == D.ev_off && B.tile_off == D.tile_off && B.row_off == D.row_off);
  }
  // ---- job blocks
  const JobTotals& t = in.tot;
  L = job_layout(t, in.W);
  if (check_pieces(id, L.head, JH_N, 0, L.desc_bytes) || check_pieces(id, L.pin, JP_N, L.desc_bytes, L.pin_bytes) || check_pieces(id, L.dev, JD_N, L.desc_bytes, L.dev_bytes)) return 1;
  CHECK(L.head[0].off == 0 && L.pin[0].off == L.desc_bytes && L.dev[0].off == L.desc_bytes && L.desc_bytes % 256 == 0 && L.pin_bytes % 256 == 0 && L.dev_bytes % 256 == 0);
  for (const Piece& p : L.head) CHECK(&p == L.head || p.off >= (&p)[-1].off + 256);   // at least 16 bytes each: no two pieces share a start
  for (const Piece& p : L.pin) CHECK(&p == L.pin || p.off >= (&p)[-1].off + 256);
  for (const Piece& p : L.dev) CHECK(&p == L.dev || p.off >= (&p)[-1].off + 256);
  // the totals are the end of the last piece under the rule: at least 16 bytes, rounded up to 256
  auto end_of = [](const Piece& p) { return up256(p.off + (p.bytes < 16 ? 16 : p.bytes)); };
  CHECK(L.desc_bytes == end_of(L.head[JH_N - 1]) && L.pin_bytes == end_of(L.pin[JP_N - 1]) && L.dev_bytes == end_of(L.dev[JD_N - 1]));
  CHECK(S.dev_blk_bytes == S.at(SP_ROW_OFF) + up256(S.p[SP_ROW_OFF].bytes));
  const uint64_t nw = (in.W + 31) / 32;
  CHECK(L.head[JH_OPS].bytes == t.op * 4 && L.head[JH_OW].bytes == t.ow * sizeof(OwDesc) && L.head[JH_WIN].bytes == t.win * sizeof(WinDesc));
  CHECK(L.head[JH_TILE_WIN].bytes == t.tile * 4 && L.head[JH_TILE_R0].bytes == t.tile * 4);
  CHECK(L.pin[JP_COUNTS].bytes == t.win * 16 + 16 && L.pin[JP_CONS_LEN].bytes == t.win * 4 && L.pin[JP_CONS_SEQ].bytes == t.row);
  CHECK(L.dev[JD_CW].bytes == (t.ow + 1) * nw * sizeof(PlaneRec) && L.dev[JD_CWD].bytes == (t.ow + 1) * nw * 4 && L.dev[JD_IEV].bytes == t.scr * sizeof(uint4));
  CHECK(L.dev[JD_INS_CNT].bytes == t.ow * 4 && L.dev[JD_OCOL].bytes == t.ow * sizeof(uint4) && L.dev[JD_KEEP].bytes == t.ow && L.dev[JD_ACC].bytes == t.ow * sizeof(float));
  CHECK(L.dev[JD_TTOTAL].bytes == t.ow * 4 && L.dev[JD_SLOT_OW].bytes == t.ow * 4 && L.dev[JD_RANK_QID].bytes == t.ow * 4 && L.dev[JD_SEL_OW].bytes == t.win * 32 * 4);
  CHECK(L.dev[JD_CTAB].bytes == t.win * 32 * sizeof(CTab) && L.dev[JD_CHDR].bytes == t.tile * sizeof(uint2) && L.dev[JD_TILE_NSUP].bytes == t.tile * 4);
  CHECK(L.dev[JD_TEV].bytes == (t.scr + 2 * t.ow) * sizeof(uint4) && L.dev[JD_TILE_EV].bytes == t.tile * sizeof(uint2) && L.dev[JD_COUNTS].bytes >= (4 * t.win + 1) * 4);
  CHECK(L.dev[JD_ROW_OF_POS].bytes == t.pos * 4 && L.dev[JD_ROWMAP].bytes == t.row * 4 && L.dev[JD_CONS_SEQ].bytes == t.row && L.dev[JD_CONS_TMP].bytes == t.row);
  CHECK(L.dev[JD_CONS_LEN].bytes == t.win * 4 && L.dev[JD_SUP_ROW].bytes == t.row * 4 && L.dev[JD_SUP_PI].bytes == t.row * 4 && L.dev[JD_SUP_NR].bytes == t.row * 4);
  CHECK(L.dev[JD_FIN_B].bytes == t.fin && L.dev[JD_FIN_Q].bytes == t.fin && L.dev[JD_ND].bytes == t.cls * 2 * 4 && L.dev[JD_VPL].bytes == t.win * 4 * nw * 4);
  {
    unsigned char* const pin = (unsigned char*)0x10000, * const dev = (unsigned char*)0x40000000;   // never dereferenced
    const JobHead HP = bind_head(pin, L), HD = bind_head(dev, L);
    // the head: identical offsets in the pinned and in the device arena
    CHECK((unsigned char*)HP.ops - pin == (unsigned char*)HD.ops - dev && (unsigned char*)HP.ow - pin == (unsigned char*)HD.ow - dev && (unsigned char*)HP.win - pin == (unsigned char*)HD.win - dev);
    CHECK((unsigned char*)HP.tile_win - pin == (unsigned char*)HD.tile_win - dev && (unsigned char*)HP.tile_r0 - pin == (unsigned char*)HD.tile_r0 - dev);
    CHECK((unsigned char*)HD.ops == dev && (unsigned char*)HD.ow == dev + L.head[JH_OW].off && (unsigned char*)HD.win == dev + L.head[JH_WIN].off);
    CHECK((unsigned char*)HD.tile_win == dev + L.head[JH_TILE_WIN].off && (unsigned char*)HD.tile_r0 == dev + L.head[JH_TILE_R0].off);
    const JobPinTail T = bind_pin_tail(pin, L);
    CHECK((unsigned char*)T.counts == pin + L.pin[JP_COUNTS].off && (unsigned char*)T.cons_len == pin + L.pin[JP_CONS_LEN].off && T.cons_seq == pin + L.pin[JP_CONS_SEQ].off);
    JobDev J{};
    bind_job_dev(J, dev, L, t.win);
    CHECK(J.ops == HD.ops && J.ow == HD.ow && J.win == HD.win && J.tile_win == HD.tile_win && J.tile_r0 == HD.tile_r0);
    const void* got[JD_N] = {J.cw, J.cwd, J.iev, J.ins_cnt, J.ocol, J.ow_keep, J.ow_acc, J.ow_ttotal, J.slot_ow, J.rank_qid, J.sel_ow, J.ctab, J.chdr2, J.tile_nsup, J.tev, J.tile_ev,
                             J.win_Lf, J.row_of_pos2, J.rowmap2, J.cons_seq, J.cons_tmp, J.cons_len, J.sup_row, J.sup_pi, J.fin_b, J.fin_q, J.nd, J.vpl, J.sup_nr};
    for (int i = 0; i < JD_N; i++) CHECK((const unsigned char*)got[i] == dev + L.dev[i].off);
    CHECK(J.win_nsup == J.win_Lf + t.win && J.win_nkept == J.win_Lf + 2 * t.win && J.win_rfbase == J.win_Lf + 3 * t.win && J.rf_alloc == J.win_Lf + 4 * t.win);
    CHECK((const unsigned char*)(J.rf_alloc + 1) <= dev + L.dev[JD_COUNTS].off + L.dev[JD_COUNTS].bytes);
    BuildDev B{};
    bind_build_head(B, HD);
    CHECK(B.ow == HD.ow && B.win == HD.win && B.tile_win == HD.tile_win && B.tile_r0 == HD.tile_r0);
  }
  // ---- logits block
  G = logits_layout(in.logit_cap);
  if (check_pieces(id, G.p, LG_N, 0, G.bytes)) return 1;
  CHECK(G.p[LG_INFO].off == 0 && G.p[LG_INFO].bytes == in.logit_cap * sizeof(float) && G.p[LG_BASE].bytes == in.logit_cap * 5 * sizeof(float));
  CHECK(G.p[LG_RFQ].off % 16 == 0 && G.p[LG_RFQ].bytes == in.logit_cap * HERRO_ROWS * 16 && G.bytes == G.p[LG_RFQ].off + G.p[LG_RFQ].bytes + 256);
  {
    unsigned char* const base = (unsigned char*)0x40000000;
    const LogitsView V = bind_logits(base, G);
    CHECK((unsigned char*)V.info == base && (unsigned char*)V.base == base + G.p[LG_BASE].off && V.rfq == base + G.p[LG_RFQ].off);
  }
  return 0;
}

// (b): what the arithmetic of herro_api.hip at 17fba03 gave for these inputs
struct Fixed {
  Input in;
  uint64_t blk_bytes, dev_blk_bytes, ops_bytes, desc_bytes, pin_bytes, dev_bytes, logits_bytes;
  uint64_t inner[6];   // offsets of CigOut, the window prefixes, WinDesc, tev, sup_nr, the receptive fields
};
static const Fixed FIXED[] = {
  {{0ull, 0u, 0u, 0ull, 0ull, 0ull, false, {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 1u}, 16u, 1ull},
   512ull, 512ull, 0ull, 1280ull, 2048ull, 8704ull, 1264ull, {256ull, 512ull, 512ull, 4864ull, 8448ull, 512ull}},
  {{0ull, 0u, 0u, 0ull, 0ull, 0ull, true, {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 1u}, 8192u, 1ull},
   512ull, 1536ull, 0ull, 1280ull, 2048ull, 12288ull, 1264ull, {256ull, 512ull, 512ull, 8448ull, 12032ull, 512ull}},
  {{5ull, 2u, 9u, 0ull, 23ull, 412ull, true, {0ull, 0ull, 9ull, 9ull, 0ull, 0ull, 4464ull, 144ull, 585ull, 1u}, 64u, 9ull},
   2560ull, 5888ull, 1792ull, 1792ull, 2560ull, 37120ull, 5232ull, {1280ull, 4864ull, 512ull, 19968ull, 36352ull, 512ull}},
  {{5ull, 2u, 9u, 1104ull, 23ull, 557ull, false, {412ull, 17ull, 9ull, 9ull, 4ull, 380ull, 35712ull, 1152ull, 585ull, 1u}, 64u, 1296ull},
   2816ull, 2816ull, 2304ull, 4608ull, 6400ull, 132608ull, 674560ull, {1536ull, 2816ull, 3328ull, 29184ull, 128000ull, 31488ull}},
  {{5ull, 2u, 9u, 1104ull, 23ull, 557ull, true, {0ull, 17ull, 9ull, 9ull, 4ull, 380ull, 35712ull, 1152ull, 585ull, 1u}, 64u, 255ull},
   3584ull, 6912ull, 2304ull, 3072ull, 4864ull, 131072ull, 132880ull, {2304ull, 5888ull, 1792ull, 27648ull, 126464ull, 6144ull}},
  {{1ull, 1u, 1u, 16ull, 3ull, 2ull, true, {0ull, 1ull, 1ull, 1ull, 1ull, 1ull, 496ull, 16ull, 17ull, 1u}, 16u, 64ull},
   2048ull, 3840ull, 256ull, 1280ull, 2048ull, 10496ull, 33536ull, {1280ull, 2816ull, 512ull, 6144ull, 10240ull, 1536ull}},
  {{4096ull, 61u, 4099u, 50331648ull, 20480ull, 25169920ull, true, {0ull, 131072ull, 4099ull, 8131ull, 3900ull, 23068672ull, 520093696ull, 16777216ull, 33583107ull, 1u}, 8192u, 18874368ull},
   51399424ull, 53039104ull, 100679680ull, 10846720ull, 27706368ull, 2795360512ull, 9814671616ull, {50612736ull, 52907008ull, 10486016ull, 928589056ull, 2728251648ull, 452984832ull}},
  {{4096ull, 61u, 4099u, 50331663ull, 20480ull, 25169920ull, false, {21000003ull, 131072ull, 4099ull, 8131ull, 3900ull, 23068672ull, 520093696ull, 16777216ull, 33583107ull, 1u}, 8192u, 7ull},
   51249664ull, 51249664ull, 100679680ull, 94846720ull, 111706368ull, 2879360512ull, 4240ull, {50462976ull, 51249664ull, 94486016ull, 1012589056ull, 2812251648ull, 512ull}},
  {{700ull, 33u, 2111u, 0ull, 2877ull, 90001ull, true, {0ull, 5001ull, 2111ull, 2111ull, 333ull, 0ull, 2094112ull, 67552ull, 8657211ull, 1u}, 4100u, 63ull},
   169984ull, 500736ull, 360192ull, 569344ull, 679168ull, 59232000ull, 33040ull, {55040ull, 433152ull, 400384ull, 14618624ull, 58961664ull, 1536ull}},
  {{3ull, 3u, 3u, 33ull, 9ull, 20ull, true, {0ull, 0ull, 3ull, 0ull, 0ull, 0ull, 0ull, 0ull, 51ull, 1u}, 16u, 65ull},
   2304ull, 4608ull, 256ull, 1280ull, 2048ull, 13312ull, 34544ull, {1280ull, 3584ull, 512ull, 9472ull, 13056ull, 2048ull}},
};

int main(int argc, char** argv) {
  const int n_random = argc > 1 ? std::atoi(argv[1]) : 20000;
  ScanLayout S; JobLayout L; LogitsLayout G;
  int id = 0;
  for (const Fixed& f : FIXED) {
    id--;   // fixed cases count -1, -2, ...
    if (check_input(id, f.in, S, L, G)) return 1;
    CHECK(S.blk_bytes == f.blk_bytes && S.dev_blk_bytes == f.dev_blk_bytes && S.ops_bytes == f.ops_bytes);
    CHECK(L.desc_bytes == f.desc_bytes && L.pin_bytes == f.pin_bytes && L.dev_bytes == f.dev_bytes && G.bytes == f.logits_bytes);
    CHECK(S.at(SP_OUT) == f.inner[0] && S.at(SP_OW_BEGIN) == f.inner[1] && L.head[JH_WIN].off == f.inner[2] && L.dev[JD_TEV].off == f.inner[3]);
    CHECK(L.dev[JD_SUP_NR].off == f.inner[4] && G.p[LG_RFQ].off == f.inner[5]);
  }
  std::mt19937_64 rng(20260);
  auto pick = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); };
  // a count: often zero, often small, sometimes job-sized
  auto count = [&](uint64_t big) { const uint64_t k = pick(0, 9); return k < 2 ? 0 : k < 6 ? pick(0, 40) : pick(0, big); };
  for (id = 0; id < n_random; id++) {
    Input in{};
    in.n_aln = count(200000); in.n_targets = (uint32_t)count(5000); in.n_win = (uint32_t)count(300000);
    in.txt = pick(0, 3) ? count(400000000) : 0;   // no text: the ops are on the device
    in.cuts = count(1000000); in.ops = count(100000000); in.try_dev = pick(0, 2) != 0;
    JobTotals& t = in.tot;
    t.op = pick(0, 1) ? 0 : count(100000000);
    t.ow = count(400000); t.win = count(300000); t.tile = pick(0, 4) ? t.win + count(1000) : 0; t.cls = count(100000);
    t.scr = count(100000000); t.row = count(40000000); t.fin = t.row * HERRO_ROWS; t.pos = t.win * (pick(0, 1) ? 17 : 8193);
    t.max_cols = (uint32_t)pick(1, 500);
    in.W = pick(0, 2) == 0 ? 16 : pick(0, 1) ? 8192 : (uint32_t)pick(16, 8192);
    in.logit_cap = pick(0, 5) ? pick(1, 30000000) : 1;
    if (check_input(id, in, S, L, G)) return 1;
  }
  std::printf("%zu fixed and %d random inputs: ok\n", sizeof FIXED / sizeof FIXED[0], n_random);
  return 0;
}
