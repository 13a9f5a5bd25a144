// job_layout.h — where every array of a job lies inside the blocks herro_job_create carves (job_create.hip, the logits block job_run.hip; DESIGN.md, "Job creation as built"), stated once.
// Plain C++17 over integers, as infer_plan.h and chop_plan.h: no HIP call, no context; job_dev.h, build_dev.h and cigar_dev.h are here for the sizeof of
// the records.  Each block has an enum that IS its order, a function that fills a layout from counts, and one bind function that turns a base pointer and
// the layout into typed pointers — no other code casts into a block.  tools/job_layout_check.cpp drives all of it in a sanitizer build.
//
//   scan block   (ScanLayout)    the records of the CIGAR scan and of the device build: a staged part that a pinned block mirrors, a device-only part
//                                behind it; in front of both, on the device, the job's op array (ops_bytes).  Rule: every piece rounded up to 256 bytes,
//                                an empty piece takes nothing, and the pieces of the device build are absent when it is not tried.
//   job blocks   (JobLayout)     the descriptor HEAD (ops, overlaps, windows, tile list) that opens BOTH the job's pinned arena and its device arena —
//                                one set of offsets, so one copy takes it up —, then the pinned tail (landing zones) or the device tail (every scratch
//                                and result array).  Rule: a piece takes at least 16 bytes, rounded up to 256.
//   logits block (LogitsLayout)  info logits, base logits, compact receptive fields of herro_job_infer.
// The two rounding rules stay two: arena sizes decide which recycled block a job gets (best fit).
#pragma once

#include <cstdint>

#include "build_dev.h"
#include "cigar_dev.h"
#include "job_dev.h"

namespace herro {

// Where a piece starts in its block and the bytes its elements need; its room reaches to the next piece (or the block's end).
struct Piece { uint64_t off = 0, bytes = 0; };

inline uint64_t up256(uint64_t x) { return (x + 255) & ~uint64_t(255); }

// ---- scan block -------------------------------------------------------------------------------------------------------------------
enum ScanPiece {
  // staged: [text][CigIn][AlnMeta][TgtMeta][window -> target] go up in one copy; [CigOut][cuts] come down when the host builds, [totals] when the device does
  SP_TEXT, SP_IN, SP_ALN_META, SP_TGT_META, SP_WIN_TGT, SP_OUT, SP_CUTS, SP_TOTALS,
  // device only (launch_build_phase1): [AlnHead][HowRec][WinAcc], then the four window prefixes in equal slots
  SP_HEAD, SP_HOW, SP_WACC, SP_OW_BEGIN, SP_EV_OFF, SP_TILE_OFF, SP_ROW_OFF,
  SP_N, SP_STAGED_N = SP_HEAD
};

struct ScanLayout {
  Piece p[SP_N];
  uint64_t blk_bytes = 0;       // the staged part: what the pinned staging block mirrors
  uint64_t dev_blk_bytes = 0;   // ... + the device-only part
  uint64_t ops_bytes = 0;       // the op array in front of the block on the device
  bool try_dev = false;
  uint64_t at(ScanPiece i) const { return p[i].off; }
};

// n_aln alignments of n_targets targets with n_win windows; txt_bytes of CIGAR text (0: the ops are on the device already), cut_slots cut records and
// op_slots ops in all.  try_dev: the device build follows the scan.
inline ScanLayout scan_layout(uint64_t n_aln, uint32_t n_targets, uint32_t n_win, uint64_t txt_bytes, uint64_t cut_slots, uint64_t op_slots, bool try_dev) {
  ScanLayout L;
  L.try_dev = try_dev;
  const uint64_t dev = try_dev ? 1 : 0, pfx = dev * ((uint64_t)n_win + 1);
  uint64_t need[SP_N], room[SP_N];
  auto piece = [&](ScanPiece i, uint64_t bytes) { need[i] = bytes; room[i] = up256(bytes); };
  piece(SP_TEXT, txt_bytes + 16);   // the scan kernel reads whole 16-byte pieces
  piece(SP_IN, n_aln * sizeof(CigIn));
  piece(SP_ALN_META, dev * n_aln * sizeof(AlnMeta));
  piece(SP_TGT_META, dev * n_targets * sizeof(TgtMeta));
  piece(SP_WIN_TGT, dev * n_win * 4);
  piece(SP_OUT, n_aln * sizeof(CigOut));
  piece(SP_CUTS, cut_slots * sizeof(CigCut));
  piece(SP_TOTALS, sizeof(BuildTotals));
  room[SP_TOTALS] = 256;
  piece(SP_HEAD, dev * n_aln * sizeof(AlnHead));
  piece(SP_HOW, dev * cut_slots * sizeof(HowRec));
  piece(SP_WACC, dev * n_win * sizeof(WinAcc));
  piece(SP_OW_BEGIN, pfx * 4);
  piece(SP_EV_OFF, pfx * 8);
  piece(SP_TILE_OFF, pfx * 8);
  piece(SP_ROW_OFF, pfx * 8);
  room[SP_OW_BEGIN] = room[SP_EV_OFF];
  uint64_t cur = 0;
  for (int i = 0; i < SP_N; i++) {
    if (i == SP_STAGED_N) L.blk_bytes = cur;
    L.p[i] = Piece{cur, need[i]};
    cur += room[i];
  }
  L.dev_blk_bytes = cur;
  L.ops_bytes = up256(op_slots * 4);
  return L;
}

struct ScanView {
  unsigned char* text;
  CigIn* in; AlnMeta* am; TgtMeta* tm; uint32_t* win_tgt;
  CigOut* out; CigCut* cuts; BuildTotals* tot;
  // the device's view only (null in the pinned mirror's)
  uint32_t* ops;
  AlnHead* head; HowRec* how; WinAcc* wacc;
  uint32_t* ow_begin; uint64_t *ev_off, *tile_off, *row_off;
};

// block: the pinned mirror, blk_bytes long
inline ScanView bind_scan_host(void* block, const ScanLayout& L) {
  unsigned char* b = (unsigned char*)block;
  ScanView V{};
  V.text = b + L.at(SP_TEXT);
  V.in = (CigIn*)(b + L.at(SP_IN)); V.am = (AlnMeta*)(b + L.at(SP_ALN_META)); V.tm = (TgtMeta*)(b + L.at(SP_TGT_META)); V.win_tgt = (uint32_t*)(b + L.at(SP_WIN_TGT));
  V.out = (CigOut*)(b + L.at(SP_OUT)); V.cuts = (CigCut*)(b + L.at(SP_CUTS)); V.tot = (BuildTotals*)(b + L.at(SP_TOTALS));
  return V;
}

// arena: the job's scan arena on the device, [op array: ops_bytes][scan block: dev_blk_bytes]
inline ScanView bind_scan_dev(void* arena, const ScanLayout& L) {
  unsigned char* b = (unsigned char*)arena + L.ops_bytes;
  ScanView V = bind_scan_host(b, L);
  V.ops = (uint32_t*)arena;
  V.head = (AlnHead*)(b + L.at(SP_HEAD)); V.how = (HowRec*)(b + L.at(SP_HOW)); V.wacc = (WinAcc*)(b + L.at(SP_WACC));
  V.ow_begin = (uint32_t*)(b + L.at(SP_OW_BEGIN));
  V.ev_off = (uint64_t*)(b + L.at(SP_EV_OFF)); V.tile_off = (uint64_t*)(b + L.at(SP_TILE_OFF)); V.row_off = (uint64_t*)(b + L.at(SP_ROW_OFF));
  return V;
}

// first phase of the device build: everything it reads and writes lies in the scan block
inline void bind_build_scan(BuildDev& B, const ScanView& V) {
  B.in = V.in; B.out = V.out; B.cuts = V.cuts; B.am = V.am; B.tm = V.tm; B.win_tgt = V.win_tgt;
  B.head = V.head; B.how = V.how; B.wacc = V.wacc; B.tot = V.tot;
  B.ow_begin = V.ow_begin; B.ev_off = V.ev_off; B.tile_off = V.tile_off; B.row_off = V.row_off;
}

// ---- job blocks -------------------------------------------------------------------------------------------------------------------
// What a job holds in all (of a target on the host path: what the targets in front of it hold): the sums every offset of the job follows from.
struct JobTotals {
  uint64_t op = 0, ow = 0, win = 0, tile = 0, cls = 0;   // ops kept in the descriptor head, overlaps, windows, tiles, ratio classes
  uint64_t scr = 0, fin = 0, row = 0, pos = 0;           // op scratch slots, bytes of a final plane set, rows, window positions (W + 1 per window)
  uint32_t max_cols = 1;                                 // 1 + most overlaps of a window
};

inline JobTotals job_totals(const BuildTotals& b, uint32_t n_win, uint32_t n_cls, uint32_t W) {   // the device build: no op lives in the head
  JobTotals t;
  t.ow = b.n_ow; t.win = n_win; t.tile = b.n_tiles; t.cls = n_cls;
  t.scr = b.scr_ops; t.fin = b.fin_bytes; t.row = b.row_elems; t.pos = (uint64_t)n_win * ((uint64_t)W + 1);
  t.max_cols = b.max_cols;
  return t;
}

enum HeadPiece { JH_OPS, JH_OW, JH_WIN, JH_TILE_WIN, JH_TILE_R0, JH_N };
// pinned tail: the per-window counts (L', informative rows, kept overlaps, first receptive-field record; + the records handed out), the corrected bases
enum PinPiece { JP_COUNTS, JP_CONS_LEN, JP_CONS_SEQ, JP_N };
enum DevPiece {
  JD_CW, JD_CWD, JD_IEV, JD_INS_CNT, JD_OCOL, JD_KEEP, JD_ACC, JD_TTOTAL, JD_SLOT_OW, JD_RANK_QID, JD_SEL_OW, JD_CTAB, JD_CHDR, JD_TILE_NSUP, JD_TEV, JD_TILE_EV,
  JD_COUNTS, JD_ROW_OF_POS, JD_ROWMAP, JD_CONS_SEQ, JD_CONS_TMP, JD_CONS_LEN, JD_SUP_ROW, JD_SUP_PI, JD_FIN_B, JD_FIN_Q, JD_ND, JD_VPL, JD_SUP_NR, JD_N
};

struct JobLayout {
  Piece head[JH_N];   // the same in the pinned and in the device arena
  Piece pin[JP_N];    // behind the head in the pinned arena
  Piece dev[JD_N];    // behind the head in the device arena
  uint64_t desc_bytes = 0, pin_bytes = 0, dev_bytes = 0;
};

// pieces of `bytes[i]` from `cur` on; returns the end of the last
inline uint64_t carve_job(Piece* p, const uint64_t* bytes, int n, uint64_t cur) {
  for (int i = 0; i < n; i++) {
    p[i] = Piece{cur, bytes[i]};
    cur = up256(cur + (bytes[i] < 16 ? 16 : bytes[i]));
  }
  return cur;
}

inline JobLayout job_layout(const JobTotals& t, uint32_t W) {
  JobLayout L;
  const uint64_t nw = (W + 31) / 32, n_ow = t.ow, n_win = t.win, n_tiles = t.tile;
  uint64_t h[JH_N], p[JP_N], d[JD_N];
  h[JH_OPS] = t.op * 4; h[JH_OW] = n_ow * sizeof(OwDesc); h[JH_WIN] = n_win * sizeof(WinDesc); h[JH_TILE_WIN] = n_tiles * 4; h[JH_TILE_R0] = n_tiles * 4;
  L.desc_bytes = carve_job(L.head, h, JH_N, 0);
  p[JP_COUNTS] = n_win * 16 + 16; p[JP_CONS_LEN] = n_win * 4; p[JP_CONS_SEQ] = t.row;
  L.pin_bytes = carve_job(L.pin, p, JP_N, L.desc_bytes);
  d[JD_CW] = (n_ow + 1) * nw * sizeof(PlaneRec); d[JD_CWD] = (n_ow + 1) * nw * 4; d[JD_IEV] = t.scr * 16; d[JD_INS_CNT] = n_ow * 4;
  d[JD_OCOL] = n_ow * 16;
  d[JD_KEEP] = n_ow; d[JD_ACC] = n_ow * 4; d[JD_TTOTAL] = n_ow * 4;
  d[JD_SLOT_OW] = n_ow * 4; d[JD_RANK_QID] = n_ow * 4; d[JD_SEL_OW] = n_win * 32 * 4;
  d[JD_CTAB] = n_win * 32 * sizeof(CTab); d[JD_CHDR] = n_tiles * 8; d[JD_TILE_NSUP] = n_tiles * 4;
  d[JD_TEV] = (t.scr + 2 * n_ow) * 16; d[JD_TILE_EV] = n_tiles * 8;
  d[JD_COUNTS] = n_win * 16 + 16;
  d[JD_ROW_OF_POS] = t.pos * 4; d[JD_ROWMAP] = t.row * 4;
  d[JD_CONS_SEQ] = t.row; d[JD_CONS_TMP] = t.row; d[JD_CONS_LEN] = n_win * 4;
  d[JD_SUP_ROW] = t.row * 4; d[JD_SUP_PI] = t.row * 4;
  d[JD_FIN_B] = t.fin; d[JD_FIN_Q] = t.fin; d[JD_ND] = t.cls * 8;
  d[JD_VPL] = n_win * 4 * nw * 4; d[JD_SUP_NR] = t.row * 4;
  L.dev_bytes = carve_job(L.dev, d, JD_N, L.desc_bytes);
  return L;
}

struct JobHead { uint32_t* ops; OwDesc* ow; WinDesc* win; uint32_t *tile_win, *tile_r0; };
inline JobHead bind_head(void* base, const JobLayout& L) {   // base: either arena
  unsigned char* b = (unsigned char*)base;
  return JobHead{(uint32_t*)(b + L.head[JH_OPS].off), (OwDesc*)(b + L.head[JH_OW].off), (WinDesc*)(b + L.head[JH_WIN].off),
                 (uint32_t*)(b + L.head[JH_TILE_WIN].off), (uint32_t*)(b + L.head[JH_TILE_R0].off)};
}

struct JobPinTail { uint32_t *counts, *cons_len; uint8_t* cons_seq; };
inline JobPinTail bind_pin_tail(void* base, const JobLayout& L) {
  unsigned char* b = (unsigned char*)base;
  return JobPinTail{(uint32_t*)(b + L.pin[JP_COUNTS].off), (uint32_t*)(b + L.pin[JP_CONS_LEN].off), b + L.pin[JP_CONS_SEQ].off};
}

// Every pointer of J into the job's device arena: the head, then the tail.  The five counters of a window share JD_COUNTS ([n_win] each, then the one
// allocation counter), so that one copy brings them down: win_Lf is the piece's start.
inline void bind_job_dev(JobDev& J, void* base, const JobLayout& L, uint64_t n_win) {
  unsigned char* b = (unsigned char*)base;
  auto at = [&](DevPiece i) { return b + L.dev[i].off; };
  const JobHead H = bind_head(base, L);
  J.ops = H.ops; J.ow = H.ow; J.win = H.win; J.tile_win = H.tile_win; J.tile_r0 = H.tile_r0;
  J.cw = (PlaneRec*)at(JD_CW); J.cwd = (uint32_t*)at(JD_CWD); J.iev = (uint4*)at(JD_IEV); J.ins_cnt = (uint32_t*)at(JD_INS_CNT); J.ocol = (uint4*)at(JD_OCOL);
  J.ow_keep = (uint8_t*)at(JD_KEEP); J.ow_acc = (float*)at(JD_ACC); J.ow_ttotal = (uint32_t*)at(JD_TTOTAL);
  J.slot_ow = (uint32_t*)at(JD_SLOT_OW); J.rank_qid = (uint32_t*)at(JD_RANK_QID); J.sel_ow = (uint32_t*)at(JD_SEL_OW);
  J.ctab = (CTab*)at(JD_CTAB); J.chdr2 = (uint2*)at(JD_CHDR); J.tile_nsup = (uint32_t*)at(JD_TILE_NSUP);
  J.tev = (uint4*)at(JD_TEV); J.tile_ev = (uint2*)at(JD_TILE_EV);
  uint32_t* counts = (uint32_t*)at(JD_COUNTS);
  J.win_Lf = counts; J.win_nsup = counts + n_win; J.win_nkept = counts + 2 * n_win; J.win_rfbase = counts + 3 * n_win; J.rf_alloc = counts + 4 * n_win;
  J.row_of_pos2 = (uint32_t*)at(JD_ROW_OF_POS); J.rowmap2 = (uint32_t*)at(JD_ROWMAP);
  J.cons_seq = (uint8_t*)at(JD_CONS_SEQ); J.cons_tmp = (uint8_t*)at(JD_CONS_TMP); J.cons_len = (uint32_t*)at(JD_CONS_LEN);
  J.sup_row = (uint32_t*)at(JD_SUP_ROW); J.sup_pi = (uint32_t*)at(JD_SUP_PI);
  J.fin_b = (uint8_t*)at(JD_FIN_B); J.fin_q = (uint8_t*)at(JD_FIN_Q); J.nd = (uint32_t*)at(JD_ND);
  J.vpl = (uint32_t*)at(JD_VPL); J.sup_nr = (uint32_t*)at(JD_SUP_NR);
}

// second phase of the device build: it writes the head of the job's device arena
inline void bind_build_head(BuildDev& B, const JobHead& H) { B.ow = H.ow; B.win = H.win; B.tile_win = H.tile_win; B.tile_r0 = H.tile_r0; }

// ---- logits block -----------------------------------------------------------------------------------------------------------------
// Room for `cap` informative rows: an info logit, five base logits and one 16-byte receptive-field record (8 tokens + 8 qualities) per row of the field.
enum LogitsPiece { LG_INFO, LG_BASE, LG_RFQ, LG_N };
struct LogitsLayout { Piece p[LG_N]; uint64_t bytes = 0; };

inline LogitsLayout logits_layout(uint64_t cap) {
  LogitsLayout L;
  L.p[LG_INFO] = Piece{0, cap * 4};
  L.p[LG_BASE] = Piece{up256(cap * 4), cap * 20};
  L.p[LG_RFQ] = Piece{up256(L.p[LG_BASE].off + cap * 20), cap * HERRO_ROWS * 16};
  L.bytes = L.p[LG_RFQ].off + L.p[LG_RFQ].bytes + 256;
  return L;
}

struct LogitsView { float *info, *base; uint8_t* rfq; };
inline LogitsView bind_logits(void* base, const LogitsLayout& L) {
  unsigned char* b = (unsigned char*)base;
  return LogitsView{(float*)(b + L.p[LG_INFO].off), (float*)(b + L.p[LG_BASE].off), b + L.p[LG_RFQ].off};
}

}  // namespace herro
