// job_create.hip — herro_job_create* of the C ABI (include/herro_amd.h): a job from CIGAR text (herro_job_create) or from device-resident ops
// (herro_job_create_aligned), in stages ("Job creation as built"); herro_job_free and what a job gives back; the host-only test hooks of the
// host build.  Host C++ (compiled by hipcc) over cigar_dev.hip and build_dev.hip; windowing.hpp is the host build, job_layout.h where the arrays lie.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <unordered_map>

#include "aligned_dev.h"
#include "api_job.h"
#include "build_dev.h"
#include "cigar_dev.h"
#include "job_layout.h"
#include "windowing.hpp"

using namespace herro;

// Whatever a job holds of its context goes back when it is destroyed, so a herro_job_create that fails half way just lets go of the job.  Nothing of the
// job may be in flight by then: herro_job_free waits for the stream first, a failed create has waited for whatever it enqueued.
herro_job::~herro_job() {
  if (!ctx) return;
  arena_release(ctx, ctx->free_dev, dev, 1);
  arena_release(ctx, ctx->free_scan, scan, 1);
  arena_release(ctx, ctx->free_pin, pin, 0);
  small_release(ctx, a_logits);
  small_release(ctx, a_bdesc);
  small_release(ctx, a_supoff);
  small_release(ctx, a_supoff_dev);
  if (ev_counts) (void)hipEventDestroy(ev_counts);
  if (ev_blob) (void)hipEventDestroy(ev_blob);
}

namespace {
// Everything herro_job_create derives from ONE target read, with target-local offsets.
struct TargetOut {
  BuildError err;
  std::vector<uint32_t> ops;
  std::vector<OwDesc> ow;    // win / cls / op_begin / scr_off are target-local
  std::vector<WinDesc> win;  // ow_begin target-local; device offsets filled at merge
  uint32_t n_cls = 0;
  uint64_t scr_ops = 0, alg_read_bytes = 0, alg_op_bytes = 0;
  uint32_t n_skipped = 0;   // alignments left out (see skip() in build_target)
  std::vector<std::pair<uint32_t, std::vector<uint32_t>>> op_patches;   // device-scan mode: (slot, ops) of texts only the host could read (e.g. 11+ digit zero padding)
  bool failed = false;      // the whole target was left without overlaps
  std::string first_skip;
};

// Results of the device CIGAR scan of a job's alignments (pinned host copies), indexed like the job's alignment range.
struct DevScanView { const CigIn* in; const CigOut* out; const CigCut* cuts; };

// ds == nullptr: the text is decoded here (scan_cigar) and the ops collect in out.ops.  Otherwise the ops are already in
// the job's device op array (at in[g].op_off, absolute) and only the scan's cut records are read; g0 = index of the
// target's first alignment in the scan arrays.
void build_target(const herro_ctx* ctx, uint32_t rid, const herro_alignment* alns, uint32_t n_aln, uint32_t W,
                  TargetOut& out, const DevScanView* ds = nullptr, uint64_t g0 = 0) {
  auto fail = [&](int code, const std::string& m) { out.err = BuildError{code, m}; };
  if (rid >= ctx->n_reads) return fail(HERRO_E_REFERENCE_PANIC, "target rid out of range (reads[rid])");
  const uint32_t tlen = ctx->read_len[rid];
  const uint32_t n_windows = (tlen + W - 1) / W;  // features.rs:338
  if (n_windows > 65535) return fail(HERRO_E_UNSUPPORTED, "more than 65535 windows in a read (wid is u16 in the reference)");
  // collect (window, overlap) in alignment order, then bucket by window (stable)
  struct Tmp { HostOw h; uint32_t op_base; uint32_t aln; };
  std::vector<Tmp> tmp;
  CigarScan cs;
  std::vector<HostOw> hows;
  std::unordered_map<uint32_t, uint32_t> cls_of_name;  // name class -> accumulator slot
  std::unordered_map<uint32_t, uint32_t> seen_qid;
  // Alignments parse_paf itself would have dropped before extract_features ever saw them (self overlaps, a second
  // alignment of a (query, target) pair — overlaps.rs:175-185) are left out and counted (herro_job_skipped).  Everything
  // else the reference processes is processed — consecutive insertion ops, an alignment that starts inside a window with
  // an insertion, any number of overlaps per window.  Inputs on which the reference PANICS fail the call: the reference
  // would have aborted the run there (Cargo.toml:18).
  auto skip = [&](uint32_t a, const char* why) {
    if (!out.n_skipped++) out.first_skip = "target rid " + std::to_string(rid) + ", alignment " + std::to_string(a) + " (qid " + std::to_string(alns[a].qid) + "): " + why;
  };
  std::vector<uint32_t> spare_ops;   // device-scan mode: ops of the rare alignment the host has to read itself
  if (!ds) {
    size_t op_room = 0;
    for (uint32_t a = 0; a < n_aln; a++) op_room += alns[a].cigar_len / 2 + 1;
    out.ops.reserve(op_room);
  }
  for (uint32_t a = 0; a < n_aln; a++) {
    const herro_alignment& al = alns[a];
    if (al.tid != rid) return fail(HERRO_E_INVALID, "alignment tid != target rid (parse_paf groups by target, overlaps.rs:189-192)");
    if (al.qid >= ctx->n_reads) return fail(HERRO_E_REFERENCE_PANIC, "alignment qid out of range");
    if (al.qid == rid) { skip(a, "self overlap (dropped by parse_paf, overlaps.rs:175-179)"); continue; }
    if (seen_qid.count(al.qid)) { skip(a, "second alignment of the same (query,target) pair (dropped by parse_paf, overlaps.rs:181-185)"); continue; }
    seen_qid[al.qid] = a;
    if (al.tlen != tlen) return fail(HERRO_E_INVALID, "alignment tlen differs from the stored read length");
    if (al.qend > ctx->read_len[al.qid] || al.tend > tlen) return fail(HERRO_E_REFERENCE_PANIC, "alignment coordinates exceed the read length");
    BuildError be;
    uint32_t op_base;
    if (ds) {
      const CigIn& ci = ds->in[g0 + a];
      const CigOut& co = ds->out[g0 + a];
      op_base = ci.op_off;
      if (co.flags & ~(uint32_t)CIG_INS_PAIR) {   // rare: malformed text (the message comes from here), more cuts than the coordinates allow
        spare_ops.resize((size_t)al.cigar_len / 2 + 1);
        if (!scan_cigar(al.cigar, al.cigar_len, al.tstart, W, spare_ops.data(), cs, be)) return fail(be.code, be.msg);
        if (co.flags & CIG_MALFORMED)   // legal text the kernel does not read (lengths padded to 11+ digits): its ops go up from here
          out.op_patches.emplace_back(ci.op_off, std::vector<uint32_t>(spare_ops.begin(), spare_ops.begin() + cs.n_ops));
      } else {
        cs.n_ops = co.n_ops; cs.t_end = co.t_end; cs.q_end = co.q_end; cs.ins_end = co.ins_end; cs.op0 = co.op0; cs.opn = co.opn;
        cs.ins_pairs.clear(); cs.cuts.clear();
        for (uint32_t c = 0; c < co.n_cuts; c++) {
          const CigCut& k = ds->cuts[ci.cut_off + c];
          cs.cuts.push_back(Cut{k.k, k.t, k.q, k.ins, k.o0, k.o1, k.o2});
        }
        std::sort(cs.cuts.begin(), cs.cuts.end(), [](const Cut& x, const Cut& y) { return x.k < y.k; });   // discovery order on the device
      }
    } else {
      // the ops are decoded straight into the target's op array (one pass over the text, scan_cigar); they stay there
      // only if the alignment contributes a window
      op_base = (uint32_t)out.ops.size();
      out.ops.resize((size_t)op_base + al.cigar_len / 2 + 1);
      if (!scan_cigar(al.cigar, al.cigar_len, al.tstart, W, out.ops.data() + op_base, cs, be)) return fail(be.code, be.msg);
    }
    hows.clear();
    if (!window_cuts(cs, al, W, n_windows, hows, be)) return fail(be.code, be.msg);
    if (!ds) out.ops.resize((size_t)op_base + (hows.empty() ? 0u : cs.n_ops));
    for (auto& h : hows) tmp.push_back(Tmp{h, op_base, a});
    const uint32_t nc = ctx->name_class[al.qid];
    if (!cls_of_name.count(nc)) cls_of_name[nc] = out.n_cls++;
  }
  std::vector<uint32_t> cnt(n_windows + 1, 0);
  for (auto& x : tmp) cnt[x.h.win + 1]++;
  for (uint32_t i = 0; i < n_windows; i++) cnt[i + 1] += cnt[i];
  out.ow.resize(tmp.size());
  std::vector<uint32_t> fill(cnt.begin(), cnt.end() - 1);
  std::vector<uint64_t> ins_sum(n_windows, 0);
  for (auto& x : tmp) {
    const herro_alignment& al = alns[x.aln];
    const uint32_t wi = x.h.win;
    const uint32_t win_start = wi * W;
    const uint32_t win_len = (wi == n_windows - 1) ? tlen - wi * W : W;
    OwDesc d{};
    d.win = wi;
    d.qid = al.qid;
    d.cls = cls_of_name[ctx->name_class[al.qid]];
    d.tstart = x.h.tstart;
    d.qlen = x.h.qend - x.h.qstart;
    d.strand = al.strand ? 1 : 0;
    if (x.h.qend < x.h.qstart) return fail(HERRO_E_REFERENCE_PANIC, "window qend < qstart");
    if (d.strand == 0) d.qbeg = al.qstart + x.h.qstart;
    else {
      if (al.qend < x.h.qend) return fail(HERRO_E_REFERENCE_PANIC, "attempt to subtract with overflow (qend - window.qend)");
      d.qbeg = al.qend - x.h.qend;
    }
    d.op_begin = x.op_base + x.h.op_lo;
    d.op_cnt = x.h.op_hi - x.h.op_lo;
    d.start_off = x.h.start_off;
    d.end_off = x.h.end_off;
    d.scr_off = (uint32_t)out.scr_ops;
    d.wtstart = win_start;
    d.wlen = win_len;
    d.t_woff = ctx->h_word_off[rid];
    d.q_woff = ctx->h_word_off[al.qid];
    d.q_qual_off = ctx->h_qual_off[al.qid];
    // ---- validate what the reference would assert / index (features.rs:585-679, 110-237)
    if (x.h.op_hi <= x.h.op_lo) return fail(HERRO_E_REFERENCE_PANIC, "empty cigar slice");
    if (d.tstart < win_start) return fail(HERRO_E_REFERENCE_PANIC, "overlap starts before its window (usize underflow)");
    // a slice may start with an insertion (an alignment that begins inside the window with I ops): its bases go behind the position in
    // front of the overlap's first (features.rs:219-228) — unless there is none: max_ins[tpos - 1] with tpos == 0 panics (features.rs:77)
    if (op_type(x.h.op_first) == OP_I && d.tstart == win_start)
      return fail(HERRO_E_REFERENCE_PANIC, "insertion in front of the window's first position (max_ins[tpos - 1], attempt to subtract with overflow)");
    // target / query bases the TRIMMED slice consumes, from the prefix sums of the parse: the slice's first op loses
    // start_off bases, its last op counts end_off bases (effective-op-length rule, features.rs:82-90); the insertion
    // total stays untrimmed (get_max_ins, features.rs:64-79).  The slice never starts with I (checked per alignment).
    const uint32_t op_f = x.h.op_first, op_l = x.h.op_last;
    uint64_t tt = x.h.st, qq = x.h.sq;
    if (d.op_cnt == 1) {
      if (d.end_off <= d.start_off) return fail(HERRO_E_REFERENCE_PANIC, "cigar_end_offset <= cigar_start_offset");
      const uint32_t e1 = d.end_off - d.start_off, l1 = op_len(op_f);
      if (op_type(op_f) != OP_I) tt = tt - l1 + e1;
      if (op_type(op_f) != OP_D) qq = qq - l1 + e1;
    } else {
      if (op_len(op_f) <= d.start_off) return fail(HERRO_E_REFERENCE_PANIC, "op length <= cigar_start_offset");
      if (d.end_off == 0) return fail(HERRO_E_REFERENCE_PANIC, "Operation length cannot be 0");
      if (op_type(op_f) != OP_I) tt -= d.start_off;
      if (op_type(op_f) != OP_D) qq -= d.start_off;
      const uint32_t ll = op_len(op_l);
      if (op_type(op_l) != OP_I) tt = tt - ll + d.end_off;
      if (op_type(op_l) != OP_D) qq = qq - ll + d.end_off;
    }
    ins_sum[wi] += x.h.si;
    if ((uint64_t)(d.tstart - win_start) + tt > win_len) return fail(HERRO_E_REFERENCE_PANIC, "cigar slice overruns the target window");
    if (qq > d.qlen) return fail(HERRO_E_REFERENCE_PANIC, "cigar slice overruns the query region");
    if ((uint64_t)d.qbeg + d.qlen > ctx->read_len[al.qid]) return fail(HERRO_E_REFERENCE_PANIC, "query region exceeds the query read");
    out.scr_ops += d.op_cnt;
    out.alg_read_bytes += (uint64_t)d.qlen + (d.qlen + 3) / 4;
    out.alg_op_bytes += (uint64_t)d.op_cnt * 4;
    out.ow[fill[wi]++] = d;
  }
  for (uint32_t wi = 0; wi < n_windows; wi++) {
    WinDesc wd{};
    wd.rid = rid; wd.wid = wi; wd.n_wids = n_windows;
    wd.tstart = wi * W;
    wd.win_len = (wi == n_windows - 1) ? tlen - wi * W : W;
    wd.ow_begin = cnt[wi];
    wd.ow_cnt = cnt[wi + 1] - cnt[wi];
    const uint64_t lub = ((uint64_t)wd.win_len + std::min<uint64_t>(ins_sum[wi], (uint64_t)50 * wd.win_len) + 15) & ~15ull;
    wd.lub = (uint32_t)lub;
    out.alg_read_bytes += (uint64_t)wd.win_len + (wd.win_len + 3) / 4;
    out.win.push_back(wd);
  }
}
}  // namespace

// ---- what herro_job_create settles on the host for the device build (round 6) because it needs no CIGAR: who is left out (parse_paf's rules), the ratio
// classes by read name, the windows of every target, the coordinate checks.  false: something this pass would have to report — the host build words it.
// Shared by herro_job_create and herro_job_create_aligned: the records are the same whether their ops arrive as text or from a device-resident handle.
namespace {
struct JobPrepass {
  std::vector<TgtMeta> tmeta;
  std::vector<AlnMeta> ameta;
  std::vector<uint64_t> cls;          // [n_targets + 1] prefix of the targets' ratio classes
  std::vector<uint32_t> skip;         // per target: alignments left out
  std::vector<std::string> first;     // ... and the message for its first
  uint32_t n_win = 0, n_cls = 0;
};

bool job_prepass(herro_ctx* ctx, HostPool& hpool, uint32_t n_targets, const uint32_t* rids, const uint64_t* aln_off, const herro_alignment* alns,
                 uint32_t W, std::vector<uint32_t>& tgt_win_off, JobPrepass& P) {
  const uint64_t a0 = n_targets ? aln_off[0] : 0, nA = n_targets ? aln_off[n_targets] - a0 : 0;
  std::vector<TgtMeta>& tmeta = P.tmeta;
  std::vector<AlnMeta>& ameta = P.ameta;
  tmeta.resize(n_targets);
  ameta.resize(nA);
  uint64_t nwin = 0, ncls = 0;
  for (uint32_t t = 0; t < n_targets; t++) {
    const uint32_t rid = rids[t];
    if (rid >= ctx->n_reads) return false;
    const uint32_t tlen = ctx->read_len[rid], nwt = (tlen + W - 1) / W;
    if (nwt > 65535) return false;
    tmeta[t] = TgtMeta{rid, tlen, nwt, (uint32_t)nwin, (uint32_t)(aln_off[t] - a0), (uint32_t)(aln_off[t + 1] - aln_off[t]), 0, 0};
    tgt_win_off[t] = (uint32_t)nwin;
    nwin += nwt;
  }
  if (nwin > 0xffffffffull || nwin == 0) return false;
  tgt_win_off[n_targets] = (uint32_t)nwin;
  P.cls.assign(n_targets + 1, 0);
  P.skip.assign(n_targets, 0);
  P.first.assign(n_targets, std::string());
  std::atomic<bool> ok{true};
  hpool.run(n_targets, [&](uint32_t t) {
    const TgtMeta& tm_ = tmeta[t];
    std::unordered_map<uint32_t, uint32_t> cls_of_name;
    std::unordered_map<uint32_t, uint32_t> seen_qid;
    uint32_t ncl = 0;
    for (uint32_t a = 0; a < tm_.n_aln; a++) {
      const herro_alignment& al = alns[a0 + tm_.aln0 + a];
      AlnMeta& m = ameta[tm_.aln0 + a];
      m = AlnMeta{al.qid, al.qstart, al.qend, al.tstart, al.tend, al.strand ? 1u : 0u, t, 0};
      if (al.tid != tm_.rid || al.qid >= ctx->n_reads) { ok = false; return; }
      const char* why = nullptr;
      if (al.qid == tm_.rid) why = "self overlap (dropped by parse_paf, overlaps.rs:175-179)";
      else if (seen_qid.count(al.qid)) why = "second alignment of the same (query,target) pair (dropped by parse_paf, overlaps.rs:181-185)";
      if (why) {
        m.flags |= 2u;
        if (!P.skip[t]++) P.first[t] = "target rid " + std::to_string(tm_.rid) + ", alignment " + std::to_string(a) + " (qid " + std::to_string(al.qid) + "): " + why;
        continue;
      }
      seen_qid[al.qid] = a;
      if (al.tlen != tm_.tlen || al.qend > ctx->read_len[al.qid] || al.tend > tm_.tlen) { ok = false; return; }
      const uint32_t nc = ctx->name_class[al.qid];
      auto it = cls_of_name.find(nc);
      if (it == cls_of_name.end()) it = cls_of_name.emplace(nc, ncl++).first;
      m.cls = it->second;   // target-local; the job-level base is added below
    }
    P.cls[t + 1] = ncl;
  });
  if (!ok) return false;
  for (uint32_t t = 0; t < n_targets; t++) P.cls[t + 1] += P.cls[t];
  ncls = P.cls[n_targets];
  if (ncls > 0xffffffffull) return false;
  hpool.run(n_targets, [&](uint32_t t) {
    const TgtMeta& tm_ = tmeta[t];
    for (uint32_t a = 0; a < tm_.n_aln; a++) ameta[tm_.aln0 + a].cls += (uint32_t)P.cls[t];
  });
  P.n_win = (uint32_t)nwin;
  P.n_cls = (uint32_t)ncls;
  return true;
}

// The ops of a job's alignments where they already lie on the device as `len << 2 | type` words (herro_job_create_aligned): alignment i of `alns` has
// n_ops[i] ops from word off[i] of d_store on.
struct OpsSrc { const uint32_t* d_store; const uint64_t* off; const uint32_t* n_ops; };
}  // namespace

// ---- job -------------------------------------------------------------------------------------------
// Job creation in stages ("Job creation as built"): argument checks; the scan plan (host only); staging into the pinned mirror of the scan
// block; the device pass (copies, scan, first phase of the device build, totals); the host build where the device did not settle the job; the job's
// pinned arena and the merge; the device arena and the descriptors' way into it.  Where the arrays lie inside the blocks is job_layout.h's.

// herro_job_create* return a pointer: the code of a failure travels through herro_job_create_status
static herro_job* create_fail(herro_ctx* ctx, int code, const std::string& m) {
  ctx->err = m + " [code " + std::to_string(code) + "]";
  ctx->create_code = code;
  return nullptr;
}

namespace {
using HostClock = std::chrono::steady_clock;
double ms_between(HostClock::time_point a, HostClock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }
struct CreateClock { HostClock::time_point begin, staged, scanned, built, merged; };   // HERRO_HOST_PROFILE: when each stage was over

struct CreateArgs {   // the arguments of herro_job_create*; src: see job_create_from
  herro_ctx* ctx; uint32_t n_targets; const uint32_t* rids; const uint64_t* aln_off; const herro_alignment* alns; uint32_t W; const OpsSrc* src;
  uint64_t a0, nA;    // the job's alignments are alns[a0, a0 + nA)
};

// a block of a free list for the length of a scope (the pinned staging block of one herro_job_create)
struct ArenaHold {
  herro_ctx* ctx; std::vector<Arena>* list; int kind; Arena a{};
  ~ArenaHold() { arena_release(ctx, *list, a, kind); }
};

// ---- stage 2: the scan plan.  One CigIn per alignment, the totals that size the scan block, and where the text comes from.  Host only.
struct ScanPlan {
  std::vector<CigIn> in;
  uint64_t txt = 0, opn = 0, cutn = 0;   // text bytes of the block, op slots, cut slots
  // Zero-copy (round 5): when the texts lie densely inside a range the caller registered (herro_host_register: the PAF text of
  // herro_paf_parse_view, a CIGAR blob), that range goes up in ONE copy from where it is — no staging pass over the bytes (0.9 of the
  // 3.4 ms an unloaded herro_job_create of 4096 windows took, and the part that fights the other feeders for memory bandwidth).  A
  // text keeps its alignment modulo 16: the scan kernel reads aligned 16-byte pieces and skips the bytes in front of the text.
  const unsigned char* t_lo = nullptr;   // the range of the caller's memory that holds the job's texts: [t_lo, t_lo + span)
  uint64_t span = 0, lead = 0;           // lead: t_lo modulo 16
  bool direct = false;                   // the range goes up as it is
  bool read_host = false;                // ... or not at all: the scan kernel reads it at t_dev over PCIe
  const unsigned char* t_dev = nullptr;
};

// (the totals run in locals: one pass over some 10^5 alignments per job on the feeder's own thread, where sums kept in S would go through memory every step)
bool plan_scan(const CreateArgs& A, ScanPlan& S) {
  herro_ctx* ctx = A.ctx;
  if (!A.alns) return create_fail(ctx, HERRO_E_INVALID, "null argument"), false;
  if (A.nA > 0x7fffffffull) return create_fail(ctx, HERRO_E_UNSUPPORTED, "job too large (alignments)"), false;
  const herro_alignment* alns = A.alns + A.a0;
  const uint64_t nA = A.nA;
  const uint32_t W = A.W;
  const OpsSrc* src = A.src;
  S.in.resize(nA);
  CigIn* in = S.in.data();
  uint64_t txt = 0, opn = 0, cutn = 0, txt_sum = 0;
  const unsigned char *t_lo = nullptr, *t_hi = nullptr;
  for (uint64_t g = 0; g < nA; g++) {
    const herro_alignment& al = alns[g];
    const uint32_t cap = (al.tend >= al.tstart ? (al.tend - al.tstart) / W : 0u) + 3u;   // one cut per window boundary the coordinates span, + slack
    if (src) {   // binary ops on the device (k_ops_scan): the slice's first word and its op count; the job's op array has room for exactly that many
      in[g] = CigIn{src->off[A.a0 + g], src->n_ops[A.a0 + g], al.tstart, (uint32_t)opn, (uint32_t)cutn, cap, 0};
      opn += src->n_ops[A.a0 + g];
      cutn += cap;
      continue;
    }
    if (al.cigar_len && !al.cigar) return create_fail(ctx, HERRO_E_INVALID, "alignment without cigar"), false;
    in[g] = CigIn{txt, al.cigar_len, al.tstart, (uint32_t)opn, (uint32_t)cutn, cap, 0};
    txt += ((uint64_t)al.cigar_len + 15) & ~uint64_t(15);
    opn += (uint64_t)al.cigar_len / 2 + 1;
    cutn += cap;
    if (al.cigar_len) {
      txt_sum += al.cigar_len;
      if (!t_lo || al.cigar < t_lo) t_lo = al.cigar;
      if (!t_hi || al.cigar + al.cigar_len > t_hi) t_hi = al.cigar + al.cigar_len;
    }
  }
  S.txt = txt; S.opn = opn; S.cutn = cutn; S.t_lo = t_lo;
  if (opn > 0xffffffffull || cutn > 0xffffffffull) return create_fail(ctx, HERRO_E_UNSUPPORTED, "job too large (ops exceed 2^32)"), false;
  // HERRO_ZERO_COPY: 0 stage every text; 1 (default) copy a registered range up as it is; 2 (round 6, measured in profiles/r6_e2e_ab.txt) no copy at all — the scan kernel
  // reads the registered range over PCIe where the caller has it (no blit kernel, no 50 MB through HBM and back per 4096 windows)
  static const int zc_mode = [] { const char* e = getenv("HERRO_ZERO_COPY"); return e ? atoi(e) : 1; }();
  const uint64_t span = t_lo ? (uint64_t)(t_hi - t_lo) : 0;
  S.span = span;
  S.direct = zc_mode != 0 && t_lo && span <= txt_sum + txt_sum / 2 + 65536 && host_range_registered(t_lo, t_hi, &S.t_dev);
  S.read_host = S.direct && zc_mode == 2 && S.t_dev != nullptr;
  if (!S.direct) return true;
  const uint64_t lead = (uintptr_t)t_lo & 15u;
  for (uint64_t g = 0; g < nA; g++) {
    const herro_alignment& al = alns[g];
    const uint64_t off = al.cigar_len ? lead + (uint64_t)(al.cigar - t_lo) : 0;
    in[g].txt_off = off & ~uint64_t(15);
    in[g].skip = (uint32_t)(off & 15u);
  }
  S.lead = lead;
  S.txt = (lead + span + 31) & ~uint64_t(15);
  g_zero_copy_jobs++;
  return true;
}

// ---- stage 3: staging.  The texts (unless they go up from where they are, or there are none), the records, and for the device build what the pre-pass
// settled, into the pinned mirror `hs` of the scan block.
void stage_scan(const CreateArgs& A, const ScanPlan& S, const JobPrepass& P, const ScanLayout& L, const ScanView& hs, HostPool& hpool) {
  const uint32_t per = 32, nblk = (uint32_t)((A.nA + per - 1) / per);
  if (!S.direct && !A.src) hpool.run(nblk, [&](uint32_t b) {
    for (uint64_t g = (uint64_t)b * per; g < std::min<uint64_t>(A.nA, (uint64_t)(b + 1) * per); g++) {
      const herro_alignment& al = A.alns[A.a0 + g];
      unsigned char* d = hs.text + S.in[g].txt_off;
      if (al.cigar_len) std::memcpy(d, al.cigar, al.cigar_len);
      std::memset(d + al.cigar_len, 0, (size_t)((((uint64_t)al.cigar_len + 15) & ~uint64_t(15)) - al.cigar_len));
    }
  });
  std::memcpy(hs.in, S.in.data(), A.nA * sizeof(CigIn));
  if (!L.try_dev) return;
  std::memcpy(hs.am, P.ameta.data(), A.nA * sizeof(AlnMeta));
  std::memcpy(hs.tm, P.tmeta.data(), (size_t)A.n_targets * sizeof(TgtMeta));
  hpool.run(A.n_targets, [&](uint32_t t) { for (uint32_t w = 0; w < P.tmeta[t].n_windows; w++) hs.win_tgt[P.tmeta[t].win0 + w] = t; });
  std::memset(hs.tot, 0, sizeof(BuildTotals));
}

// ---- stage 4: the device pass, on the context's prep stream.  The staged part goes up, the scan kernel writes the job's op array and the cut records; with
// the device build behind it (L.try_dev) the first build phase follows and 64 bytes of totals come down instead of the records.
//   BUILT        the device settled the job: *btot holds its totals, BD is bound for the second phase
//   HOST_BUILDS  the scan's records are in `hs`: the host cuts the windows from them (and words whatever is wrong with the input)
//   UNSETTLED    (ops from the device only) the text path rebuilds the job; the stream is idle: the totals' event has been waited for
//   FAILED       reported
// HERRO_HOST_PROFILE: copy up / kernels / copy down on the device clock, here and nowhere else.
enum class DevPass { BUILT, HOST_BUILDS, UNSETTLED, FAILED };

DevPass device_pass(const CreateArgs& A, const ScanPlan& S, const ScanLayout& L, const ScanView& hs, const ScanView& dv, uint32_t n_win, BuildDev& BD,
                    BuildTotals& btot, bool prof, const CreateClock& clk) {
  herro_ctx* ctx = A.ctx;
  const hipStream_t st = ctx->prep_stream;
  const uint64_t up_bytes = L.at(SP_OUT) - L.at(SP_IN), down_bytes = L.at(SP_TOTALS) - L.at(SP_OUT);   // [CigIn .. window -> target], [CigOut][cuts]
  hipEvent_t pe[4] = {nullptr, nullptr, nullptr, nullptr};
  if (prof) for (auto& ev : pe) (void)hipEventCreate(&ev);
  auto drop_events = [&] { for (auto& ev : pe) if (ev) (void)hipEventDestroy(ev); };
  if (pe[0]) (void)hipEventRecord(pe[0], st);
  hipError_t e;
  if (S.direct) {   // the texts from the caller's registered range (same alignment modulo 16), the alignment records from the staging block
    e = S.read_host ? hipSuccess : hipMemcpyAsync(dv.text + S.lead, S.t_lo, S.span, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(dv.in, hs.in, up_bytes, hipMemcpyHostToDevice, st);
  } else if (A.src) {   // no text: the alignment records alone
    e = hipMemcpyAsync(dv.in, hs.in, up_bytes, hipMemcpyHostToDevice, st);
  } else {
    e = hipMemcpyAsync(dv.text, hs.text, L.at(SP_OUT), hipMemcpyHostToDevice, st);
  }
  if (L.try_dev && e == hipSuccess) e = hipMemcpyAsync(dv.tot, hs.tot, sizeof(BuildTotals), hipMemcpyHostToDevice, st);
  if (pe[1]) (void)hipEventRecord(pe[1], st);
  if (e == hipSuccess && A.src) {
    launch_ops_scan(A.src->d_store, dv.in, dv.out, dv.cuts, dv.ops, &dv.tot->err, BLD_SCAN_FLAG, (uint32_t)A.nA, A.W, st);
    e = hipGetLastError();
  } else if (e == hipSuccess) {
    launch_cigar_scan(S.read_host ? S.t_dev - S.lead : dv.text, dv.in, dv.out, dv.cuts, dv.ops, (uint32_t)A.nA, A.W, st);
    e = hipGetLastError();
  }
  if (pe[2]) (void)hipEventRecord(pe[2], st);
  bool dev_built = false;
  if (L.try_dev && e == hipSuccess) {   // windows and counts behind the scan
    bind_build_scan(BD, dv);
    BD.n_aln = (uint32_t)A.nA; BD.n_tgt = A.n_targets; BD.n_win = n_win; BD.W = A.W;
    BD.read_word_off = ctx->d_word_off; BD.read_qual_off = ctx->d_qual_off;
    launch_build_phase1(BD, dv.ow_begin, dv.ev_off, dv.tile_off, dv.row_off, st);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(hs.tot, dv.tot, sizeof(BuildTotals), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipEventRecord(ctx->prep_ev, st);
    if (e == hipSuccess) e = hipEventSynchronize(ctx->prep_ev);
    if (e == hipSuccess) {
      std::memcpy(&btot, hs.tot, sizeof btot);
      dev_built = btot.err == 0;
    }
  }
  if (A.src && e == hipSuccess && !dev_built) { drop_events(); return DevPass::UNSETTLED; }
  if (!dev_built) {
    if (e == hipSuccess) e = hipMemcpyAsync(hs.out, dv.out, down_bytes, hipMemcpyDeviceToHost, st);
    if (pe[3]) (void)hipEventRecord(pe[3], st);
    if (e == hipSuccess) e = hipEventRecord(ctx->prep_ev, st);
    if (e == hipSuccess) e = hipEventSynchronize(ctx->prep_ev);
  } else if (pe[3]) (void)hipEventRecord(pe[3], st);
  if (prof && e == hipSuccess) {
    float up = 0, kn = 0, dn = 0;
    (void)hipEventElapsedTime(&up, pe[0], pe[1]); (void)hipEventElapsedTime(&kn, pe[1], pe[2]); (void)hipEventElapsedTime(&dn, pe[2], pe[3]);
    fprintf(stderr, "  cigar scan: %.1f MiB text staged in %.2f ms; device: copy up %.2f ms, kernel %.2f, copy down %.2f (%.1f MiB); wall %.2f ms\n", S.txt / 1048576.0,
            ms_between(clk.begin, clk.staged), up, kn, dn, (dev_built ? 64.0 : (double)down_bytes) / 1048576.0, ms_between(clk.staged, HostClock::now()));
  }
  drop_events();
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(st);
    create_fail(ctx, HERRO_E_NO_DEVICE, std::string("CIGAR scan failed: ") + hipGetErrorString(e));
    return DevPass::FAILED;
  }
  return dev_built ? DevPass::BUILT : DevPass::HOST_BUILDS;
}

// what the device build settled besides its totals (job_totals): the algorithmic bytes; the pre-pass knows who was left out
void adopt_device_build(herro_job* job, const BuildTotals& btot, const JobPrepass& P) {
  job->alg_read_bytes = btot.rd_bytes; job->alg_op_bytes = btot.op_bytes;
  for (size_t t = 0; t < P.skip.size(); t++)
    if (P.skip[t]) {
      if (!job->n_skipped_alns) job->first_skip = P.first[t];
      job->n_skipped_alns += P.skip[t];
    }
}

// ---- stage 5: the host build.  Per-target host work (CIGAR parse or the scan's records in `ds`, windowing, validation) is independent: it runs on the
// context's thread pool, each target into its own buffers with target-local offsets.  A serial pass over the per-target SIZES then fixes every base
// offset: base[t] is what the targets in front of t hold, base[n_targets] the job.
bool host_build(const CreateArgs& A, const DevScanView* ds, HostPool& hpool, herro_job* job, std::vector<TargetOut>& outs, std::vector<JobTotals>& base,
                CreateClock& clk) {
  herro_ctx* ctx = A.ctx;
  outs.resize(A.n_targets);
  hpool.run(A.n_targets, [&](uint32_t t) {
    build_target(ctx, A.rids[t], A.alns + A.aln_off[t], (uint32_t)(A.aln_off[t + 1] - A.aln_off[t]), A.W, outs[t], ds, A.aln_off[t] - A.a0);
  });
  clk.built = HostClock::now();
  base.resize(A.n_targets + 1);
  JobTotals b;
  for (uint32_t t = 0; t < A.n_targets; t++) {
    const TargetOut& o = outs[t];
    if (o.err.code != HERRO_OK) return create_fail(ctx, o.err.code, "target " + std::to_string(t) + " (rid " + std::to_string(A.rids[t]) + "): " + o.err.msg), false;
    if (o.n_skipped) {
      if (!job->n_skipped_alns && !job->n_failed_targets) job->first_skip = o.first_skip;
      job->n_skipped_alns += o.n_skipped;
      job->n_failed_targets += o.failed ? 1u : 0u;
    }
    for (auto& pt : o.op_patches) {   // rare; synchronous
      if (hipMemcpy((uint32_t*)job->scan.p + pt.first, pt.second.data(), pt.second.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
        return create_fail(ctx, HERRO_E_NO_DEVICE, "op upload failed"), false;
    }
    base[t] = b;
    b.op += o.ops.size(); b.ow += o.ow.size(); b.win += o.win.size(); b.cls += o.n_cls; b.scr += o.scr_ops;
    for (const WinDesc& wd : o.win) {
      b.tile += (wd.lub + HERRO_TILE - 1) / HERRO_TILE;
      b.fin += (uint64_t)HERRO_ROWS * wd.lub; b.row += wd.lub; b.pos += (uint64_t)A.W + 1;
      b.max_cols = std::max(b.max_cols, wd.ow_cnt + 1);
    }
    if (b.op > 0xffffffffull) return create_fail(ctx, HERRO_E_UNSUPPORTED, "job too large (ops exceed 2^32)"), false;
    job->alg_read_bytes += o.alg_read_bytes;
    job->alg_op_bytes += o.alg_op_bytes;
    job->tgt_win_off[t + 1] = (uint32_t)b.win;
  }
  base[A.n_targets] = b;
  return true;
}

// ---- stage 6: the job's pinned arena — the descriptor head, then the landing zones of the counts and of the corrected bases
bool bind_job_pin(herro_ctx* ctx, herro_job* job, const JobLayout& L, const JobTotals& tot) {
  job->pin = arena_acquire(ctx, ctx->free_pin, L.pin_bytes, 0);
  if (!job->pin.p) return create_fail(ctx, HERRO_E_NO_DEVICE, "out of pinned host memory for the job"), false;
  const JobHead H = bind_head(job->pin.p, L);
  job->ops.p = H.ops; job->ops.n = tot.op;
  job->ow.p = H.ow; job->ow.n = tot.ow;
  job->win.p = H.win; job->win.n = tot.win;
  job->tile_win.p = H.tile_win; job->tile_win.n = tot.tile;
  job->tile_r0.p = H.tile_r0; job->tile_r0.n = tot.tile;
  const JobPinTail T = bind_pin_tail(job->pin.p, L);
  job->h_counts = T.counts; job->h_cons_len = T.cons_len; job->h_cons_seq = T.cons_seq;
  return true;
}

// ... and the merge in target order (host build): the bytes are copied, and the target-local indices rebased, by the pool, straight into the head of the
// pinned arena
void merge_targets(herro_job* job, std::vector<TargetOut>& outs, const std::vector<JobTotals>& base, uint32_t W, HostPool& hpool) {
  hpool.run((uint32_t)outs.size(), [&](uint32_t t) {
    TargetOut& o = outs[t];
    const JobTotals& b = base[t];
    if (!o.ops.empty()) std::memcpy(job->ops.data() + b.op, o.ops.data(), o.ops.size() * 4);
    for (size_t i = 0; i < o.ow.size(); i++) {
      OwDesc d = o.ow[i];
      d.win += (uint32_t)b.win; d.cls += (uint32_t)b.cls; d.op_begin += (uint32_t)b.op; d.scr_off += (uint32_t)b.scr;
      job->ow[b.ow + i] = d;
    }
    uint64_t fin = b.fin, row = b.row, pos = b.pos, tile = b.tile, evo = b.scr + 2 * b.ow;
    for (size_t i = 0; i < o.win.size(); i++) {
      WinDesc wd = o.win[i];
      wd.ev_off = evo;
      for (uint32_t k = 0; k < wd.ow_cnt; k++) evo += o.ow[wd.ow_begin + k].op_cnt + 2u;   // target-local ow_begin here
      wd.ow_begin += (uint32_t)b.ow;
      wd.col_off = tile;   // first tile of the window
      wd.fin_off = fin; fin += (uint64_t)HERRO_ROWS * wd.lub;
      wd.row_off = row; row += wd.lub;
      wd.pos_off = pos; pos += (uint64_t)W + 1;
      for (uint32_t r0 = 0; r0 < wd.lub; r0 += HERRO_TILE) { job->tile_win[tile] = (uint32_t)(b.win + i); job->tile_r0[tile] = r0; tile++; }
      job->win[b.win + i] = wd;
    }
    o = TargetOut();  // release
  });
}

// ---- stage 7: the device arena and the descriptors' way into it.  ops_in_scan: the ops lie in the job's scan arena (the device scanned them).
// BD: bound by the device pass when it built the job (null: the host did).
bool job_to_device(herro_ctx* ctx, herro_job* job, const JobLayout& L, const JobTotals& tot, bool ops_in_scan, BuildDev* BD) {
  JobDev& J = job->J;
  J.read_words = ctx->d_words; J.read_word_off = ctx->d_word_off; J.read_p0 = ctx->d_p0; J.read_p1 = ctx->d_p1;
  J.read_qual = ctx->d_qual; J.read_qual_off = ctx->d_qual_off; J.read_qual_bytes = ctx->qual_bytes; J.read_n_words = ctx->n_words;
  J.ln_table = ctx->d_ln; J.ln_table_n = ctx->ln_n;
  J.prof = ctx->d_prof;
  J.n_ow = (uint32_t)tot.ow; J.n_win = (uint32_t)tot.win; J.n_cls = (uint32_t)tot.cls;
  J.n_tiles = (uint32_t)tot.tile; J.window_size = job->W; J.nw = (job->W + 31) / 32; J.max_cols = tot.max_cols;
  { const char* e = getenv("HERRO_DEBUG_CDIR_OVERFLOW"); J.dbg_flags = (e && atoi(e)) ? 1u : 0u; }
  job->dev = arena_acquire(ctx, ctx->free_dev, L.dev_bytes, 1);
  if (!job->dev.p) return create_fail(ctx, HERRO_E_NO_DEVICE, "out of device memory for the job (" + std::to_string(L.dev_bytes >> 20) + " MiB)"), false;
  bind_job_dev(J, job->dev.p, L, tot.win);
  if (ops_in_scan) J.ops = (const uint32_t*)job->scan.p;
  job->d_counts = J.win_Lf;
  J.rf = nullptr; J.rf_cap = 0; J.rf_half = 0;
  hipError_t e;
  if (BD) {
    // the descriptors are written where they are read (build_dev.hip, behind the scan on the prep stream); the window descriptors come down — the host hands
    // windows out by them — and the context's stream waits for the event, so the kernels of herro_job_featurize queue behind the build in stream order
    bind_build_head(*BD, bind_head(job->dev.p, L));
    launch_build_phase2(*BD, ctx->prep_stream);
    e = hipGetLastError();
    if (e == hipSuccess && J.n_win) e = hipMemcpyAsync(job->win.data(), BD->win, (size_t)J.n_win * sizeof(WinDesc), hipMemcpyDeviceToHost, ctx->prep_stream);
    if (e == hipSuccess) e = hipEventRecord(ctx->prep_ev, ctx->prep_stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream, ctx->prep_ev, 0);
    if (e == hipSuccess) e = hipEventSynchronize(ctx->prep_ev);
    job->dev_built = true;
  } else {
    // one copy, pinned -> device, asynchronous on the context stream: the head has the same layout in both arenas.  The kernels of herro_job_featurize
    // queue behind it in stream order, nobody waits here
    e = hipMemcpyAsync(job->dev.p, job->pin.p, L.desc_bytes, hipMemcpyHostToDevice, ctx->stream);
  }
  if (e == hipSuccess) e = hipEventCreateWithFlags(&job->ev_counts, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&job->ev_blob, hipEventDisableTiming);
  if (e == hipSuccess) return true;
  (void)hipStreamSynchronize(ctx->stream);
  return create_fail(ctx, HERRO_E_NO_DEVICE, std::string("descriptor upload failed: ") + hipGetErrorString(e)), false;
}
}  // namespace

// herro_job_create (src == nullptr: the ops come as CIGAR text) and the direct path of herro_job_create_aligned (src: they are on the device; the caller
// has checked that the context builds on the device).  *unsettled is raised, with nothing reported, when the direct path does not settle the job: the
// caller then goes through the text of the job's ops.  A job that is let go of half way returns what it holds (~herro_job).
static herro_job* job_create_from(herro_ctx* ctx, uint32_t n_targets, const uint32_t* rids, const uint64_t* aln_off,
                                  const herro_alignment* alns, uint32_t W, const OpsSrc* src, bool* unsettled) {
  if (!ctx) return nullptr;
  ctx->create_code = HERRO_OK;
  if (!ctx->d_words && !ctx->host_only) return create_fail(ctx, HERRO_E_STATE, "herro_set_reads must be called first");
  if (W < 16 || W > HERRO_MAX_WINDOW) return create_fail(ctx, HERRO_E_UNSUPPORTED, "window_size must be in [16, 8192]");
  if (n_targets && (!rids || !aln_off)) return create_fail(ctx, HERRO_E_INVALID, "null argument");
  if (!ctx->host_only && hipSetDevice(ctx->device) != hipSuccess) return create_fail(ctx, HERRO_E_NO_DEVICE, "hipSetDevice failed");
  const uint64_t a0 = n_targets ? aln_off[0] : 0;
  const CreateArgs A{ctx, n_targets, rids, aln_off, alns, W, src, a0, n_targets ? aln_off[n_targets] - a0 : 0};

  const bool prof = getenv("HERRO_HOST_PROFILE") != nullptr;
  ProfSpan span_(ctx, "create");
  CreateClock clk;
  clk.begin = clk.scanned = HostClock::now();
  auto job = std::make_unique<herro_job>();
  job->ctx = ctx;
  job->W = W;
  job->n_targets = n_targets;
  job->tgt_win_off.assign(n_targets + 1, 0);
  HostPool& hpool = host_pool(ctx);

  // ---- the CIGAR text goes to the GPU first (cigar_dev.hip): one kernel (a workgroup per alignment) writes the binary ops into the job's op array and
  // returns, per alignment, the totals and the ops that reach a window boundary.  Device build (round 6): what needs no CIGAR is settled by the pre-pass
  // and goes up beside the text; anything it would have to report sends the job down the host path, which words it.
  ArenaHold stage{ctx, &ctx->free_stage, 0};
  JobPrepass P;
  BuildDev BD{};
  BuildTotals btot{};
  DevScanView dsv{nullptr, nullptr, nullptr};
  bool scanned = false, dev_built = false;
  if (!ctx->host_only && ctx->dev_scan && A.nA) {
    ScanPlan S;
    if (!plan_scan(A, S)) return nullptr;
    const bool try_dev = ctx->dev_build && job_prepass(ctx, hpool, n_targets, rids, aln_off, alns, W, job->tgt_win_off, P);
    if (src && !try_dev) { *unsettled = true; return nullptr; }
    const ScanLayout SL = scan_layout(A.nA, n_targets, P.n_win, S.txt, S.cutn, S.opn, try_dev);
    stage.a = arena_acquire(ctx, ctx->free_stage, SL.blk_bytes, 0);
    job->scan = arena_acquire(ctx, ctx->free_scan, SL.ops_bytes + SL.dev_blk_bytes, 1);
    if (!stage.a.p || !job->scan.p)
      return create_fail(ctx, HERRO_E_NO_DEVICE, "out of memory for the CIGAR scan (" + std::to_string((SL.ops_bytes + SL.dev_blk_bytes) >> 20) + " MiB)");
    const ScanView hs = bind_scan_host(stage.a.p, SL), dv = bind_scan_dev(job->scan.p, SL);
    stage_scan(A, S, P, SL, hs, hpool);
    clk.staged = HostClock::now();
    switch (device_pass(A, S, SL, hs, dv, P.n_win, BD, btot, prof, clk)) {
      case DevPass::FAILED: return nullptr;
      case DevPass::UNSETTLED: *unsettled = true; return nullptr;
      case DevPass::BUILT: dev_built = true; break;
      case DevPass::HOST_BUILDS: break;
    }
    dsv = DevScanView{hs.in, hs.out, hs.cuts};
    scanned = true;
    job->scan_ops = S.opn;
    clk.scanned = HostClock::now();
  }
  std::vector<TargetOut> outs;
  std::vector<JobTotals> base;   // host build: per target, what lies in front of it
  JobTotals tot;
  if (dev_built) {
    clk.built = HostClock::now();
    adopt_device_build(job.get(), btot, P);
    tot = job_totals(btot, P.n_win, P.n_cls, W);
  } else {
    if (!host_build(A, scanned ? &dsv : nullptr, hpool, job.get(), outs, base, clk)) return nullptr;
    tot = base[n_targets];
  }
  // the windows' event slices live behind scr_ops + 2 * n_ow slots and are indexed with 32 bits on the device (WinDesc::ev_off -> CTab::ev_off)
  if (tot.scr + 2ull * tot.ow > 0xffffffffull) return create_fail(ctx, HERRO_E_UNSUPPORTED, "job too large (op scratch exceeds 2^32)");
  // (what was left out is reported by herro_job_skipped; the error slot is for errors only)
  const JobLayout L = job_layout(tot, W);
  if (!bind_job_pin(ctx, job.get(), L, tot)) return nullptr;
  if (!dev_built) merge_targets(job.get(), outs, base, W, hpool);
  job->row_elems = tot.row;
  job->reads_gen = ctx->reads_gen;
  clk.merged = HostClock::now();
  if (ctx->host_only) {  // test hook: the host half (descriptors) only
    if (prof) fprintf(stderr, "herro_job_create (host half): build %.2f ms, merge %.2f (%zu windows)\n", ms_between(clk.begin, clk.built), ms_between(clk.built, clk.merged), job->win.size());
  } else {
    if (!job_to_device(ctx, job.get(), L, tot, scanned, dev_built ? &BD : nullptr)) return nullptr;
    if (prof)
      fprintf(stderr, "herro_job_create: scan %.2f ms, build %.2f, merge %.2f, arena + enqueue %.2f (%u windows, %zu MiB device)\n", ms_between(clk.begin, clk.scanned),
              ms_between(clk.scanned, clk.built), ms_between(clk.built, clk.merged), ms_between(clk.merged, HostClock::now()), job->J.n_win, (size_t)(L.dev_bytes >> 20));
  }
  ctx->live_jobs++;
  return job.release();
}

extern "C" {

herro_job* herro_job_create(herro_ctx* ctx, uint32_t n_targets, const uint32_t* rids, const uint64_t* aln_off,
                            const herro_alignment* alns, uint32_t W) {
  return job_create_from(ctx, n_targets, rids, aln_off, alns, W, nullptr, nullptr);
}

int herro_job_create_status(const herro_ctx* ctx) { return ctx ? ctx->create_code.load() : HERRO_E_INVALID; }

int herro_job_skipped(const herro_job* job, uint32_t* n_alignments, uint32_t* n_targets) {
  if (!job) return HERRO_E_INVALID;
  if (n_alignments) *n_alignments = job->n_skipped_alns;
  if (n_targets) *n_targets = job->n_failed_targets;
  return HERRO_OK;
}

void herro_job_free(herro_job* job) {
  if (!job) return;
  herro_ctx* ctx = job->ctx;
  if (ctx->live_jobs.load()) ctx->live_jobs--;
  if (job->pending) { job->pending = false; ctx->n_pending--; }   // featurized, never inferred
  ctx->sib_suspects.erase(std::remove(ctx->sib_suspects.begin(), ctx->sib_suspects.end(), job), ctx->sib_suspects.end());
  if (ctx->host_only) { delete job; return; }
  ProfSpan span_(ctx, "destroy");
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);   // nothing of this job is in flight once its memory is recycled
  delete job;
}

int herro_debug_set_host_build(herro_ctx* ctx, int on) {
  if (!ctx) return HERRO_E_INVALID;
  ctx->dev_build = on == 0;
  return HERRO_OK;
}

int herro_debug_job_dev_built(const herro_job* job) { return job ? (job->dev_built && !job->from_ops_text ? 1 : 0) : HERRO_E_INVALID; }

// ---- host-only test hooks: the host half of herro_job_create without a device ------------------------
// herro_debug_host_ctx builds a context that only knows the read lengths (and name classes); herro_job_create on it
// runs CIGAR parsing, windowing, validation and the merge, then stops; herro_debug_job_array exposes the descriptors.
herro_ctx* herro_debug_host_ctx(uint32_t n_reads, const uint32_t* read_len, const uint32_t* name_class) {
  auto ctx = new herro_ctx();
  ctx->host_only = true;
  ctx->n_reads = n_reads;
  ctx->read_len.assign(read_len, read_len + n_reads);
  ctx->name_class.resize(n_reads);
  for (uint32_t i = 0; i < n_reads; i++) ctx->name_class[i] = name_class ? name_class[i] : i;
  ctx->h_word_off.assign(n_reads + 1, 0);
  ctx->h_qual_off.assign(n_reads + 1, 0);
  for (uint32_t i = 0; i < n_reads; i++) {  // the layout herro_set_reads produces
    ctx->h_word_off[i + 1] = ctx->h_word_off[i] + ((uint64_t)read_len[i] + 31) / 32;
    ctx->h_qual_off[i + 1] = ctx->h_qual_off[i] + read_len[i];
  }
  return ctx;
}

// ---- host-only test hook: the product's windowing on one alignment (no device needed) -----------
// out rows of 8 u64: window, tstart, qstart, qend, op_lo, op_hi, start_off, end_off.
int64_t herro_debug_extract_windows(const herro_alignment* a, uint32_t n_windows, uint32_t W, uint64_t* out,
                                    uint64_t cap, char* err, uint64_t err_cap) {
  std::vector<uint32_t> ops;
  std::vector<HostOw> hows;
  BuildError be;
  if (!a || !parse_cigar(a->cigar, a->cigar_len, ops, be) || !window_alignment(ops, *a, W, n_windows, hows, be)) {
    if (err && err_cap) { std::strncpy(err, a ? be.msg.c_str() : "null", err_cap - 1); err[err_cap - 1] = 0; }
    return a ? be.code : HERRO_E_INVALID;
  }
  if (hows.size() > cap) return HERRO_E_INVALID;
  for (size_t k = 0; k < hows.size(); k++) {
    uint64_t* o = out + 8 * k;
    o[0] = hows[k].win; o[1] = hows[k].tstart; o[2] = hows[k].qstart; o[3] = hows[k].qend;
    o[4] = hows[k].op_lo; o[5] = hows[k].op_hi; o[6] = hows[k].start_off; o[7] = hows[k].end_off;
  }
  return (int64_t)hows.size();
}

// ---- a job from device-resident alignments (the handle and its helpers: aligned_dev.h, frontend_api.hip) ----------------------
herro_job* herro_job_create_aligned(herro_ctx* ctx, uint32_t n_targets, const uint32_t* rids, const uint64_t* aln_off, const uint32_t* rec,
                                    const herro_aligned_dev* a, uint32_t W) {
  if (!ctx) return nullptr;
  auto fail = [&](int code, const std::string& m) { return create_fail(ctx, code, m); };
  ctx->create_code = HERRO_OK;
  if (!a) return fail(HERRO_E_INVALID, "herro_job_create_aligned: null handle");
  if (n_targets && (!rids || !aln_off)) return fail(HERRO_E_INVALID, "null argument");
  const uint64_t a0 = n_targets ? aln_off[0] : 0, a1 = n_targets ? aln_off[n_targets] : 0;
  if (a1 < a0) return fail(HERRO_E_INVALID, "aln_off must ascend");
  if (a1 > a0 && !rec) return fail(HERRO_E_INVALID, "herro_job_create_aligned: null rec");
  if (a->ctx != ctx) return fail(HERRO_E_INVALID, "herro_job_create_aligned: the handle belongs to another context");
  // the job's records, in its order: coordinates from the handle, ops by reference
  std::vector<herro_alignment> sel(a1);
  std::vector<uint64_t> off(a1, 0);
  std::vector<uint32_t> nops(a1, 0);
  uint64_t lo = ~0ull, hi = 0;
  for (uint64_t g = a0; g < a1; g++) {
    const uint32_t r = rec[g];
    if (r >= a->alns.size())
      return fail(HERRO_E_INVALID, "herro_job_create_aligned: rec[" + std::to_string(g) + "] = " + std::to_string(r) + " is outside the handle's " + std::to_string(a->alns.size()) + " records");
    if (!a->n_ops[r])
      return fail(HERRO_E_INVALID, "herro_job_create_aligned: rec[" + std::to_string(g) + "] = " + std::to_string(r) + " is a failed record (no ops)");
    sel[g] = a->alns[r];
    off[g] = a->op_off[r];
    nops[g] = a->n_ops[r];
    lo = std::min(lo, off[g]);
    hi = std::max(hi, off[g] + nops[g]);
  }
  if (!ctx->host_only && ctx->dev_scan && ctx->dev_build && a1 > a0) {   // direct: k_ops_scan reads the handle's store, no text anywhere
    const OpsSrc src{a->d_ops, off.data(), nops.data()};
    bool unsettled = false;
    herro_job* job = job_create_from(ctx, n_targets, rids, aln_off, sel.data(), W, &src, &unsettled);
    if (job || !unsettled) return job;
  }
  // Not taken (host build, host scan, a device-free context) or not settled (BuildTotals::err, the pre-pass): this job's ops come down, are formatted and
  // go through herro_job_create, whose results and error texts are then the text path's by construction.  The span [lo, hi) of the store comes down in one copy.
  std::vector<uint32_t> ops;
  if (a1 > a0) {
    const int rc = aligned_dev_fetch(a, lo, hi, ops);
    if (rc != HERRO_OK) return fail(rc, "herro_job_create_aligned: copying the ops down failed");
  }
  for (uint64_t g = a0; g < a1; g++) off[g] -= lo;
  std::string text;
  ops_text_block(ctx, ops.data(), off.data(), nops.data(), a0, a1, sel.data(), text);
  herro_job* job = herro_job_create(ctx, n_targets, rids, aln_off, sel.data(), W);
  if (job) job->from_ops_text = true;
  return job;
}

}  // extern "C"
