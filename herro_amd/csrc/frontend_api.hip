// frontend_api.hip — the C ABI's front end (include/herro_amd.h): reads alone -> overlap records -> their ops on the device.
// herro_find_overlaps[_core], herro_extend_overlaps, herro_align_overlaps[_dev], herro_aligned_dev_*, herro_find_overlap_pairs[_core], herro_pairs_*, the PAF / .oec.zst
// writer (herro_aligned_dev_paf, herro_pairs_paf, herro_pairs_write_alns) herro_set_seed_rescue, herro_set_chain_params, herro_set_index_params with herro_index_plan (csrc/index_plan.h), and the test hooks herro_debug_sketch, herro_debug_occ_census, herro_debug_seed_rescue and herro_debug_chain.  Host C++ (compiled by
// hipcc) over overlap_dev.hip, align_dev.hip and paf_dev.hip; contexts are herro_api.hip, the model model_api.hip, jobs job_create.hip, job_run.hip and job_out.hip.  Ahead of them all, for raw reads:
// herro_find_adapters and its handle, over adapter_dev.hip (the plan and the cut are host code: fastx.cpp), and herro_store_cut with its test hook
// herro_debug_store_copy, over store_dev.hip: the store cut to the plan's pieces on the device.  The primitives every device stage stands on have hooks of
// their own: herro_debug_scan_u32, herro_debug_radix_sort (scan_sort_dev.hip) and herro_debug_offsets64 (fasta_dev.hip's offset join).  Behind the finder: herro_cluster_graph, herro_pairs_cluster and
// herro_clusters_*, over cluster_dev.hip (the checks and the part rule are host code: cluster_plan.h): the reads partitioned by their overlap graph.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>

#include "adapter_dev.h"
#include "aligned_dev.h"
#include "align_dev.h"
#include "alns_file.h"
#include "cluster_dev.h"
#include "cluster_plan.h"
#include "dev_bufs.h"
#include "fasta_dev.h"
#include "index_plan.h"
#include "overlap_dev.h"
#include "paf_dev.h"
#include "scan_sort_dev.h"
#include "store_dev.h"

namespace {
constexpr uint32_t SLICE = 1u << 20;   // records per turn of herro_extend_overlaps and herro_aligned_dev_mirror: their descriptors and results stay small whatever n is

// A HIP call of a front-end entry failed: "<who>: <what>: <HIP's text>" and HERRO_E_NO_DEVICE.  Scratch in a Bufs goes with the return.
int hip_failed(herro_ctx* ctx, const char* who, const char* what, hipError_t e) {
  ctx->err = std::string(who) + ": " + what + ": " + hipGetErrorString(e);
  return HERRO_E_NO_DEVICE;
}
#define FRONT_TRY(ctx, who, what, expr) do { const hipError_t _e = (expr); if (_e != hipSuccess) return hip_failed(ctx, who, what, _e); } while (0)

// What every front-end entry (`who`) asks of a context's state before anything runs.
int device_ready(herro_ctx* ctx, const char* who) {
  if (ctx->host_only) { ctx->err = std::string(who) + ": the context has no device"; return HERRO_E_NO_DEVICE; }
  if (!ctx->d_words) { ctx->err = "herro_set_reads must be called first"; return HERRO_E_STATE; }
  return HERRO_OK;
}

herro::OvlStore ovl_store(const herro_ctx* ctx) { return herro::OvlStore{ctx->d_words, ctx->d_word_off, ctx->d_qual_off, ctx->read_len.data(), ctx->n_reads}; }

using AlignedDevPtr = std::unique_ptr<herro_aligned_dev, void (*)(herro_aligned_dev*)>;
AlignedDevPtr new_aligned_dev(herro_ctx* ctx) {
  AlignedDevPtr h(new herro_aligned_dev(), herro_aligned_dev_free);
  h->ctx = ctx; h->device = ctx->device; h->host_only = ctx->host_only;
  return h;
}

uint32_t dec_digits(uint32_t v) { uint32_t k = 1; while (v >= 10) { v /= 10; k++; } return k; }
// bytes of "<len><M|I|D>" per op
uint64_t ops_text_bytes(const uint32_t* ops, uint32_t n) {
  uint64_t b = 0;
  for (uint32_t x = 0; x < n; x++) b += dec_digits(ops[x] >> 2) + 1;
  return b;
}
char* ops_text(const uint32_t* ops, uint32_t n, char* p) {
  for (uint32_t x = 0; x < n; x++) {
    p += snprintf(p, 12, "%u", ops[x] >> 2);
    *p++ = "MID?"[ops[x] & 3u];   // ('?': type 3 of a caller's own ops; herro_job_create refuses the letter)
  }
  return p;
}

// One record's result in its handle: a failed record is counted, gets INT32_MIN and 0 ops and keeps its coordinates; any other its score, its op
// count and the coordinates after fix_cigar dropped a leading / trailing indel.
void fold_result(const herro::AlignOut& o, herro_alignment& a, int32_t& score, uint32_t& n_ops, uint32_t& failed) {
  if (o.failed) { score = INT32_MIN; n_ops = 0; failed++; return; }
  score = o.score;
  n_ops = o.n_ops;
  a.tstart += o.tdrop0; a.tend -= o.tdrop1;
  if (a.strand == 0) { a.qstart += o.qdrop0; a.qend -= o.qdrop1; }
  else { a.qend -= o.qdrop0; a.qstart += o.qdrop1; }
}

// What herro_align_overlaps[_dev], herro_extend_overlaps and herro_aligned_dev_mirror (`who`) ask of a context and of coordinate-only records before anything runs.
int check_record_fields(herro_ctx* ctx, const char* who, uint32_t n, const herro_alignment* in);
int check_records(herro_ctx* ctx, const char* who, uint32_t n, const herro_alignment* in) {
  if (const int rc = device_ready(ctx, who)) return rc;
  return check_record_fields(ctx, who, n, in);
}
// ... and of the records alone (herro_pairs_from_table, which a device-free context may call)
int check_record_fields(herro_ctx* ctx, const char* who, uint32_t n, const herro_alignment* in) {
  for (uint32_t r = 0; r < n; r++) {
    const herro_alignment& a = in[r];
    std::string why;
    if (a.qid >= ctx->n_reads || a.tid >= ctx->n_reads) why = "read id outside the read store";
    else if (a.qstart > a.qend || a.qend > ctx->read_len[a.qid]) why = "query coordinates outside the read";
    else if (a.tstart > a.tend || a.tend > ctx->read_len[a.tid]) why = "target coordinates outside the read";
    else if (a.strand > 1) why = "strand must be 0 or 1";
    else if ((uint64_t)(a.qend - a.qstart) + (a.tend - a.tstart) > herro::ALIGN_MAX_CELLS) why = "overlap longer than 2^25 bases in all";
    if (!why.empty()) {
      ctx->err = std::string(who) + ": record " + std::to_string(r) + ": " + why;
      return HERRO_E_INVALID;
    }
  }
  return HERRO_OK;
}

// Validation, chunking (HERRO_ALIGN_SCRATCH_MB) and the kernel runs of herro_align_overlaps and herro_align_overlaps_dev.  Behind every chunk the host
// reads its op total and its AlignOut records and hands the chunk's dense ops, still on the device, to take(total, d_dense, r_done, at): it stores them and
// says where (at: the chunk's first op in the caller's store; r_done: records aligned so far, this chunk's included).  ops_at[r]: record r's first op there.
template <class Take>
int align_chunks(herro_ctx* ctx, uint32_t n, const herro_alignment* in, std::vector<herro::AlignOut>& res, std::vector<uint64_t>& ops_at, Take take) {
  const char* const who = "herro_align_overlaps";
  if (const int rc = check_records(ctx, who, n, in)) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const uint64_t budget = scratch_budget("HERRO_ALIGN_SCRATCH_MB");
  std::vector<herro::AlignIn> recs(n);
  res.resize(n);
  ops_at.assign(n, 0);
  // chunks: consecutive records whose scratch fits the budget (a record larger than the budget runs alone)
  uint64_t max_scr = 0, max_dense = 0;
  std::vector<uint32_t> cut{0};
  {
    uint64_t acc = 0, dn = 0;
    for (uint32_t r = 0; r < n; r++) {
      const uint32_t qn = in[r].qend - in[r].qstart, tm = in[r].tend - in[r].tstart;
      const uint64_t need = herro::align_scratch_bytes(qn, tm);
      if (acc && acc + need > budget) { cut.push_back(r); acc = 0; dn = 0; }
      recs[r] = herro::AlignIn{ctx->h_word_off[in[r].tid], ctx->h_word_off[in[r].qid], acc, in[r].tstart, tm, in[r].qstart, qn, in[r].strand, 0};
      acc += need;
      dn += (uint64_t)qn + tm + 1;
      max_scr = std::max(max_scr, acc);
      max_dense = std::max(max_dense, dn);
    }
    if (cut.back() != n) cut.push_back(n);
  }
  herro::Bufs B;
  uint8_t* d_scr = nullptr;
  herro::AlignIn* d_in = nullptr;
  herro::AlignOut* d_out = nullptr;
  uint32_t *d_dense = nullptr, *d_count = nullptr;
  if (n) {
    FRONT_TRY(ctx, who, "scratch", B.bytes(&d_scr, std::max<uint64_t>(max_scr, 256)));
    FRONT_TRY(ctx, who, "records", B.bytes(&d_in, sizeof(herro::AlignIn) * n));
    FRONT_TRY(ctx, who, "results", B.bytes(&d_out, sizeof(herro::AlignOut) * n));
    FRONT_TRY(ctx, who, "ops", B.bytes(&d_dense, 4 * std::max<uint64_t>(max_dense, 1)));
    FRONT_TRY(ctx, who, "counter", B.bytes(&d_count, 4));
    FRONT_TRY(ctx, who, "record upload", hipMemcpyAsync(d_in, recs.data(), sizeof(herro::AlignIn) * n, hipMemcpyHostToDevice, ctx->stream));
  }
  for (size_t c = 0; c + 1 < cut.size(); c++) {
    const uint32_t r0 = cut[c], r1 = cut[c + 1];
    FRONT_TRY(ctx, who, "counter reset", hipMemsetAsync(d_count, 0, 4, ctx->stream));
    herro::launch_align(ctx->d_words, d_in + r0, d_out + r0, d_scr, d_dense, d_count, r1 - r0, ctx->stream);
    FRONT_TRY(ctx, who, "k_align launch", hipGetLastError());
    uint32_t total = 0;
    FRONT_TRY(ctx, who, "count", hipMemcpyAsync(&total, d_count, 4, hipMemcpyDeviceToHost, ctx->stream));
    FRONT_TRY(ctx, who, "results", hipMemcpyAsync(res.data() + r0, d_out + r0, sizeof(herro::AlignOut) * (r1 - r0), hipMemcpyDeviceToHost, ctx->stream));
    FRONT_TRY(ctx, who, "k_align", hipStreamSynchronize(ctx->stream));
    uint64_t at = 0;
    FRONT_TRY(ctx, who, "ops", take(total, d_dense, r1, at));
    for (uint32_t r = r0; r < r1; r++) ops_at[r] = at + res[r].ops_off;
  }
  FRONT_TRY(ctx, who, "ops", hipStreamSynchronize(ctx->stream));   // (a device-resident store: its last copy has landed)
  return HERRO_OK;
}

int overlap_params(herro_ctx* ctx, const herro_overlap_params* in, herro::OvlParams& P) {
  const herro_overlap_params z{};
  const herro_overlap_params& p = in ? *in : z;
  P.k = p.k ? p.k : 25;
  P.w = p.w ? p.w : 17;
  P.occ_frac_ppm = p.occ_frac_ppm;
  P.max_occ = p.max_occ ? p.max_occ : (P.occ_frac_ppm ? 0 : 128);   // (with a fraction: the ceiling of the cut, 0 = none)
  P.bandwidth = p.bandwidth ? p.bandwidth : 150;
  P.max_gap = p.max_gap ? p.max_gap : 5000;
  P.min_score = p.min_score ? p.min_score : 2500;
  P.min_anchors = p.min_anchors ? p.min_anchors : 3;
  if (P.k < 5 || P.k > 31 || P.w > 64) {
    ctx->err = "overlap parameters: 5 <= k <= 31 and 1 <= w <= 64";
    return HERRO_E_INVALID;
  }
  P.occ_dist = ctx->seed_rescue.occ_dist;       // herro_set_seed_rescue (validated there)
  P.rescue_max_occ = ctx->seed_rescue.rescue_max_occ ? ctx->seed_rescue.rescue_max_occ : 4095;
  P.lookback = ctx->chain_lookback;             // herro_set_chain_params (validated there)
  P.index_kmers = ctx->index_parts.max_kmers;   // herro_set_index_params (validated there)
  P.occ_ranges = ctx->index_parts.occ_ranges;
  if (P.occ_frac_ppm > 999999) {
    ctx->err = "overlap parameters: occ_frac_ppm must be below 1000000 (0: the fixed cut max_occ)";
    return HERRO_E_INVALID;
  }
  return HERRO_OK;
}

// HERRO_OVL_STATS=1 (tools/overlaprate.py): the sizes of the finder's stages, one line on stderr; a second one for the cut taken from the index
void print_ovl_stats(const herro::OvlParams& P, const herro::OvlStats& stats) {
  const char* e = getenv("HERRO_OVL_STATS");
  if (!e || !atoi(e)) return;
  fprintf(stderr, "OVL kmers=%llu minimizers=%llu anchors=%llu groups=%llu chained=%llu chunks=%llu\n", (unsigned long long)stats.kmers,
          (unsigned long long)stats.minimizers, (unsigned long long)stats.anchors, (unsigned long long)stats.groups,
          (unsigned long long)stats.chained, (unsigned long long)stats.chunks);
  if (P.occ_frac_ppm)
    fprintf(stderr, "OVLOCC cut=%llu distinct=%llu cut_runs=%llu cut_minimizers=%llu\n", (unsigned long long)stats.occ_cut,
            (unsigned long long)stats.distinct, (unsigned long long)stats.cut_runs, (unsigned long long)stats.cut_minimizers);
  if (P.occ_dist)
    fprintf(stderr, "OVLRESC high=%llu rescued=%llu anchors=%llu\n", (unsigned long long)stats.resc_high, (unsigned long long)stats.rescued,
            (unsigned long long)stats.resc_anchors);
  if (P.lookback != herro::OVL_LOOKBACK)
    fprintf(stderr, "OVLCHAIN lookback=%u chained=%llu\n", P.lookback, (unsigned long long)stats.chained);
  if (P.index_kmers)
    fprintf(stderr, "OVLPART blocks=%llu pairs=%llu ranges=%llu peak_bytes=%llu\n", (unsigned long long)stats.blocks,
            (unsigned long long)stats.block_pairs, (unsigned long long)stats.ranges, (unsigned long long)stats.peak_bytes);
}

// A call's core mask (n_reads bytes, non-zero: the read is a target) goes up once, into the call's scratch; NULL stays NULL: every read is core.
int upload_core(herro_ctx* ctx, const char* who, const uint8_t* core, herro::Bufs& B, uint8_t** d_core) {
  *d_core = nullptr;
  if (!core) return HERRO_OK;
  FRONT_TRY(ctx, who, "core mask", B.bytes(d_core, std::max<uint64_t>(ctx->n_reads, 1)));
  FRONT_TRY(ctx, who, "core mask upload", hipMemcpyAsync(*d_core, core, ctx->n_reads, hipMemcpyHostToDevice, ctx->stream));
  return HERRO_OK;
}

int overlap_rc(herro_ctx* ctx, int rc, const std::string& msg) {
  if (rc == herro::OVL_OK) return HERRO_OK;
  ctx->err = msg;
  return rc == herro::OVL_UNSUPPORTED ? HERRO_E_UNSUPPORTED : HERRO_E_NO_DEVICE;
}
}  // namespace

int aligned_dev_fetch(const herro_aligned_dev* a, uint64_t lo, uint64_t hi, std::vector<uint32_t>& v) {
  v.resize(hi - lo);
  if (hi == lo) return HERRO_OK;
  if (a->host_only) { std::memcpy(v.data(), a->h_ops.data() + lo, (hi - lo) * 4); return HERRO_OK; }
  if (hipSetDevice(a->device) != hipSuccess || hipMemcpy(v.data(), a->d_ops + lo, (hi - lo) * 4, hipMemcpyDeviceToHost) != hipSuccess) return HERRO_E_NO_DEVICE;
  return HERRO_OK;
}

void ops_text_block(herro_ctx* ctx, const uint32_t* ops, const uint64_t* at, const uint32_t* n_ops, uint64_t r0, uint64_t r1, herro_alignment* alns,
                    std::string& text) {
  std::vector<uint64_t> toff(r1 + 1, 0);
  for (uint64_t r = r0; r < r1; r++) toff[r + 1] = toff[r] + ops_text_bytes(ops + at[r], n_ops[r]);
  text.assign(toff[r1] + 1, '\0');
  host_pool(ctx).run((uint32_t)((r1 - r0 + 63) / 64), [&](uint32_t b) {
    for (uint64_t r = r0 + (uint64_t)b * 64; r < std::min(r1, r0 + (uint64_t)(b + 1) * 64); r++) {
      ops_text(ops + at[r], n_ops[r], &text[toff[r]]);
      alns[r].cigar = reinterpret_cast<const uint8_t*>(text.data() + toff[r]);
      alns[r].cigar_len = (uint32_t)(toff[r + 1] - toff[r]);
    }
  });
}

extern "C" {

// ---- base-level alignment of coordinate-only overlaps (align_dev.hip) ------------------------------------------------
// The step `herro inference` hands to `minimap2 -cx ava-ont` when it is not given --read-alns (mm2.rs:15-30), followed by
// fix_cigar (aligners.rs:138-250): records in chunks that fit HERRO_ALIGN_SCRATCH_MB of traceback scratch, one kernel per
// chunk on the context's stream, the ops back to the host and formatted into one text block there.
struct herro_aligned {
  std::vector<herro_alignment> alns;
  std::vector<int32_t> scores;
  std::string text;
  uint32_t failed = 0;
};

int herro_align_overlaps(herro_ctx* ctx, uint32_t n, const herro_alignment* in, herro_aligned** out) {
  if (!ctx || !out || (n && !in)) return HERRO_E_INVALID;
  *out = nullptr;
  std::vector<herro::AlignOut> res;
  std::vector<uint32_t> ops;            // every record's final ops, record order
  std::vector<uint64_t> ops_at;
  const int rc = align_chunks(ctx, n, in, res, ops_at, [&](uint32_t total, const uint32_t* d_dense, uint32_t, uint64_t& at) {
    at = ops.size();
    ops.resize(at + total);
    return total ? hipMemcpy(ops.data() + at, d_dense, 4ull * total, hipMemcpyDeviceToHost) : hipSuccess;
  });
  if (rc != HERRO_OK) return rc;
  auto* h = new herro_aligned();
  h->alns.assign(in, in + n);
  h->scores.resize(n);
  std::vector<uint32_t> n_ops(n);
  for (uint32_t r = 0; r < n; r++) fold_result(res[r], h->alns[r], h->scores[r], n_ops[r], h->failed);
  ops_text_block(ctx, ops.data(), ops_at.data(), n_ops.data(), 0, n, h->alns.data(), h->text);
  *out = h;
  return HERRO_OK;
}

const herro_alignment* herro_aligned_alignments(const herro_aligned* a) { return a ? a->alns.data() : nullptr; }
const int32_t* herro_aligned_scores(const herro_aligned* a) { return a ? a->scores.data() : nullptr; }
uint32_t herro_aligned_failed(const herro_aligned* a) { return a ? a->failed : 0; }
void herro_aligned_free(herro_aligned* a) { delete a; }

// ---- extension of coordinate-only overlaps to the read ends (k_extend in align_dev.hip) ----------------------------------------
// Two sides per record, one wave each; the host turns the four flank lengths into coordinates.  Records go through in slices of 2^20, so the side
// descriptors and results (72 B per side) stay small whatever n is.
struct herro_extended {
  std::vector<herro_alignment> alns;   // extended coordinates; cigar = NULL, cigar_len = 0
  std::vector<uint32_t> ext;           // [n][4]: t_left, q_left, t_right, q_right
  std::vector<int32_t> scores;         // [n][2]: left, right
};

int herro_extend_overlaps(herro_ctx* ctx, uint32_t n, const herro_alignment* in, const herro_extend_params* params, herro_extended** out) {
  if (!ctx || !out || (n && !in)) return HERRO_E_INVALID;
  *out = nullptr;
  const char* const who = "herro_extend_overlaps";
  const uint32_t zdrop = params && params->zdrop ? params->zdrop : herro::EXTEND_ZDROP;
  const uint32_t max_ext = params && params->max_ext ? params->max_ext : herro::EXTEND_MAX_EXT;
  if (max_ext > herro::EXTEND_MAX_EXT_LIMIT) { ctx->err = "herro_extend_overlaps: max_ext must be at most 2^20"; return HERRO_E_INVALID; }
  if (const int rc = check_records(ctx, who, n, in)) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  std::unique_ptr<herro_extended> h(new herro_extended());
  h->alns.assign(in, in + n);
  h->ext.assign((size_t)n * 4, 0);
  h->scores.assign((size_t)n * 2, 0);
  const uint32_t cap = std::min(n, SLICE);
  std::vector<herro::ExtIn> sides((size_t)cap * 2);
  std::vector<herro::ExtOut> res((size_t)cap * 2);
  herro::Bufs B;
  herro::ExtIn* d_in = nullptr;
  herro::ExtOut* d_out = nullptr;
  if (n) FRONT_TRY(ctx, who, "sides", B.bytes(&d_in, sizeof(herro::ExtIn) * sides.size()));
  if (n) FRONT_TRY(ctx, who, "results", B.bytes(&d_out, sizeof(herro::ExtOut) * res.size()));
  for (uint32_t r0 = 0; r0 < n; r0 += SLICE) {
    const uint32_t cnt = std::min(SLICE, n - r0);
    for (uint32_t x = 0; x < cnt; x++) {
      const herro_alignment& a = in[r0 + x];
      const uint64_t tw = ctx->h_word_off[a.tid], qw = ctx->h_word_off[a.qid];
      const uint32_t t_below = a.tstart, t_above = ctx->read_len[a.tid] - a.tend;
      const uint32_t q_below = a.qstart, q_above = ctx->read_len[a.qid] - a.qend;
      // left: the target below tstart read downwards; the oriented query in front of the span read backwards — the forward bases below qstart read
      // downwards (strand 0) or those from qend upwards (strand 1), complemented like the target's (T rev = 1, Q rev = !strand: the same equalities)
      const uint32_t ml = std::min(t_below, max_ext), nl = std::min(a.strand ? q_above : q_below, max_ext);
      sides[2 * x] = herro::ExtIn{tw, qw, a.tstart - ml, ml, a.strand ? a.qend : a.qstart - nl, nl, 1u, a.strand ? 0u : 1u};
      // right: the target from tend upwards; the oriented query behind the span
      const uint32_t mr = std::min(t_above, max_ext), nr = std::min(a.strand ? q_below : q_above, max_ext);
      sides[2 * x + 1] = herro::ExtIn{tw, qw, a.tend, mr, a.strand ? a.qstart - nr : a.qend, nr, 0u, a.strand};
    }
    FRONT_TRY(ctx, who, "side upload", hipMemcpyAsync(d_in, sides.data(), sizeof(herro::ExtIn) * 2 * cnt, hipMemcpyHostToDevice, ctx->stream));
    herro::launch_extend(ctx->d_words, d_in, d_out, zdrop, 2 * cnt, ctx->stream);
    FRONT_TRY(ctx, who, "k_extend launch", hipGetLastError());
    FRONT_TRY(ctx, who, "results", hipMemcpyAsync(res.data(), d_out, sizeof(herro::ExtOut) * 2 * cnt, hipMemcpyDeviceToHost, ctx->stream));
    FRONT_TRY(ctx, who, "k_extend", hipStreamSynchronize(ctx->stream));
    for (uint32_t x = 0; x < cnt; x++) {
      herro_alignment& a = h->alns[r0 + x];
      const herro::ExtOut &l = res[2 * x], &r = res[2 * x + 1];
      a.cigar = nullptr; a.cigar_len = 0;
      a.tstart -= l.j; a.tend += r.j;
      if (a.strand == 0) { a.qstart -= l.i; a.qend += r.i; }
      else { a.qend += l.i; a.qstart -= r.i; }
      uint32_t* ex = &h->ext[(size_t)(r0 + x) * 4];
      ex[0] = l.j; ex[1] = l.i; ex[2] = r.j; ex[3] = r.i;
      h->scores[(size_t)(r0 + x) * 2] = l.score;
      h->scores[(size_t)(r0 + x) * 2 + 1] = r.score;
    }
  }
  *out = h.release();
  return HERRO_OK;
}

uint32_t herro_extended_n(const herro_extended* x) { return x ? (uint32_t)x->alns.size() : 0; }
const herro_alignment* herro_extended_alignments(const herro_extended* x) { return x ? x->alns.data() : nullptr; }
const uint32_t* herro_extended_ext(const herro_extended* x) { return x ? x->ext.data() : nullptr; }
const int32_t* herro_extended_scores(const herro_extended* x) { return x ? x->scores.data() : nullptr; }
void herro_extended_free(herro_extended* x) { delete x; }

// ---- device-resident hand-off: the aligner's ops stay where k_align wrote them, the job builder reads them there ----------------
int herro_align_overlaps_dev(herro_ctx* ctx, uint32_t n, const herro_alignment* in, herro_aligned_dev** out) {
  if (!ctx || !out || (n && !in)) return HERRO_E_INVALID;
  *out = nullptr;
  AlignedDevPtr h = new_aligned_dev(ctx);
  std::vector<herro::AlignOut> res;
  // The store grows by chunks: the first chunk's ops per record, projected over all records plus an eighth, sizes it; a chunk that does not fit moves it
  // to twice the projection (device to device, behind the chunk's synchronisation: nothing reads the old block any more).
  const int rc = align_chunks(ctx, n, in, res, h->op_off, [&](uint32_t total, const uint32_t* d_dense, uint32_t r_done, uint64_t& at) {
    at = h->used;
    if (!total) return hipSuccess;
    hipError_t e;
    if (h->used + total > h->cap) {
      const uint64_t proj = (h->used + total) * (uint64_t)n / std::max(r_done, 1u);
      const uint64_t cap = std::max<uint64_t>(h->used + total, (h->cap ? 2 : 1) * (proj + proj / 8)) + 1024;
      uint32_t* const old = h->d_ops;
      uint32_t* d = nullptr;
      if ((e = hipMalloc((void**)&d, cap * 4)) != hipSuccess) return e;
      h->d_ops = d; h->cap = cap;   // (the handle's from here on, whatever follows)
      e = h->used ? hipMemcpyAsync(d, old, h->used * 4, hipMemcpyDeviceToDevice, ctx->stream) : hipSuccess;
      if (old) {
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        (void)hipFree(old);
      }
      if (e != hipSuccess) return e;
    }
    // (stream order: the next chunk's kernel, which overwrites d_dense, queues behind this copy)
    if ((e = hipMemcpyAsync(h->d_ops + h->used, d_dense, 4ull * total, hipMemcpyDeviceToDevice, ctx->stream)) != hipSuccess) return e;
    h->used += total;
    return hipSuccess;
  });
  if (rc != HERRO_OK) return rc;
  h->alns.assign(in, in + n);
  h->scores.resize(n);
  h->n_ops.resize(n);
  for (uint32_t r = 0; r < n; r++) {
    h->alns[r].cigar = nullptr; h->alns[r].cigar_len = 0;
    fold_result(res[r], h->alns[r], h->scores[r], h->n_ops[r], h->failed);
  }
  *out = h.release();
  return HERRO_OK;
}

int herro_aligned_dev_from_ops(herro_ctx* ctx, uint32_t n, const herro_alignment* alns, const uint64_t* op_off, const uint32_t* ops, herro_aligned_dev** out) {
  if (!ctx || !out || !op_off || (n && !alns)) return HERRO_E_INVALID;
  *out = nullptr;
  for (uint32_t r = 0; r < n; r++)
    if (op_off[r + 1] < op_off[r] || op_off[r + 1] - op_off[r] > 0xffffffffull) {
      ctx->err = "herro_aligned_dev_from_ops: record " + std::to_string(r) + ": op_off must ascend";
      return HERRO_E_INVALID;
    }
  const uint64_t lo = op_off[0], total = op_off[n] - lo;
  if (total && !ops) return HERRO_E_INVALID;
  AlignedDevPtr h = new_aligned_dev(ctx);
  h->alns.assign(alns, alns + n);
  h->scores.assign(n, 0);
  h->n_ops.resize(n);
  h->op_off.resize(n);
  for (uint32_t r = 0; r < n; r++) {
    h->alns[r].cigar = nullptr; h->alns[r].cigar_len = 0;
    h->n_ops[r] = (uint32_t)(op_off[r + 1] - op_off[r]);
    h->op_off[r] = op_off[r] - lo;
    if (!h->n_ops[r]) { h->scores[r] = INT32_MIN; h->failed++; }
  }
  h->used = h->cap = total;
  if (ctx->host_only) {
    h->h_ops.assign(ops + lo, ops + lo + total);
  } else if (total) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMalloc((void**)&h->d_ops, total * 4));
    HIP_TRY(ctx, hipMemcpy(h->d_ops, ops + lo, total * 4, hipMemcpyHostToDevice));
  }
  *out = h.release();
  return HERRO_OK;
}

// ---- mirrored records (k_mirror in align_dev.hip): every record's alignment the other way round, without a second sweep ----------
// The new handle's store is src's ops (device to device) and behind them one reservation per mirror — the prefix sum of src's n_ops, since a mirror never
// has more ops than its source.  Records go through in slices of 2^20, one synchronisation per slice to fetch the results.
int herro_aligned_dev_mirror(herro_ctx* ctx, const herro_aligned_dev* src, herro_aligned_dev** out) {
  if (!ctx || !src || !out) return HERRO_E_INVALID;
  *out = nullptr;
  const char* const who = "herro_aligned_dev_mirror";
  if (src->ctx != ctx) { ctx->err = "herro_aligned_dev_mirror: the handle belongs to another context"; return HERRO_E_INVALID; }
  if (src->host_only) { ctx->err = "herro_aligned_dev_mirror: the context has no device"; return HERRO_E_NO_DEVICE; }
  if (src->alns.size() > 0x7fffffffull) { ctx->err = "herro_aligned_dev_mirror: more than 2^31 - 1 records"; return HERRO_E_INVALID; }
  const uint32_t n = (uint32_t)src->alns.size();
  if (const int rc = check_records(ctx, who, n, src->alns.data())) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  AlignedDevPtr h = new_aligned_dev(ctx);
  h->alns = src->alns; h->scores = src->scores; h->n_ops = src->n_ops; h->op_off = src->op_off;
  h->failed = src->failed;
  h->alns.resize(2 * (size_t)n); h->scores.resize(2 * (size_t)n, INT32_MIN); h->n_ops.resize(2 * (size_t)n, 0); h->op_off.resize(2 * (size_t)n, 0);
  uint64_t total = src->used;
  for (uint32_t r = 0; r < n; r++) {
    const herro_alignment& s = src->alns[r];
    herro_alignment& a = h->alns[n + r];
    a = herro_alignment{};
    a.qid = s.tid; a.qlen = s.tlen; a.qstart = s.tstart; a.qend = s.tend; a.strand = s.strand;
    a.tid = s.qid; a.tlen = s.qlen; a.tstart = s.qstart; a.tend = s.qend;
    h->op_off[n + r] = total;
    total += src->n_ops[r];
  }
  h->used = h->cap = total;
  const uint32_t cap = std::min(n, SLICE);
  std::vector<herro::MirrorIn> recs(cap);
  std::vector<herro::AlignOut> res(cap);
  herro::Bufs B;
  herro::MirrorIn* d_in = nullptr;
  herro::AlignOut* d_out = nullptr;
  if (total) FRONT_TRY(ctx, who, "op store", hipMalloc((void**)&h->d_ops, total * 4));
  if (src->used) FRONT_TRY(ctx, who, "op copy", hipMemcpyAsync(h->d_ops, src->d_ops, src->used * 4, hipMemcpyDeviceToDevice, ctx->stream));
  if (n) FRONT_TRY(ctx, who, "records", B.bytes(&d_in, sizeof(herro::MirrorIn) * cap));
  if (n) FRONT_TRY(ctx, who, "results", B.bytes(&d_out, sizeof(herro::AlignOut) * cap));
  for (uint32_t r0 = 0; r0 < n; r0 += SLICE) {
    const uint32_t cnt = std::min(SLICE, n - r0);
    for (uint32_t x = 0; x < cnt; x++) {
      const uint32_t r = r0 + x;
      const herro_alignment& s = src->alns[r];
      // the mirror's target is the source's query read, forward; its query the source's target read, reversed and complemented on strand 1
      recs[x] = herro::MirrorIn{ctx->h_word_off[s.qid], ctx->h_word_off[s.tid], src->op_off[r], h->op_off[n + r], s.qstart, s.qend - s.qstart,
                                s.tstart, s.tend - s.tstart, s.strand, src->n_ops[r], src->n_ops[r] ? src->scores[r] : 0, 0u};
    }
    FRONT_TRY(ctx, who, "record upload", hipMemcpyAsync(d_in, recs.data(), sizeof(herro::MirrorIn) * cnt, hipMemcpyHostToDevice, ctx->stream));
    herro::launch_mirror(ctx->d_words, d_in, d_out, h->d_ops, cnt, ctx->stream);
    FRONT_TRY(ctx, who, "k_mirror launch", hipGetLastError());
    FRONT_TRY(ctx, who, "results", hipMemcpyAsync(res.data(), d_out, sizeof(herro::AlignOut) * cnt, hipMemcpyDeviceToHost, ctx->stream));
    FRONT_TRY(ctx, who, "k_mirror", hipStreamSynchronize(ctx->stream));
    // (a failed mirror: n_ops 0, INT32_MIN and the swapped coordinates, untrimmed)
    for (uint32_t x = 0; x < cnt; x++) fold_result(res[x], h->alns[n + r0 + x], h->scores[n + r0 + x], h->n_ops[n + r0 + x], h->failed);
  }
  FRONT_TRY(ctx, who, "op copy", hipStreamSynchronize(ctx->stream));   // (n = 0 with ops in src's store: the copy has landed)
  *out = h.release();
  return HERRO_OK;
}

uint32_t herro_aligned_dev_n(const herro_aligned_dev* a) { return a ? (uint32_t)a->alns.size() : 0; }
const herro_alignment* herro_aligned_dev_alignments(const herro_aligned_dev* a) { return a ? a->alns.data() : nullptr; }
const int32_t* herro_aligned_dev_scores(const herro_aligned_dev* a) { return a ? a->scores.data() : nullptr; }
const uint32_t* herro_aligned_dev_n_ops(const herro_aligned_dev* a) { return a ? a->n_ops.data() : nullptr; }
uint32_t herro_aligned_dev_failed(const herro_aligned_dev* a) { return a ? a->failed : 0; }

void herro_aligned_dev_free(herro_aligned_dev* a) {
  if (!a) return;
  if (a->d_ops && hipSetDevice(a->device) == hipSuccess) (void)hipFree(a->d_ops);   // (hipFree waits for the device: no kernel is still reading the store)
  delete a;
}

int64_t herro_aligned_dev_cigar(const herro_aligned_dev* a, uint32_t r, char* out, uint64_t cap) {
  if (!a || r >= a->alns.size()) return HERRO_E_INVALID;
  std::vector<uint32_t> v;
  const int rc = aligned_dev_fetch(a, a->op_off[r], a->op_off[r] + a->n_ops[r], v);
  if (rc != HERRO_OK) return rc;
  const uint64_t need = ops_text_bytes(v.data(), (uint32_t)v.size());
  if (out && need <= cap) ops_text(v.data(), (uint32_t)v.size(), out);
  return (int64_t)need;
}

// ---- overlap finding (overlap_dev.hip) ---------------------------------------------------------------------------------------
// The seeding and chaining the reference leaves to `minimap2 -x ava-ont` (mm2.rs:15-30): the device returns the kept chains per
// (t, q, strand); the strand choice, the dual records and their grouping by target are a few lines of host code over them.
struct herro_overlaps {
  std::vector<uint32_t> rids;
  std::vector<uint64_t> aln_off;
  std::vector<herro_alignment> alns;
  std::vector<int32_t> scores;
  uint32_t occ_cut = 0;                  // the frequency cut the call used
  uint32_t rescued = 0;                  // minimizers the rescue kept (herro_set_seed_rescue; 0: off)
  uint32_t index_blocks = 0;             // read blocks of an index in parts (herro_set_index_params; 0: off)
};

int herro_find_overlaps(herro_ctx* ctx, const herro_overlap_params* params, herro_overlaps** out) { return herro_find_overlaps_core(ctx, params, nullptr, out); }

// core: the targets (overlaps.rs:154-159) — chains exist only for pairs with a core read, and a record only where its target is core
int herro_find_overlaps_core(herro_ctx* ctx, const herro_overlap_params* params, const uint8_t* core, herro_overlaps** out) {
  if (!ctx || !out) return HERRO_E_INVALID;
  *out = nullptr;
  herro::OvlParams P;
  if (int rc = overlap_params(ctx, params, P)) return rc;
  if (int rc = device_ready(ctx, "herro_find_overlaps")) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  std::vector<herro::OvlPair> chains;
  herro::OvlStats stats;
  std::string msg;
  herro::Bufs CB;
  uint8_t* d_core = nullptr;
  if (int rc = upload_core(ctx, "herro_find_overlaps", core, CB, &d_core)) return rc;
  if (int rc = overlap_rc(ctx, herro::ovl_find(ovl_store(ctx), P, d_core, scratch_budget("HERRO_OVL_SCRATCH_MB"), ctx->stream, chains, stats, msg), msg)) return rc;
  print_ovl_stats(P, stats);
  // one overlap per pair: chains arrive in ascending (t, q, rel), so the two strands of a pair are neighbours
  std::vector<herro::OvlPair> best;
  for (const herro::OvlPair& c : chains) {
    if (!best.empty() && best.back().t == c.t && best.back().q == c.q) {
      if (c.score > best.back().score) best.back() = c;
    } else {
      best.push_back(c);
    }
  }
  struct Rec { herro_alignment a; int32_t score; };
  std::vector<Rec> recs;
  recs.reserve(best.size() * 2);
  for (const herro::OvlPair& c : best) {
    const uint32_t tl = ctx->read_len[c.t], ql = ctx->read_len[c.q];
    if (!core || core[c.t]) recs.push_back(Rec{herro_alignment{c.q, ql, c.qstart, c.qend, c.rel, c.t, tl, c.tstart, c.tend, 0, nullptr}, c.score});
    if (!core || core[c.q]) recs.push_back(Rec{herro_alignment{c.t, tl, c.tstart, c.tend, c.rel, c.q, ql, c.qstart, c.qend, 0, nullptr}, c.score});   // the dual
  }
  std::sort(recs.begin(), recs.end(), [](const Rec& x, const Rec& y) { return x.a.tid != y.a.tid ? x.a.tid < y.a.tid : x.a.qid < y.a.qid; });
  auto* h = new herro_overlaps();
  h->occ_cut = (uint32_t)stats.occ_cut;
  h->rescued = (uint32_t)stats.rescued;
  h->index_blocks = P.index_kmers ? (uint32_t)stats.blocks : 0;
  h->alns.reserve(recs.size());
  h->scores.reserve(recs.size());
  for (const Rec& r : recs) {
    if (h->rids.empty() || h->rids.back() != r.a.tid) { h->rids.push_back(r.a.tid); h->aln_off.push_back(h->alns.size()); }
    h->alns.push_back(r.a);
    h->scores.push_back(r.score);
  }
  h->aln_off.push_back(h->alns.size());
  *out = h;
  return HERRO_OK;
}

uint32_t herro_overlaps_n(const herro_overlaps* o) { return o ? (uint32_t)o->alns.size() : 0; }
uint32_t herro_overlaps_n_targets(const herro_overlaps* o) { return o ? (uint32_t)o->rids.size() : 0; }
const uint32_t* herro_overlaps_target_ids(const herro_overlaps* o) { return o ? o->rids.data() : nullptr; }
const uint64_t* herro_overlaps_aln_off(const herro_overlaps* o) { return o ? o->aln_off.data() : nullptr; }
const herro_alignment* herro_overlaps_alignments(const herro_overlaps* o) { return o ? o->alns.data() : nullptr; }
const int32_t* herro_overlaps_scores(const herro_overlaps* o) { return o ? o->scores.data() : nullptr; }
uint32_t herro_overlaps_occ_cut(const herro_overlaps* o) { return o ? o->occ_cut : 0; }
uint32_t herro_overlaps_rescued(const herro_overlaps* o) { return o ? o->rescued : 0; }
uint32_t herro_overlaps_index_blocks(const herro_overlaps* o) { return o ? o->index_blocks : 0; }
void herro_overlaps_free(herro_overlaps* o) { delete o; }

// The rescue of high-frequency minimizers is a setting of the context (include/herro_amd.h): overlap_params hands it to every finder call.
int herro_set_seed_rescue(herro_ctx* ctx, const herro_seed_rescue_params* params) {
  if (!ctx) return HERRO_E_INVALID;
  const herro_seed_rescue_params off{};
  const herro_seed_rescue_params& p = params ? *params : off;
  if (p.occ_dist > (1u << 20) || p.rescue_max_occ > herro::OVL_OCC_BINS - 2 || p.reserved[0] || p.reserved[1]) {
    ctx->err = "herro_set_seed_rescue: occ_dist <= 2^20 (0: off), rescue_max_occ <= 65534 (0: 4095), reserved fields 0";
    return HERRO_E_INVALID;
  }
  ctx->seed_rescue = p;
  return HERRO_OK;
}

// The chain look-back is a setting of the context too: overlap_params hands it to every finder call and to herro_debug_chain.
int herro_set_chain_params(herro_ctx* ctx, const herro_chain_params* params) {
  if (!ctx) return HERRO_E_INVALID;
  const herro_chain_params dflt{};
  const herro_chain_params& p = params ? *params : dflt;
  const uint32_t h = p.lookback ? p.lookback : herro::OVL_LOOKBACK;
  if (h % 64 || h > herro::OVL_MAX_LOOKBACK || p.reserved[0] || p.reserved[1] || p.reserved[2]) {
    ctx->err = "herro_set_chain_params: lookback is a multiple of 64 in 64 .. 1024 (0: 64), reserved fields 0";
    return HERRO_E_INVALID;
  }
  ctx->chain_lookback = h;
  return HERRO_OK;
}

// The index in parts is a setting of the context too (include/herro_amd.h, "an index in parts"): overlap_params hands it to every finder call.
int herro_set_index_params(herro_ctx* ctx, const herro_index_params* params) {
  if (!ctx) return HERRO_E_INVALID;
  const herro_index_params off{};
  const herro_index_params& p = params ? *params : off;
  if (p.max_kmers > herro::OVL_MAX_KMERS || p.occ_ranges > herro::INDEX_MAX_RANGES || p.reserved) {
    ctx->err = "herro_set_index_params: max_kmers <= 2^32 - 4096 (0: off), occ_ranges <= 65536 (0: chosen by the library), reserved 0";
    return HERRO_E_INVALID;
  }
  ctx->index_parts = p;
  return HERRO_OK;
}

// The block rule alone (csrc/index_plan.h): host code, works on a context without a device.
int64_t herro_index_plan(herro_ctx* ctx, uint64_t n_reads, const uint32_t* read_len, uint32_t k, uint32_t w, uint64_t max_kmers, uint64_t* cuts, uint64_t cap) {
  if (!ctx) return HERRO_E_INVALID;
  if ((n_reads && !read_len) || k < 5 || k > 31 || w < 1 || w > 64 || max_kmers > herro::OVL_MAX_KMERS || n_reads > herro::OVL_MAX_READS) {
    ctx->err = "herro_index_plan: lengths for every read, 5 <= k <= 31, 1 <= w <= 64, max_kmers <= 2^32 - 4096, at most 2^31 - 1 reads";
    return HERRO_E_INVALID;
  }
  std::vector<uint64_t> c, kmers;
  herro::index_plan(n_reads, read_len, k, w, max_kmers, c, &kmers);
  uint64_t bi = 0, bj = 0;
  if (herro::index_plan_overflow(kmers, herro::OVL_MAX_KMERS, bi, bj)) {
    ctx->err = herro::index_plan_overflow_text(c, bi, bj);
    return HERRO_E_UNSUPPORTED;
  }
  if (cuts && c.size() <= cap) std::memcpy(cuts, c.data(), 8 * c.size());
  return (int64_t)c.size() - 1;
}

// ---- pair overlaps ("Pairs on the device"): reads -> one record per pair and the table of its two rows -> mirrored alignments ----
struct herro_pairs {
  herro_ctx* ctx = nullptr;
  std::vector<herro_alignment> alns;     // [P] primaries, ascending (tid, qid); cigar = NULL
  std::vector<int32_t> chain_scores;     // [P]
  std::vector<uint32_t> ext;             // [P][4]
  std::vector<int32_t> ext_scores;       // [P][2]
  std::vector<uint32_t> rids;            // targets of the 2 P rows
  std::vector<uint64_t> aln_off;         // [n_targets + 1]
  std::vector<uint32_t> rec_of_row;      // [n_rows]: 2 P, fewer with a core mask
  uint32_t occ_cut = 0;                  // the frequency cut the finder used; 0: a handle over the caller's table
  uint32_t rescued = 0;                  // minimizers the rescue kept; 0: off, or a handle over the caller's table
  uint32_t index_blocks = 0;             // read blocks of an index in parts; 0: off, or a handle over the caller's table
};

int herro_find_overlap_pairs(herro_ctx* ctx, const herro_overlap_params* params, const herro_extend_params* eparams, uint32_t flags, herro_pairs** out) {
  return herro_find_overlap_pairs_core(ctx, params, eparams, flags, nullptr, out);
}

// core: the pairs with a core read, the rows with a core target (include/herro_amd.h, "a core set of targets")
int herro_find_overlap_pairs_core(herro_ctx* ctx, const herro_overlap_params* params, const herro_extend_params* eparams, uint32_t flags, const uint8_t* core,
                                  herro_pairs** out) {
  if (!ctx || !out) return HERRO_E_INVALID;
  *out = nullptr;
  const char* const who = "herro_find_overlap_pairs";
  herro::OvlParams P;
  if (int rc = overlap_params(ctx, params, P)) return rc;
  const uint32_t zdrop = eparams && eparams->zdrop ? eparams->zdrop : herro::EXTEND_ZDROP;
  const uint32_t max_ext = eparams && eparams->max_ext ? eparams->max_ext : herro::EXTEND_MAX_EXT;
  if (max_ext > herro::EXTEND_MAX_EXT_LIMIT) { ctx->err = "herro_find_overlap_pairs: max_ext must be at most 2^20"; return HERRO_E_INVALID; }
  if (flags & ~HERRO_PAIRS_NO_EXTEND) { ctx->err = "herro_find_overlap_pairs: unknown flag"; return HERRO_E_INVALID; }
  if (int rc = device_ready(ctx, who)) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  herro::OvlRecs recs;
  herro::OvlStats stats;
  std::string msg;
  herro::Bufs CB;
  uint8_t* d_core = nullptr;
  if (int rc = upload_core(ctx, who, core, CB, &d_core)) return rc;
  if (int rc = overlap_rc(ctx, herro::ovl_find_pairs(ovl_store(ctx), P, d_core, scratch_budget("HERRO_OVL_SCRATCH_MB"), ctx->stream, recs, stats, msg), msg)) return rc;
  print_ovl_stats(P, stats);
  std::unique_ptr<herro_pairs> h(new herro_pairs());
  h->ctx = ctx;
  h->occ_cut = (uint32_t)stats.occ_cut;
  h->rescued = (uint32_t)stats.rescued;
  h->index_blocks = P.index_kmers ? (uint32_t)stats.blocks : 0;
  if (int rc = overlap_rc(ctx, herro::ovl_row_table(recs, ctx->n_reads, d_core, ctx->stream, h->rids, h->aln_off, h->rec_of_row, msg), msg)) return rc;
  const uint32_t n = (uint32_t)recs.n;   // (<= 2^31 - 1: ovl_find_pairs)
  h->ext.assign((size_t)n * 4, 0);
  h->ext_scores.assign((size_t)n * 2, 0);
  herro::Bufs B;
  if (n && !(flags & HERRO_PAIRS_NO_EXTEND)) {
    // the primaries are extended where they are: sides, k_extend and the fold in slices of 2^20 records, nothing in between comes down
    const uint32_t cap = std::min(n, SLICE);
    // one block: the sides and results of a slice (40 and 32 B per side), ext and scores of all records
    const uint64_t b_in = sizeof(herro::ExtIn) * 2ull * cap, b_out = sizeof(herro::ExtOut) * 2ull * cap;
    uint8_t* blk = nullptr;
    FRONT_TRY(ctx, who, "sides, results, ext, scores", B.bytes(&blk, b_in + b_out + 24ull * n));
    herro::ExtIn* const d_in = reinterpret_cast<herro::ExtIn*>(blk);
    herro::ExtOut* const d_out = reinterpret_cast<herro::ExtOut*>(blk + b_in);
    uint32_t* const d_ext = reinterpret_cast<uint32_t*>(blk + b_in + b_out);
    int32_t* const d_sc = reinterpret_cast<int32_t*>(blk + b_in + b_out + 16ull * n);
    for (uint32_t r0 = 0; r0 < n; r0 += SLICE) {
      const uint32_t cnt = std::min(SLICE, n - r0);
      herro::launch_ext_sides(recs.d + r0, cnt, ctx->d_word_off, ctx->d_qual_off, max_ext, d_in, ctx->stream);
      herro::launch_extend(ctx->d_words, d_in, d_out, zdrop, 2 * cnt, ctx->stream);
      herro::launch_ext_fold(recs.d + r0, cnt, d_out, d_ext + 4ull * r0, d_sc + 2ull * r0, ctx->stream);
      FRONT_TRY(ctx, who, "k_extend launch", hipGetLastError());
    }
    FRONT_TRY(ctx, who, "ext", hipMemcpyAsync(h->ext.data(), d_ext, 16ull * n, hipMemcpyDeviceToHost, ctx->stream));
    FRONT_TRY(ctx, who, "scores", hipMemcpyAsync(h->ext_scores.data(), d_sc, 8ull * n, hipMemcpyDeviceToHost, ctx->stream));
  }
  std::vector<herro::OvlRec> host(n);
  if (n) FRONT_TRY(ctx, who, "records", hipMemcpyAsync(host.data(), recs.d, sizeof(herro::OvlRec) * n, hipMemcpyDeviceToHost, ctx->stream));
  FRONT_TRY(ctx, who, "k_extend", hipStreamSynchronize(ctx->stream));
  h->alns.resize(n);
  h->chain_scores.resize(n);
  for (uint32_t p = 0; p < n; p++) {
    const herro::OvlRec& r = host[p];
    h->alns[p] = herro_alignment{r.qid, r.qlen, r.qstart, r.qend, r.strand, r.tid, r.tlen, r.tstart, r.tend, 0, nullptr};
    h->chain_scores[p] = r.score;
  }
  *out = h.release();
  return HERRO_OK;
}

namespace {
// herro_pairs_from_table (`strict`: exactly 2 P rows, every record in one) and herro_pairs_from_table_core (n_rows <= 2 P rows, no record in two)
int pairs_from_table(herro_ctx* ctx, const char* who, bool strict, uint32_t n_pairs, const herro_alignment* primaries, const int32_t* chain_scores,
                     uint32_t n_targets, const uint32_t* rids, const uint64_t* aln_off, uint64_t n_rows, const uint32_t* rec_of_row, herro_pairs** out) {
  if (!ctx || !out || !aln_off || (n_pairs && !primaries) || (n_rows && !rec_of_row) || (n_targets && !rids)) return HERRO_E_INVALID;
  *out = nullptr;
  if (n_pairs > herro::OVL_MAX_PAIRS) { ctx->err = std::string(who) + ": more than 2^31 - 1 pairs"; return HERRO_E_UNSUPPORTED; }
  if (const int rc = check_record_fields(ctx, who, n_pairs, primaries)) return rc;
  const uint64_t n_recs = 2ull * n_pairs;
  if (n_rows > n_recs) { ctx->err = std::string(who) + ": " + std::to_string(n_rows) + " rows for " + std::to_string(n_pairs) + " pairs: at most two rows per pair"; return HERRO_E_INVALID; }
  for (uint32_t t = 0; t <= n_targets; t++) {   // aln_off[0] = 0, aln_off[n_targets] = n_rows, ascending between
    const uint64_t lo = t == n_targets ? n_rows : (t ? aln_off[t - 1] : 0), hi = t ? n_rows : 0;
    if (aln_off[t] < lo || aln_off[t] > hi) {
      ctx->err = std::string(who) + ": aln_off[" + std::to_string(t) + "] = " + std::to_string(aln_off[t]) + ": aln_off must ascend from 0 to " + std::to_string(n_rows) +
                 (strict ? " (two rows per pair)" : " (the rows)");
      return HERRO_E_INVALID;
    }
  }
  std::vector<bool> seen(n_recs, false);
  for (uint64_t i = 0; i < n_rows; i++) {
    const uint32_t r = rec_of_row[i];
    if (r >= n_recs || seen[r]) {
      ctx->err = std::string(who) + ": rec_of_row[" + std::to_string(i) + "] = " + std::to_string(r) + (r >= n_recs ? " is outside the " + std::to_string(n_recs) + " records" : " occurs twice");
      return HERRO_E_INVALID;
    }
    seen[r] = true;
  }
  std::unique_ptr<herro_pairs> h(new herro_pairs());
  h->ctx = ctx;
  h->alns.assign(primaries, primaries + n_pairs);
  for (herro_alignment& a : h->alns) { a.cigar = nullptr; a.cigar_len = 0; }
  h->chain_scores.assign(n_pairs, 0);
  if (chain_scores) h->chain_scores.assign(chain_scores, chain_scores + n_pairs);
  h->ext.assign((size_t)n_pairs * 4, 0);
  h->ext_scores.assign((size_t)n_pairs * 2, 0);
  h->rids.assign(rids, rids + n_targets);
  h->aln_off.assign(aln_off, aln_off + n_targets + 1);
  h->rec_of_row.assign(rec_of_row, rec_of_row + n_rows);
  *out = h.release();
  return HERRO_OK;
}
}  // namespace

int herro_pairs_from_table(herro_ctx* ctx, uint32_t n_pairs, const herro_alignment* primaries, const int32_t* chain_scores, uint32_t n_targets,
                           const uint32_t* rids, const uint64_t* aln_off, const uint32_t* rec_of_row, herro_pairs** out) {
  return pairs_from_table(ctx, "herro_pairs_from_table", true, n_pairs, primaries, chain_scores, n_targets, rids, aln_off, 2ull * n_pairs, rec_of_row, out);
}

int herro_pairs_from_table_core(herro_ctx* ctx, uint32_t n_pairs, const herro_alignment* primaries, const int32_t* chain_scores, uint32_t n_targets,
                                const uint32_t* rids, const uint64_t* aln_off, uint64_t n_rows, const uint32_t* rec_of_row, herro_pairs** out) {
  return pairs_from_table(ctx, "herro_pairs_from_table_core", false, n_pairs, primaries, chain_scores, n_targets, rids, aln_off, n_rows, rec_of_row, out);
}

int herro_pairs_align(herro_ctx* ctx, const herro_pairs* p, herro_aligned_dev** out) {
  if (!ctx || !p || !out) return HERRO_E_INVALID;
  *out = nullptr;
  if (p->ctx != ctx) { ctx->err = "herro_pairs_align: the handle belongs to another context"; return HERRO_E_INVALID; }
  herro_aligned_dev* prim = nullptr;
  if (const int rc = herro_align_overlaps_dev(ctx, (uint32_t)p->alns.size(), p->alns.data(), &prim)) return rc;
  const int rc = herro_aligned_dev_mirror(ctx, prim, out);
  herro_aligned_dev_free(prim);
  return rc;
}

herro_job* herro_job_create_paired(herro_ctx* ctx, const herro_pairs* p, const herro_aligned_dev* m, uint32_t window_size) {
  if (!ctx) return nullptr;
  auto fail = [&](const std::string& why) -> herro_job* {
    ctx->err = "herro_job_create_paired: " + why + " [code " + std::to_string(HERRO_E_INVALID) + "]";
    ctx->create_code = HERRO_E_INVALID;
    return nullptr;
  };
  if (!p || !m) return fail("null handle");
  if (p->ctx != ctx || m->ctx != ctx) return fail("the handle belongs to another context");
  if (m->alns.size() != 2 * p->alns.size())   // (not the row count: a table of core targets has fewer rows than records)
    return fail("the aligned handle has " + std::to_string(m->alns.size()) + " records, the pairs need " + std::to_string(2 * p->alns.size()) + " (primaries, then mirrors)");
  // api.paired_job_args: a row whose record failed is dropped, the rest regrouped over the targets, which keep their place
  const uint32_t nt = (uint32_t)p->rids.size();
  std::vector<uint64_t> off(nt + 1ull, 0);
  std::vector<uint32_t> rec;
  rec.reserve(p->rec_of_row.size());
  for (uint32_t t = 0; t < nt; t++) {
    for (uint64_t i = p->aln_off[t]; i < p->aln_off[t + 1]; i++)
      if (m->n_ops[p->rec_of_row[i]]) rec.push_back(p->rec_of_row[i]);
    off[t + 1] = rec.size();
  }
  return herro_job_create_aligned(ctx, nt, p->rids.data(), off.data(), rec.data(), m, window_size);
}

uint32_t herro_pairs_n(const herro_pairs* p) { return p ? (uint32_t)p->alns.size() : 0; }
const herro_alignment* herro_pairs_primaries(const herro_pairs* p) { return p ? p->alns.data() : nullptr; }
const int32_t* herro_pairs_chain_scores(const herro_pairs* p) { return p ? p->chain_scores.data() : nullptr; }
const uint32_t* herro_pairs_ext(const herro_pairs* p) { return p ? p->ext.data() : nullptr; }
const int32_t* herro_pairs_ext_scores(const herro_pairs* p) { return p ? p->ext_scores.data() : nullptr; }
uint32_t herro_pairs_n_targets(const herro_pairs* p) { return p ? (uint32_t)p->rids.size() : 0; }
const uint32_t* herro_pairs_target_ids(const herro_pairs* p) { return p ? p->rids.data() : nullptr; }
const uint64_t* herro_pairs_aln_off(const herro_pairs* p) { return p ? p->aln_off.data() : nullptr; }
const uint32_t* herro_pairs_rec_of_row(const herro_pairs* p) { return p ? p->rec_of_row.data() : nullptr; }
uint64_t herro_pairs_n_rows(const herro_pairs* p) { return p ? p->rec_of_row.size() : 0; }
uint32_t herro_pairs_occ_cut(const herro_pairs* p) { return p ? p->occ_cut : 0; }
uint32_t herro_pairs_rescued(const herro_pairs* p) { return p ? p->rescued : 0; }
uint32_t herro_pairs_index_blocks(const herro_pairs* p) { return p ? p->index_blocks : 0; }
void herro_pairs_free(herro_pairs* p) { delete p; }

// ---- PAF / .oec.zst of found alignments (paf_dev.hip) ----------------------------------------------------------------------------
// What `herro inference --write-alns` keeps of a batch (AlnMode::Write: overlaps.rs:248-286, the lines themselves 349-352): one PAF line with `cg:Z:` per
// alignment.  Line format: paf_dev.h.  Columns 10 and 11 are the summed M lengths and the summed op lengths, not minimap2's residue matches and block
// length; the reference reads neither (overlaps.rs:135-172).  A device handle's lines are formed by k_paf_len / k_paf_write in chunks of text that
// fit HERRO_PAF_SCRATCH_MB and come down through two pinned buffers; a device-free handle's by paf_line_host below, which is the specification.
struct herro_paf_text {
  std::string text;
  uint64_t lines = 0;
};

namespace {
struct PafStats { uint64_t rows = 0, lines = 0, bytes = 0, chunks = 0; };
using PafSink = std::function<int(const char*, uint64_t)>;   // whole lines, in order; HERRO_OK, or the code whose message it left in ctx->err
constexpr uint64_t PAF_BUDGET_CHUNKS = 16;                   // a chunk's text is this fraction of the budget (64 MiB at the default): the two pinned halves stay small, and a text as large as the budget still overlaps its copies with the next chunk's kernels
constexpr uint64_t PAF_HOST_ROWS = 16384;                    // rows of a turn of the host formatter

int paf_invalid(herro_ctx* ctx, const char* who, const std::string& why) {
  ctx->err = std::string(who) + ": " + why;
  return HERRO_E_INVALID;
}

// a name is a PAF field: not empty, no tab, no newline
int check_names(herro_ctx* ctx, const char* who, const char* names, const uint64_t* name_off) {
  for (uint32_t r = 0; r < ctx->n_reads; r++) {
    const uint64_t b = name_off[r], e = name_off[r + 1];
    if (e <= b) return paf_invalid(ctx, who, "read " + std::to_string(r) + ": empty name");
    if (memchr(names + b, '\t', e - b) || memchr(names + b, '\n', e - b))
      return paf_invalid(ctx, who, "read " + std::to_string(r) + ": a name must not contain a tab or a newline");
  }
  return HERRO_OK;
}

// The specification of a line: row `a` with its ops, appended to out.
void paf_line_host(const herro_alignment& a, const uint32_t* ops, uint32_t n_ops, const char* names, const uint64_t* name_off, std::string& out) {
  if (!n_ops) return;
  uint64_t mbases = 0, blocklen = 0;
  for (uint32_t x = 0; x < n_ops; x++) {
    blocklen += ops[x] >> 2;
    if ((ops[x] & 3u) == 0) mbases += ops[x] >> 2;
  }
  char buf[160];
  out.append(names + name_off[a.qid], name_off[a.qid + 1] - name_off[a.qid]);
  out.append(buf, snprintf(buf, sizeof buf, "\t%u\t%u\t%u\t%c\t", a.qlen, a.qstart, a.qend, a.strand ? '-' : '+'));
  out.append(names + name_off[a.tid], name_off[a.tid + 1] - name_off[a.tid]);
  out.append(buf, snprintf(buf, sizeof buf, "\t%u\t%u\t%u\t%llu\t%llu\t255\tcg:Z:", a.tlen, a.tstart, a.tend, (unsigned long long)mbases, (unsigned long long)blocklen));
  const size_t at = out.size();
  out.resize(at + ops_text_bytes(ops, n_ops) + 1);   // (+ 1: snprintf's terminator of the last op lands where the newline goes)
  ops_text(ops, n_ops, &out[at]);
  out.back() = '\n';
}

int paf_emit_host(herro_ctx* ctx, const herro_aligned_dev* a, const std::vector<uint32_t>& recs, const char* names, const uint64_t* name_off, const PafSink& sink,
                  PafStats& st) {
  std::vector<std::string> part;
  std::string turn;
  for (uint64_t r0 = 0; r0 < recs.size(); r0 += PAF_HOST_ROWS) {
    const uint64_t r1 = std::min<uint64_t>(recs.size(), r0 + PAF_HOST_ROWS);
    part.assign((r1 - r0 + 63) / 64, std::string());
    host_pool(ctx).run((uint32_t)part.size(), [&](uint32_t b) {
      for (uint64_t i = r0 + (uint64_t)b * 64; i < std::min(r1, r0 + (uint64_t)(b + 1) * 64); i++)
        paf_line_host(a->alns[recs[i]], a->h_ops.data() + a->op_off[recs[i]], a->n_ops[recs[i]], names, name_off, part[b]);
    });
    turn.clear();
    for (const std::string& s : part) turn += s;
    for (uint64_t i = r0; i < r1; i++) st.lines += a->n_ops[recs[i]] != 0;
    if (turn.empty()) continue;
    st.bytes += turn.size(); st.chunks++;
    if (const int rc = sink(turn.data(), turn.size())) return rc;
  }
  return HERRO_OK;
}

// the pinned halves and events of paf_emit_dev: nothing of the stream is in flight when they go
struct PafStage {
  hipStream_t st = nullptr;
  char* pin[2] = {nullptr, nullptr};
  hipEvent_t ev[2] = {nullptr, nullptr};
  ~PafStage() {
    (void)hipStreamSynchronize(st);
    for (int b = 0; b < 2; b++) {
      if (pin[b]) (void)hipHostFree(pin[b]);
      if (ev[b]) (void)hipEventDestroy(ev[b]);
    }
  }
};

int paf_emit_dev(herro_ctx* ctx, const char* who, const herro_aligned_dev* a, const std::vector<uint32_t>& recs, const char* names, const uint64_t* name_off,
                 const PafSink& sink, PafStats& st) {
  const uint32_t n = (uint32_t)recs.size();   // (<= PAF_MAX_ROWS: paf_emit)
  if (!n) return HERRO_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  std::vector<herro::PafRow> rows(n);
  for (uint32_t i = 0; i < n; i++) {
    const herro_alignment& x = a->alns[recs[i]];
    rows[i] = herro::PafRow{a->op_off[recs[i]], a->n_ops[recs[i]], x.qid, x.qlen, x.qstart, x.qend, x.strand, x.tid, x.tlen, x.tstart, x.tend};
  }
  std::vector<uint64_t> noff(ctx->n_reads + 1ull);   // the names from their first byte
  for (uint32_t r = 0; r <= ctx->n_reads; r++) noff[r] = name_off[r] - name_off[0];
  herro::Bufs B;
  PafStage S;
  S.st = ctx->stream;
  herro::PafRow* d_rows = nullptr;
  herro::PafSums* d_sums = nullptr;
  uint32_t* d_len = nullptr;
  uint64_t* d_noff = nullptr;
  char* d_names = nullptr;
  FRONT_TRY(ctx, who, "rows", B.bytes(&d_rows, sizeof(herro::PafRow) * (uint64_t)n));
  FRONT_TRY(ctx, who, "sums", B.bytes(&d_sums, sizeof(herro::PafSums) * (uint64_t)n));
  FRONT_TRY(ctx, who, "line bytes", B.bytes(&d_len, 4ull * n));
  FRONT_TRY(ctx, who, "name offsets", B.bytes(&d_noff, 8ull * noff.size()));
  FRONT_TRY(ctx, who, "names", B.bytes(&d_names, std::max<uint64_t>(noff.back(), 1)));
  FRONT_TRY(ctx, who, "row upload", hipMemcpyAsync(d_rows, rows.data(), sizeof(herro::PafRow) * (uint64_t)n, hipMemcpyHostToDevice, ctx->stream));
  FRONT_TRY(ctx, who, "name offset upload", hipMemcpyAsync(d_noff, noff.data(), 8ull * noff.size(), hipMemcpyHostToDevice, ctx->stream));
  if (noff.back()) FRONT_TRY(ctx, who, "name upload", hipMemcpyAsync(d_names, names + name_off[0], noff.back(), hipMemcpyHostToDevice, ctx->stream));
  herro::launch_paf_len(d_rows, a->d_ops, d_noff, n, d_len, d_sums, ctx->stream);
  FRONT_TRY(ctx, who, "k_paf_len launch", hipGetLastError());
  std::vector<uint32_t> len(n);
  FRONT_TRY(ctx, who, "line bytes", hipMemcpyAsync(len.data(), d_len, 4ull * n, hipMemcpyDeviceToHost, ctx->stream));
  FRONT_TRY(ctx, who, "k_paf_len", hipStreamSynchronize(ctx->stream));
  // chunks: consecutive rows whose text fits a sixteenth of the budget (two such buffers are resident); a longer line runs alone
  // ... and no chunk reaches 2^32 bytes whatever the budget: its line offsets are a 32-bit scan (a line alone is at most PAF_MAX_CHUNK, checked below)
  const uint64_t cap = std::min<uint64_t>(std::max<uint64_t>(scratch_budget("HERRO_PAF_SCRATCH_MB", 1024) / PAF_BUDGET_CHUNKS, 1), herro::PAF_MAX_CHUNK);
  std::vector<uint32_t> cut{0};
  std::vector<uint64_t> cbytes;
  uint64_t acc = 0, max_bytes = 0;
  uint32_t max_rows = 0;
  for (uint32_t i = 0; i < n; i++) {
    if (len[i] > herro::PAF_MAX_CHUNK) {
      ctx->err = std::string(who) + ": row " + std::to_string(i) + ": a line of 2^32 bytes or more";
      return HERRO_E_UNSUPPORTED;
    }
    if (acc && acc + len[i] > cap) { cut.push_back(i); cbytes.push_back(acc); acc = 0; }
    acc += len[i];
    st.lines += len[i] != 0;
  }
  cut.push_back(n); cbytes.push_back(acc);
  for (size_t c = 0; c < cbytes.size(); c++) {
    max_bytes = std::max(max_bytes, cbytes[c]);
    max_rows = std::max(max_rows, cut[c + 1] - cut[c]);
  }
  if (!max_bytes) return HERRO_OK;   // every row failed
  char* d_text[2] = {nullptr, nullptr};
  uint32_t *d_off[2] = {nullptr, nullptr}, *d_part[2] = {nullptr, nullptr};
  const int halves = cbytes.size() > 1 ? 2 : 1;
  for (int b = 0; b < halves; b++) {
    FRONT_TRY(ctx, who, "text", B.bytes(&d_text[b], max_bytes));
    FRONT_TRY(ctx, who, "line offsets", B.bytes(&d_off[b], 4ull * (max_rows + 1ull)));
    FRONT_TRY(ctx, who, "scan scratch", B.bytes(&d_part[b], 4ull * herro::dev_scan_partials(max_rows) + 64));
    FRONT_TRY(ctx, who, "pinned text", hipHostMalloc((void**)&S.pin[b], max_bytes, hipHostMallocDefault));
    FRONT_TRY(ctx, who, "event", hipEventCreateWithFlags(&S.ev[b], hipEventDisableTiming));
  }
  std::string msg;
  // chunk c: offsets, text, the copy into pinned half c & 1 and the event behind it.  The stream orders a half's reuse on the device; the host has
  // consumed the pinned half of chunk c - 2 before chunk c is queued.
  auto queue = [&](size_t c) -> int {
    if (!cbytes[c]) return HERRO_OK;
    const int b = (int)(c & 1);
    const uint32_t r0 = cut[c], cnt = cut[c + 1] - cut[c];
    if (herro::dev_scan_u32(d_len + r0, cnt, d_off[b], d_part[b], ctx->stream, msg) != herro::OVL_OK) { ctx->err = std::string(who) + ": " + msg; return HERRO_E_NO_DEVICE; }
    herro::launch_paf_write(d_rows + r0, a->d_ops, d_names, d_noff, d_off[b], d_sums + r0, cnt, d_text[b], cbytes[c], ctx->stream);
    FRONT_TRY(ctx, who, "k_paf_write launch", hipGetLastError());
    FRONT_TRY(ctx, who, "text copy", hipMemcpyAsync(S.pin[b], d_text[b], cbytes[c], hipMemcpyDeviceToHost, ctx->stream));
    FRONT_TRY(ctx, who, "event", hipEventRecord(S.ev[b], ctx->stream));
    return HERRO_OK;
  };
  if (const int rc = queue(0)) return rc;
  for (size_t c = 0; c < cbytes.size(); c++) {
    if (c + 1 < cbytes.size())
      if (const int rc = queue(c + 1)) return rc;
    if (!cbytes[c]) continue;
    FRONT_TRY(ctx, who, "k_paf_write", hipEventSynchronize(S.ev[c & 1]));
    st.bytes += cbytes[c]; st.chunks++;
    if (const int rc = sink(S.pin[c & 1], cbytes[c])) return rc;
  }
  return HERRO_OK;
}

// Checks in the order of include/herro_amd.h, then the lines of rows rec[0 .. n_rows) (NULL: row i is record i) to the sink, chunk by chunk.
int paf_emit(herro_ctx* ctx, const char* who, const herro_aligned_dev* a, uint64_t n_rows, const uint32_t* rec, const char* names, const uint64_t* name_off,
             const PafSink& sink, PafStats& st) {
  if (a->ctx != ctx) return paf_invalid(ctx, who, "the handle belongs to another context");
  if (!ctx->n_reads || (!ctx->host_only && !ctx->d_words)) { ctx->err = "herro_set_reads must be called first"; return HERRO_E_STATE; }   // (device-free: made over no read)
  if (n_rows > herro::PAF_MAX_ROWS) { ctx->err = std::string(who) + ": more than 2^31 - 1 rows"; return HERRO_E_UNSUPPORTED; }
  std::vector<uint32_t> recs(n_rows);
  for (uint64_t i = 0; i < n_rows; i++) {
    const uint64_t r = rec ? rec[i] : i;
    if (r >= a->alns.size()) return paf_invalid(ctx, who, "rec[" + std::to_string(i) + "] = " + std::to_string(r) + " is outside the " + std::to_string(a->alns.size()) + " records");
    if (a->alns[r].qid >= ctx->n_reads || a->alns[r].tid >= ctx->n_reads)
      return paf_invalid(ctx, who, "row " + std::to_string(i) + " (record " + std::to_string(r) + "): read id outside the read store");
    recs[i] = (uint32_t)r;
  }
  st.rows = n_rows;
  const int rc = a->host_only ? paf_emit_host(ctx, a, recs, names, name_off, sink, st) : paf_emit_dev(ctx, who, a, recs, names, name_off, sink, st);
  if (rc != HERRO_OK) return rc;
  const char* e = getenv("HERRO_PAF_STATS");   // (tools/pafwriterate.py, the budget test): one line on stderr
  if (e && atoi(e))
    fprintf(stderr, "PAF rows=%llu lines=%llu bytes=%llu chunks=%llu\n", (unsigned long long)st.rows, (unsigned long long)st.lines, (unsigned long long)st.bytes,
            (unsigned long long)st.chunks);
  return HERRO_OK;
}

// what the pair entries ask before anything runs: the names, then the two handles
int check_pairs_paf(herro_ctx* ctx, const char* who, const herro_pairs* p, const herro_aligned_dev* m, const char* names, const uint64_t* name_off) {
  if (const int rc = check_names(ctx, who, names, name_off)) return rc;
  if (p->ctx != ctx || m->ctx != ctx) return paf_invalid(ctx, who, "the handle belongs to another context");
  if (m->alns.size() != 2 * p->alns.size())
    return paf_invalid(ctx, who, "the aligned handle has " + std::to_string(m->alns.size()) + " records, the pairs need " + std::to_string(2 * p->alns.size()) + " (primaries, then mirrors)");
  return HERRO_OK;
}

int paf_to_text(herro_ctx* ctx, const char* who, const herro_aligned_dev* a, uint64_t n_rows, const uint32_t* rec, const char* names, const uint64_t* name_off,
                herro_paf_text** out) {
  std::unique_ptr<herro_paf_text> h(new herro_paf_text());
  PafStats st;
  const int rc = paf_emit(ctx, who, a, n_rows, rec, names, name_off, [&](const char* p, uint64_t n) { h->text.append(p, n); return HERRO_OK; }, st);
  if (rc != HERRO_OK) return rc;
  h->lines = st.lines;
  *out = h.release();
  return HERRO_OK;
}
}  // namespace

int herro_aligned_dev_paf(herro_ctx* ctx, const herro_aligned_dev* a, uint64_t n_rows, const uint32_t* rec, const char* names, const uint64_t* name_off,
                          herro_paf_text** out) {
  if (!ctx || !a || !out || !name_off || (ctx->n_reads && !names)) return HERRO_E_INVALID;
  *out = nullptr;
  const char* const who = "herro_aligned_dev_paf";
  if (const int rc = check_names(ctx, who, names, name_off)) return rc;
  return paf_to_text(ctx, who, a, n_rows, rec, names, name_off, out);
}

int herro_pairs_paf(herro_ctx* ctx, const herro_pairs* p, const herro_aligned_dev* m, const char* names, const uint64_t* name_off, herro_paf_text** out) {
  if (!ctx || !p || !m || !out || !name_off || (ctx->n_reads && !names)) return HERRO_E_INVALID;
  *out = nullptr;
  const char* const who = "herro_pairs_paf";
  if (const int rc = check_pairs_paf(ctx, who, p, m, names, name_off)) return rc;
  return paf_to_text(ctx, who, m, p->rec_of_row.size(), p->rec_of_row.data(), names, name_off, out);
}

const char* herro_paf_text_data(const herro_paf_text* t) { return t ? t->text.data() : nullptr; }
uint64_t herro_paf_text_len(const herro_paf_text* t) { return t ? t->text.size() : 0; }
uint64_t herro_paf_text_lines(const herro_paf_text* t) { return t ? t->lines : 0; }
void herro_paf_text_free(herro_paf_text* t) { delete t; }

// The batch file of AlnMode::Write (overlaps.rs:270-282): "<n_targets>\n", the targets' names, the lines — one zstd frame (HERRO_ALNS_OEC), or the lines alone.
int herro_pairs_write_alns(herro_ctx* ctx, const herro_pairs* p, const herro_aligned_dev* m, const char* names, const uint64_t* name_off, const char* path,
                           uint32_t flags, uint64_t* lines, uint64_t* bytes) {
  if (!ctx || !p || !m || !path || !name_off || (ctx->n_reads && !names)) return HERRO_E_INVALID;
  const char* const who = "herro_pairs_write_alns";
  if (const int rc = check_pairs_paf(ctx, who, p, m, names, name_off)) return rc;
  if (flags & ~HERRO_ALNS_OEC) return paf_invalid(ctx, who, "unknown flag");
  for (size_t t = 0; t < p->rids.size(); t++)
    if (p->rids[t] >= ctx->n_reads) return paf_invalid(ctx, who, "target " + std::to_string(t) + ": read id outside the read store");
  AlnsFile f;   // (leaves no file unless committed)
  std::string why;
  bool unsupported = false;
  auto file_failed = [&]() { ctx->err = std::string(who) + ": " + why; return unsupported ? HERRO_E_UNSUPPORTED : HERRO_E_INVALID; };
  if (!f.open(path, (flags & HERRO_ALNS_OEC) != 0, why, unsupported)) return file_failed();
  if (flags & HERRO_ALNS_OEC) {
    std::string head = std::to_string(p->rids.size()) + "\n";
    for (const uint32_t t : p->rids) { head.append(names + name_off[t], name_off[t + 1] - name_off[t]); head += '\n'; }
    if (!f.write(head.data(), head.size(), why)) return file_failed();
  }
  PafStats st;
  const int rc = paf_emit(ctx, who, m, p->rec_of_row.size(), p->rec_of_row.data(), names, name_off,
                          [&](const char* q, uint64_t n) { return f.write(q, n, why) ? HERRO_OK : file_failed(); }, st);
  if (rc != HERRO_OK) return rc;
  if (!f.commit(why)) return file_failed();
  const char* e = getenv("HERRO_PAF_STATS");
  if (e && atoi(e)) fprintf(stderr, "PAFFILE file_bytes=%llu zstd_s=%.6f\n", (unsigned long long)f.file_bytes, f.zstd_seconds);
  if (lines) *lines = st.lines;
  if (bytes) *bytes = f.file_bytes;
  return HERRO_OK;
}

int64_t herro_debug_sketch(herro_ctx* ctx, const herro_overlap_params* params, uint64_t* hash, uint32_t* rid, uint32_t* pos,
                           uint8_t* strand, uint64_t cap) {
  if (!ctx) return HERRO_E_INVALID;
  herro::OvlParams P;
  if (int rc = overlap_params(ctx, params, P)) return rc;
  if (int rc = device_ready(ctx, "herro_debug_sketch")) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  std::vector<uint64_t> h, m;
  std::string msg;
  if (int rc = overlap_rc(ctx, herro::ovl_sketch(ovl_store(ctx), P, ctx->stream, h, m, msg), msg)) return rc;
  if (h.size() <= cap && hash && rid && pos && strand) {
    for (size_t i = 0; i < h.size(); i++) {
      hash[i] = h[i];
      rid[i] = (uint32_t)(m[i] >> 32);
      pos[i] = ((uint32_t)m[i]) >> 1;
      strand[i] = (uint8_t)(m[i] & 1u);
    }
  }
  return (int64_t)h.size();
}

int64_t herro_debug_seed_rescue(herro_ctx* ctx, const herro_overlap_params* params, uint32_t* occ, uint8_t* rescued, uint64_t cap) {
  if (!ctx) return HERRO_E_INVALID;
  herro::OvlParams P;
  if (int rc = overlap_params(ctx, params, P)) return rc;
  if (int rc = device_ready(ctx, "herro_debug_seed_rescue")) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  std::vector<uint32_t> c;
  std::vector<uint8_t> f;
  std::string msg;
  if (int rc = overlap_rc(ctx, herro::ovl_seed_rescue(ovl_store(ctx), P, ctx->stream, c, f, msg), msg)) return rc;
  if (c.size() <= cap && occ && rescued && !c.empty()) {
    std::memcpy(occ, c.data(), 4 * c.size());
    std::memcpy(rescued, f.data(), f.size());
  }
  return (int64_t)c.size();
}

int herro_debug_occ_census(herro_ctx* ctx, const herro_overlap_params* params, uint32_t* hist, uint64_t out[4]) {
  if (!ctx || !out) return HERRO_E_INVALID;
  herro::OvlParams P;
  if (int rc = overlap_params(ctx, params, P)) return rc;
  if (!P.occ_frac_ppm) { ctx->err = "herro_debug_occ_census: occ_frac_ppm is 0 (the fixed cut takes no census)"; return HERRO_E_INVALID; }
  if (int rc = device_ready(ctx, "herro_debug_occ_census")) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  std::vector<uint32_t> h;
  std::string msg;
  if (int rc = overlap_rc(ctx, herro::ovl_occ_census(ovl_store(ctx), P, ctx->stream, hist ? &h : nullptr, out, msg), msg)) return rc;
  if (hist) std::memcpy(hist, h.data(), 4ull * herro::OVL_OCC_BINS);
  return HERRO_OK;
}

// ---- adapters in the resident reads (adapter_dev.hip) --------------------------------------------------------------
// The host's share: the pattern table (both strands, their bit planes), the segment length, and the order of the hits — the kernels append
// them in no order, the specification's key (rid, end, start, adapter, strand) is unique per hit, and sorting by it gives the bytes.
struct herro_adapter_hits {
  std::vector<herro_adapter_hit> hits;
  std::vector<uint64_t> off;             // [n_reads + 1]
};

int herro_find_adapters(herro_ctx* ctx, uint32_t n_adapters, const char* seq, const uint64_t* off, const herro_adapter_params* params,
                        herro_adapter_hits** out) {
  if (!ctx || !out) return HERRO_E_INVALID;
  *out = nullptr;
  const char* const who = "herro_find_adapters";
  const herro_adapter_params z{};
  const herro_adapter_params& p = params ? *params : z;
  const uint32_t pm = p.max_err_pm ? p.max_err_pm : 250;
  if (pm > 500 || (p.flags & ~HERRO_ADAPTERS_FORWARD_ONLY) || p.reserved[0] || p.reserved[1]) {
    ctx->err = std::string(who) + ": max_err_pm <= 500 (0: 250), flags HERRO_ADAPTERS_FORWARD_ONLY or 0, reserved fields 0";
    return HERRO_E_INVALID;
  }
  if (n_adapters < 1 || n_adapters > 32 || !seq || !off) { ctx->err = std::string(who) + ": 1 <= n_adapters <= 32, seq and off not NULL"; return HERRO_E_INVALID; }
  std::vector<herro::AdaptPattern> pats(2 * (size_t)n_adapters, herro::AdaptPattern{});
  for (uint32_t a = 0; a < n_adapters; a++) {
    if (off[a + 1] < off[a] || off[a + 1] - off[a] < 8 || off[a + 1] - off[a] > 64) {
      ctx->err = std::string(who) + ": adapter " + std::to_string(a) + ": 8 <= length <= 64";
      return HERRO_E_INVALID;
    }
    const uint32_t m = (uint32_t)(off[a + 1] - off[a]);
    uint8_t code[64];
    for (uint32_t i = 0; i < m; i++) {
      switch (seq[off[a] + i]) {
        case 'A': case 'a': code[i] = 0; break;
        case 'C': case 'c': code[i] = 1; break;
        case 'G': case 'g': code[i] = 2; break;
        case 'T': case 't': code[i] = 3; break;
        default:
          ctx->err = std::string(who) + ": adapter " + std::to_string(a) + ": base " + std::to_string(i) + " is not A, C, G or T";
          return HERRO_E_INVALID;
      }
    }
    for (uint32_t s = 0; s < ((p.flags & HERRO_ADAPTERS_FORWARD_ONLY) ? 1u : 2u); s++) {
      uint64_t f0 = 0, f1 = 0, b0 = 0, b1 = 0;   // the planes of the pattern and of the pattern reversed
      for (uint32_t i = 0; i < m; i++) {
        const uint64_t c = s ? 3u - code[m - 1 - i] : code[i];   // strand 1: the reverse complement
        f0 |= (c & 1u) << i;           f1 |= (c >> 1) << i;
        b0 |= (c & 1u) << (m - 1 - i); b1 |= (c >> 1) << (m - 1 - i);
      }
      pats[2 * a + s] = herro::AdaptPattern{~f0, ~f1, ~b0, ~b1, m, (uint32_t)((uint64_t)m * pm / 1000), (uint16_t)a, (uint8_t)s, 0, 0};
    }
  }
  if (int rc = device_ready(ctx, who)) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  uint32_t seg = herro::ADAPT_SEG_DEFAULT;
  if (const char* e = getenv("HERRO_ADAPT_SEG")) seg = (uint32_t)std::min<long long>(std::max<long long>(atoll(e), herro::ADAPT_SEG_MIN), herro::ADAPT_SEG_MAX);
  std::unique_ptr<herro_adapter_hits> h(new herro_adapter_hits());
  herro::AdaptStats stats;
  std::string msg;
  const herro::AdaptStore S{ctx->d_p0, ctx->d_p1, ctx->d_word_off, ctx->d_qual_off, ctx->read_len.data(), ctx->n_reads};
  const int rc = herro::adapt_find(S, pats, seg, ctx->debug_adapter_cap, ctx->stream, h->hits, stats, msg);
  if (rc != herro::ADAPT_OK) { ctx->err = msg; return rc == herro::ADAPT_UNSUPPORTED ? HERRO_E_UNSUPPORTED : HERRO_E_NO_DEVICE; }
  const auto t0 = std::chrono::steady_clock::now();
  // by read first (a counting sort: the offsets are the result's anyway), then every read's hits by the rest of the key on the pool
  h->off.assign((size_t)ctx->n_reads + 1, 0);
  for (const herro_adapter_hit& x : h->hits) h->off[x.rid + 1]++;
  for (uint32_t r = 0; r < ctx->n_reads; r++) h->off[r + 1] += h->off[r];
  {
    std::vector<herro_adapter_hit> by_read(h->hits.size());
    std::vector<uint64_t> at(h->off.begin(), h->off.end() - 1);
    for (const herro_adapter_hit& x : h->hits) by_read[at[x.rid]++] = x;
    h->hits.swap(by_read);
  }
  constexpr uint32_t READS_PER_TASK = 1024;
  host_pool(ctx).run((ctx->n_reads + READS_PER_TASK - 1) / READS_PER_TASK, [&](uint32_t b) {
    const uint32_t r1 = (uint32_t)std::min<uint64_t>((uint64_t)(b + 1) * READS_PER_TASK, ctx->n_reads);
    for (uint32_t r = b * READS_PER_TASK; r < r1; r++)
      std::sort(h->hits.begin() + h->off[r], h->hits.begin() + h->off[r + 1], [](const herro_adapter_hit& x, const herro_adapter_hit& y) {
        if (x.end != y.end) return x.end < y.end;
        if (x.start != y.start) return x.start < y.start;
        if (x.adapter != y.adapter) return x.adapter < y.adapter;
        return x.strand < y.strand;
      });
  });
  if (const char* e = getenv("HERRO_ADAPT_STATS")) {
    if (atoi(e))
      fprintf(stderr, "ADAPT seg=%llu segments=%llu patterns=%u hits=%llu scans=%llu scan_ms=%.3f start_ms=%.3f host_ms=%.3f\n", (unsigned long long)stats.seg,
              (unsigned long long)stats.segments, (uint32_t)((p.flags & HERRO_ADAPTERS_FORWARD_ONLY) ? n_adapters : 2 * n_adapters),
              (unsigned long long)stats.hits, (unsigned long long)stats.scans, stats.scan_ms, stats.start_ms, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  }
  *out = h.release();
  return HERRO_OK;
}

uint64_t herro_adapter_hits_n(const herro_adapter_hits* h) { return h ? h->hits.size() : 0; }
const herro_adapter_hit* herro_adapter_hits_data(const herro_adapter_hits* h) { return h ? h->hits.data() : nullptr; }
const uint64_t* herro_adapter_hits_off(const herro_adapter_hits* h) { return h ? h->off.data() : nullptr; }
void herro_adapter_hits_free(herro_adapter_hits* h) { delete h; }

// Test hook: the hits the buffer of a call's first scan holds (0: the default), so that a small read set can outgrow it
int herro_debug_set_adapter_cap(herro_ctx* ctx, uint64_t cap) {
  if (!ctx) return HERRO_E_INVALID;
  ctx->debug_adapter_cap = cap;
  return HERRO_OK;
}

// ---- the store cut to a piece table on the device ("The cut on the device"; store_dev.hip) ---------------------------
// The host's share: the table's checks and the new offsets (store_cut_plan), then the context's state as herro_set_reads leaves it.
int herro_store_cut(herro_ctx* ctx, uint64_t n_pieces, const herro_piece* pieces, const uint32_t* name_class) {
  if (!ctx) return HERRO_E_INVALID;
  try {
    // everything the host allocates comes first: an allocation that fails leaves the store as it was
    std::vector<uint64_t> word_off, qual_off;
    std::string msg;
    if (int rc = herro::store_cut_plan(ctx->n_reads, ctx->read_len.data(), n_pieces, pieces, word_off, qual_off, msg)) { ctx->err = msg; return rc; }
    if (int rc = device_ready(ctx, "herro_store_cut")) return rc;
    const uint32_t n = (uint32_t)n_pieces;
    std::vector<uint32_t> len(n), nc(n);
    for (uint32_t x = 0; x < n; x++) { len[x] = pieces[x].end - pieces[x].start; nc[x] = name_class ? name_class[x] : x; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // what is queued reads the store that this context is about to let go
    const char* const e = getenv("HERRO_CUT_STATS");
    const int stats_level = e ? atoi(e) : 0;
    herro::StoreCutStats stats;
    const herro::StoreArrays old{ctx->d_words, ctx->d_word_off, ctx->d_qual, ctx->d_qual_off, ctx->d_p0, ctx->d_p1};
    herro::StoreArrays S;
    if (herro::store_cut(old, pieces, n, word_off, qual_off, ctx->stream, S, stats_level > 0 ? &stats : nullptr, stats_level, msg) != hipSuccess) {
      ctx->err = msg;
      return HERRO_E_NO_DEVICE;
    }
    void* const ptrs[6] = {(void*)S.words, (void*)S.word_off, (void*)S.qual, (void*)S.qual_off, (void*)S.p0, (void*)S.p1};
    std::shared_ptr<void> owner;
    try {
      owner = make_store_owner(ctx->device, ptrs);
    } catch (...) {
      for (void* q : ptrs) if (q) (void)hipFree(q);
      throw;
    }
    // from here on nothing can fail
    ctx->store_owner = std::move(owner);   // lets the old store go: freed unless another context still shares it
    ctx->d_words = S.words; ctx->d_word_off = S.word_off; ctx->d_qual = S.qual; ctx->d_qual_off = S.qual_off; ctx->d_p0 = S.p0; ctx->d_p1 = S.p1;
    ctx->n_reads = n;
    ctx->read_len.swap(len);
    ctx->name_class.swap(nc);
    ctx->n_words = word_off[n];
    ctx->qual_bytes = qual_off[n];
    ctx->read_bytes = ctx->n_words * 8 + ctx->qual_bytes;
    ctx->h_word_off.swap(word_off);
    ctx->h_qual_off.swap(qual_off);
    ctx->reads_gen++;   // jobs built on the previous store refuse to run from here on
    if (stats_level > 0)
      fprintf(stderr, "CUT pieces=%u words=%llu qual_bytes=%llu words_ms=%.4f qual_ms=%.4f copy_words_ms=%.4f copy_qual_ms=%.4f\n", n, (unsigned long long)ctx->n_words,
              (unsigned long long)ctx->qual_bytes, stats.words_ms, stats.qual_ms, stats.copy_words_ms, stats.copy_qual_ms);
    return HERRO_OK;
  } catch (const std::exception& e) {   // host memory: nothing of the context was touched
    ctx->err = std::string("herro_store_cut: ") + e.what();
    return HERRO_E_UNSUPPORTED;
  }
}

// Test hook: one array of the context's store as it lies on the device.
int64_t herro_debug_store_copy(herro_ctx* ctx, int which, void* out, uint64_t cap) {
  if (!ctx) return HERRO_E_INVALID;
  if (which < 0 || which > 5) { ctx->err = "herro_debug_store_copy: which is 0 .. 5"; return HERRO_E_INVALID; }
  if (int rc = device_ready(ctx, "herro_debug_store_copy")) return rc;
  const void* const src[6] = {ctx->d_words, ctx->d_word_off, ctx->d_qual, ctx->d_qual_off, ctx->d_p0, ctx->d_p1};
  const uint64_t bytes[6] = {8 * (ctx->n_words + 1), 8 * ((uint64_t)ctx->n_reads + 1), ctx->qual_bytes, 8 * ((uint64_t)ctx->n_reads + 1),
                             4 * (ctx->n_words + 2), 4 * (ctx->n_words + 2)};
  if (!out) return (int64_t)bytes[which];
  if (cap < bytes[which]) { ctx->err = "herro_debug_store_copy: the buffer is smaller than the array"; return HERRO_E_INVALID; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (bytes[which]) HIP_TRY(ctx, hipMemcpy(out, src[which], bytes[which], hipMemcpyDeviceToHost));
  return (int64_t)bytes[which];
}

// ---- test hooks: the shared scan and radix sort (scan_sort_dev.hip) and the 64-bit offset join (fasta_dev.hip) on arrays of the caller's ----------
// The arrays are carved from ONE device block, as fasta_dev.hip's Carver and cluster_dev.hip's Bufs lay theirs next to live arrays, every one
// exactly as large as its client sizes it and with GUARD_WORDS words of a fixed pattern directly behind it: a store one entry past an array or past
// dev_scan_partials(n) / dev_sort_scratch(n) lands in a guard and is counted, where in a client it would change a neighbour without any fault.
namespace {
constexpr uint32_t GUARD_WORDS = 64;
inline uint32_t guard_word(uint32_t i) { return 0xA5C3E1F0u ^ (i * 0x01010101u); }

struct Guarded {
  struct Part { uint64_t at, bytes; };
  std::vector<Part> parts;
  uint64_t total = 0;
  char* base = nullptr;
  size_t add(uint64_t bytes) {                       // an array of `bytes` (a multiple of 4) at an 8-byte boundary, its guard behind it
    total = (total + 7) & ~7ull;
    parts.push_back(Part{total, bytes});
    total += bytes + 4ull * GUARD_WORDS;
    return parts.size() - 1;
  }
  uint32_t* u32(size_t i) const { return (uint32_t*)(base + parts[i].at); }
  uint64_t* u64(size_t i) const { return (uint64_t*)(base + parts[i].at); }
  hipError_t alloc(herro::Bufs& B, hipStream_t st) {  // the block, and the pattern into every guard
    hipError_t e = B.bytes(&base, total);
    uint32_t g[GUARD_WORDS];
    for (uint32_t i = 0; i < GUARD_WORDS; i++) g[i] = guard_word(i);
    for (size_t i = 0; e == hipSuccess && i < parts.size(); i++) e = hipMemcpyAsync(base + parts[i].at + parts[i].bytes, g, sizeof g, hipMemcpyHostToDevice, st);
    return e == hipSuccess ? hipStreamSynchronize(st) : e;   // (g leaves the stack)
  }
  hipError_t hits(hipStream_t st, uint32_t* n_changed) {    // waits for the stream; counts the guard words that no longer hold the pattern
    std::vector<uint32_t> g((size_t)GUARD_WORDS * parts.size());
    hipError_t e = hipSuccess;
    for (size_t i = 0; e == hipSuccess && i < parts.size(); i++)
      e = hipMemcpyAsync(g.data() + i * GUARD_WORDS, base + parts[i].at + parts[i].bytes, 4ull * GUARD_WORDS, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    *n_changed = 0;
    for (size_t i = 0; e == hipSuccess && i < g.size(); i++) *n_changed += g[i] != guard_word((uint32_t)(i % GUARD_WORDS));
    return e;
  }
};

// What the three hooks (`who`) ask before anything runs: a context with a device, and at most 2^31 - 1 elements.
int debug_prims_ready(herro_ctx* ctx, const char* who, uint64_t n) {
  if (ctx->host_only) { ctx->err = std::string(who) + ": the context has no device"; return HERRO_E_NO_DEVICE; }
  if (n > 0x7fffffffull) { ctx->err = std::string(who) + ": more than 2^31 - 1 elements"; return HERRO_E_UNSUPPORTED; }
  return HERRO_OK;
}
}  // namespace

int herro_debug_scan_u32(herro_ctx* ctx, const uint32_t* in, uint64_t n, uint32_t* out, uint32_t* guard_hits) {
  if (!ctx) return HERRO_E_INVALID;
  const char* const who = "herro_debug_scan_u32";
  if (!out || !guard_hits || (n && !in)) { ctx->err = std::string(who) + ": null argument"; return HERRO_E_INVALID; }
  if (int rc = debug_prims_ready(ctx, who, n)) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  herro::Bufs B;
  Guarded Q;
  const size_t a_in = Q.add(4 * n), a_out = Q.add(4 * (n + 1)), a_part = Q.add(4ull * herro::dev_scan_partials((uint32_t)n));
  FRONT_TRY(ctx, who, "device block", Q.alloc(B, ctx->stream));
  if (n) FRONT_TRY(ctx, who, "upload", hipMemcpyAsync(Q.u32(a_in), in, 4 * n, hipMemcpyHostToDevice, ctx->stream));
  std::string msg;
  if (herro::dev_scan_u32(Q.u32(a_in), (uint32_t)n, Q.u32(a_out), Q.u32(a_part), ctx->stream, msg) != herro::OVL_OK) {
    (void)hipStreamSynchronize(ctx->stream);
    ctx->err = std::string(who) + ": " + msg;
    return HERRO_E_NO_DEVICE;
  }
  FRONT_TRY(ctx, who, "download", hipMemcpyAsync(out, Q.u32(a_out), 4 * (n + 1), hipMemcpyDeviceToHost, ctx->stream));
  FRONT_TRY(ctx, who, "guards", Q.hits(ctx->stream, guard_hits));
  return HERRO_OK;
}

int herro_debug_chain(herro_ctx* ctx, uint64_t n_groups, const uint64_t* group_off, const uint32_t* tpos, const uint32_t* qpos,
                      const herro_overlap_params* params, int32_t* out) {
  if (!ctx) return HERRO_E_INVALID;
  const char* const who = "herro_debug_chain";
  if (!group_off || (n_groups && (!out || !tpos || !qpos))) { ctx->err = std::string(who) + ": null argument"; return HERRO_E_INVALID; }
  herro::OvlParams P;
  if (int rc = overlap_params(ctx, params, P)) return rc;
  if (group_off[0] != 0) { ctx->err = std::string(who) + ": group_off[0] must be 0"; return HERRO_E_INVALID; }
  for (uint64_t g = 0; g < n_groups; g++) {
    const uint64_t a = group_off[g], b = group_off[g + 1];
    std::string why;
    if (b <= a) why = "is empty";
    for (uint64_t i = a; why.empty() && i < b; i++) {
      if ((tpos[i] | qpos[i]) >> 31) why = "holds a coordinate of 2^31 or more";
      else if (i > a && ((uint64_t)tpos[i] << 32 | qpos[i]) <= ((uint64_t)tpos[i - 1] << 32 | qpos[i - 1])) why = "is not strictly ascending by (tpos, qpos)";
    }
    if (!why.empty()) { ctx->err = std::string(who) + ": group " + std::to_string(g) + " " + why; return HERRO_E_INVALID; }
  }
  if (n_groups > 0x7fffffffull) { ctx->err = std::string(who) + ": more than 2^31 - 1 groups"; return HERRO_E_UNSUPPORTED; }
  if (int rc = debug_prims_ready(ctx, who, group_off[n_groups])) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  try {
    std::string msg;
    const int rc = herro::ovl_chain_groups(n_groups, group_off, tpos, qpos, P, ctx->stream, out, msg);
    return overlap_rc(ctx, rc, std::string(who) + ": " + msg);
  } catch (const std::exception& e) {
    ctx->err = std::string(who) + ": " + e.what();
    return HERRO_E_UNSUPPORTED;
  }
}

int herro_debug_radix_sort(herro_ctx* ctx, uint64_t* keys, uint64_t* pays, uint64_t n, const uint32_t* shifts, uint32_t n_shifts, uint32_t* guard_hits) {
  if (!ctx) return HERRO_E_INVALID;
  const char* const who = "herro_debug_radix_sort";
  if (!guard_hits || (n && (!keys || !pays)) || (n_shifts && !shifts)) { ctx->err = std::string(who) + ": null argument"; return HERRO_E_INVALID; }
  for (uint32_t i = 0; i < n_shifts; i++)
    if (shifts[i] > 63) { ctx->err = std::string(who) + ": shift " + std::to_string(i) + " is above 63"; return HERRO_E_INVALID; }
  if (int rc = debug_prims_ready(ctx, who, n)) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  herro::Bufs B;
  Guarded Q;
  size_t arr[4];                                     // k0, p0, k1, p1
  for (size_t& a : arr) a = Q.add(8 * n);
  const size_t a_scr = Q.add(4ull * herro::dev_sort_scratch(n));
  FRONT_TRY(ctx, who, "device block", Q.alloc(B, ctx->stream));
  uint64_t *k0 = Q.u64(arr[0]), *p0 = Q.u64(arr[1]), *k1 = Q.u64(arr[2]), *p1 = Q.u64(arr[3]);
  if (n) {
    FRONT_TRY(ctx, who, "key upload", hipMemcpyAsync(k0, keys, 8 * n, hipMemcpyHostToDevice, ctx->stream));
    FRONT_TRY(ctx, who, "payload upload", hipMemcpyAsync(p0, pays, 8 * n, hipMemcpyHostToDevice, ctx->stream));
  }
  std::string msg;
  const std::vector<uint32_t> sh(shifts, shifts + n_shifts);
  if (herro::dev_radix_sort(&k0, &p0, &k1, &p1, (uint32_t)n, sh, Q.u32(a_scr), ctx->stream, msg) != herro::OVL_OK) {
    (void)hipStreamSynchronize(ctx->stream);
    ctx->err = std::string(who) + ": " + msg;
    return HERRO_E_NO_DEVICE;
  }
  if (n) {
    FRONT_TRY(ctx, who, "key download", hipMemcpyAsync(keys, k0, 8 * n, hipMemcpyDeviceToHost, ctx->stream));
    FRONT_TRY(ctx, who, "payload download", hipMemcpyAsync(pays, p0, 8 * n, hipMemcpyDeviceToHost, ctx->stream));
  }
  FRONT_TRY(ctx, who, "guards", Q.hits(ctx->stream, guard_hits));
  return HERRO_OK;
}

int herro_debug_offsets64(herro_ctx* ctx, const uint64_t* bytes, uint64_t n, uint64_t* off, uint32_t* guard_hits) {
  if (!ctx) return HERRO_E_INVALID;
  const char* const who = "herro_debug_offsets64";
  if (!off || !guard_hits || (n && !bytes)) { ctx->err = std::string(who) + ": null argument"; return HERRO_E_INVALID; }
  if (int rc = debug_prims_ready(ctx, who, n)) return rc;
  *guard_hits = 0;
  if (!n) { off[0] = 0; return HERRO_OK; }           // (fasta_text_dev never gets here without a piece)
  try {
    std::vector<uint32_t> halves(2 * n);             // what k_fa_piece leaves: lo_in, then hi_in
    for (uint64_t p = 0; p < n; p++) { halves[p] = (uint32_t)bytes[p]; halves[n + p] = (uint32_t)(bytes[p] >> 32); }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    herro::Bufs B;
    Guarded Q;
    const size_t a_off = Q.add(8 * (n + 1)), a_lo_in = Q.add(4 * n), a_hi_in = Q.add(4 * n), a_lo = Q.add(4 * (n + 1)), a_hi = Q.add(4 * (n + 1)),
                 a_part = Q.add(4ull * herro::dev_scan_partials((uint32_t)n));
    FRONT_TRY(ctx, who, "device block", Q.alloc(B, ctx->stream));
    FRONT_TRY(ctx, who, "upload", hipMemcpyAsync(Q.u32(a_lo_in), halves.data(), 4 * n, hipMemcpyHostToDevice, ctx->stream));
    FRONT_TRY(ctx, who, "upload", hipMemcpyAsync(Q.u32(a_hi_in), halves.data() + n, 4 * n, hipMemcpyHostToDevice, ctx->stream));
    std::string msg;
    if (herro::fasta_offsets64(Q.u32(a_lo_in), Q.u32(a_hi_in), (uint32_t)n, Q.u32(a_lo), Q.u32(a_hi), Q.u64(a_off),
                               Q.u32(a_part), ctx->stream, msg) != herro::FASTA_OK) {
      ctx->err = std::string(who) + ": " + msg;      // (the stream is idle: fasta_dev.hip waits before it reports)
      return HERRO_E_NO_DEVICE;
    }
    FRONT_TRY(ctx, who, "download", hipMemcpyAsync(off, Q.u64(a_off), 8 * (n + 1), hipMemcpyDeviceToHost, ctx->stream));
    FRONT_TRY(ctx, who, "guards", Q.hits(ctx->stream, guard_hits));
    return HERRO_OK;
  } catch (const std::exception& e) {
    ctx->err = std::string(who) + ": " + e.what();
    return HERRO_E_UNSUPPORTED;
  }
}

// ---- clusters: the reads partitioned by their overlap graph (cluster_dev.hip, cluster_plan.h) -----------------------------
// The host's share: the checks (cluster_check), the edges of a pairs handle, and the handle, which keeps the graph on the device for the masks.
struct herro_clusters {
  herro_ctx* ctx = nullptr;
  int device = 0;
  herro::ClGraph G;
  herro::ClResult R;
};

namespace {
int cluster_run(herro_ctx* ctx, const char* who, uint64_t n_reads, const uint32_t* weights, uint64_t n_edges, const uint32_t* a, const uint32_t* b,
                const uint32_t* span, const herro_cluster_params* params, herro_clusters** out) {
  try {
    std::string msg;
    if (int rc = herro::cluster_check(who, n_reads, weights, n_edges, a, b, params, nullptr, msg)) { ctx->err = msg; return rc; }
    if (ctx->host_only) { ctx->err = std::string(who) + ": the context has no device"; return HERRO_E_NO_DEVICE; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<herro_clusters> h(new herro_clusters());
    h->ctx = ctx;
    h->device = ctx->device;
    const char* const e = getenv("HERRO_CLUSTER_STATS");
    herro::ClTimes times;
    const bool stats = e && atoi(e) > 0;
    if (herro::cl_build((uint32_t)n_reads, weights, (uint32_t)n_edges, a, b, span, params->n_parts, params->min_span, ctx->stream, h->G, h->R,
                        stats ? &times : nullptr, msg) != herro::CL_OK) {
      ctx->err = std::string(who) + ": " + msg;
      return HERRO_E_NO_DEVICE;
    }
    if (stats)
      fprintf(stderr, "CLUSTER reads=%llu edges=%llu parts=%u components=%llu levels=%llu edge_cut=%llu arcs_ms=%.4f comp_ms=%.4f bfs_ms=%.4f order_ms=%.4f stats_ms=%.4f hook_rounds=%u bfs_launches=%u host_reads=%u\n",
              (unsigned long long)n_reads, (unsigned long long)n_edges, params->n_parts, (unsigned long long)h->R.stats[0], (unsigned long long)h->R.stats[1],
              (unsigned long long)h->R.stats[3], times.arcs_ms, times.comp_ms, times.bfs_ms, times.order_ms, times.stats_ms, times.hook_rounds, times.bfs_launches,
              times.host_reads);
    *out = h.release();
    return HERRO_OK;
  } catch (const std::exception& e) {   // host memory (four arrays of n_reads entries): nothing was handed out
    ctx->err = std::string(who) + ": " + e.what();
    return HERRO_E_UNSUPPORTED;
  }
}
}  // namespace

int herro_cluster_graph(herro_ctx* ctx, uint64_t n_reads, const uint32_t* weights, uint64_t n_edges, const uint32_t* a, const uint32_t* b, const uint32_t* span,
                        const herro_cluster_params* params, herro_clusters** out) {
  if (!ctx || !out) return HERRO_E_INVALID;
  *out = nullptr;
  return cluster_run(ctx, "herro_cluster_graph", n_reads, weights, n_edges, a, b, span, params, out);
}

// The primaries of a handle lie on the host (herro_pairs keeps no device copy of them): their (tid, qid, span) go up as herro_cluster_graph's edges do.
int herro_pairs_cluster(herro_ctx* ctx, const herro_pairs* pairs, const uint32_t* weights, const herro_cluster_params* params, herro_clusters** out) {
  if (!ctx || !out) return HERRO_E_INVALID;
  *out = nullptr;
  const char* const who = "herro_pairs_cluster";
  if (!pairs) { ctx->err = std::string(who) + ": pairs is NULL"; return HERRO_E_INVALID; }
  if (pairs->ctx != ctx) { ctx->err = std::string(who) + ": the pairs handle belongs to another context"; return HERRO_E_INVALID; }
  const size_t P = pairs->alns.size();
  std::vector<uint32_t> a, b, span;
  try {
    a.resize(P); b.resize(P); span.resize(P);
  } catch (const std::exception& e) {
    ctx->err = std::string(who) + ": " + e.what();
    return HERRO_E_UNSUPPORTED;
  }
  for (size_t p = 0; p < P; p++) {
    const herro_alignment& r = pairs->alns[p];
    a[p] = r.tid; b[p] = r.qid;
    span[p] = std::min(r.tend - r.tstart, r.qend - r.qstart);
  }
  return cluster_run(ctx, who, ctx->n_reads, weights, P, a.data(), b.data(), span.data(), params, out);
}

uint32_t herro_clusters_n_parts(const herro_clusters* cl) { return cl ? cl->G.k : 0; }
uint64_t herro_clusters_n_reads(const herro_clusters* cl) { return cl ? cl->R.part.size() : 0; }
const uint32_t* herro_clusters_part(const herro_clusters* cl) { return cl ? cl->R.part.data() : nullptr; }
const uint32_t* herro_clusters_rank(const herro_clusters* cl) { return cl ? cl->R.rank.data() : nullptr; }
const uint32_t* herro_clusters_comp(const herro_clusters* cl) { return cl ? cl->R.comp.data() : nullptr; }
const uint32_t* herro_clusters_level(const herro_clusters* cl) { return cl ? cl->R.level.data() : nullptr; }

int herro_clusters_stats(const herro_clusters* cl, uint64_t out[4]) {
  if (!cl || !out) return HERRO_E_INVALID;
  for (int i = 0; i < 4; i++) out[i] = cl->R.stats[i];
  return HERRO_OK;
}

int herro_clusters_part_stats(const herro_clusters* cl, uint32_t p, uint64_t out[5]) {
  if (!cl || !out) return HERRO_E_INVALID;
  if (p >= cl->G.k) { cl->ctx->err = "herro_clusters_part_stats: part " + std::to_string(p) + " of " + std::to_string(cl->G.k); return HERRO_E_INVALID; }
  for (int i = 0; i < 5; i++) out[i] = cl->R.part_stats[(size_t)p * 5 + i];
  return HERRO_OK;
}

int herro_clusters_mask(const herro_clusters* cl, uint32_t p, uint8_t* out) {
  if (!cl) return HERRO_E_INVALID;
  herro_ctx* const ctx = cl->ctx;
  if (p >= cl->G.k) { ctx->err = "herro_clusters_mask: part " + std::to_string(p) + " of " + std::to_string(cl->G.k); return HERRO_E_INVALID; }
  if (!out && !cl->R.part.empty()) { ctx->err = "herro_clusters_mask: out is NULL"; return HERRO_E_INVALID; }
  HIP_TRY(ctx, hipSetDevice(cl->device));
  std::string msg;
  if (herro::cl_mask(cl->G, p, ctx->stream, out, msg) != herro::CL_OK) { ctx->err = "herro_clusters_mask: " + msg; return HERRO_E_NO_DEVICE; }
  return HERRO_OK;
}

void herro_clusters_free(herro_clusters* cl) {
  if (!cl) return;
  if (cl->G.n && hipSetDevice(cl->device) != hipSuccess) { cl->G.d_a = cl->G.d_b = cl->G.d_part = nullptr; cl->G.d_mask = nullptr; }   // (no device to free on)
  delete cl;
}

}  // extern "C"
