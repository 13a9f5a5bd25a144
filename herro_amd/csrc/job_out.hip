// job_out.hip — what comes out of a job (include/herro_amd.h): window descriptions and planes, the logits, the corrected bases, the three FASTA entries
// (herro_job_consensus_fasta, herro_job_fasta, herro_job_fasta_dev with its text handle), the feature files, the job's statistics, and the test hooks that
// read or replace a job's arrays.  Host C++ (compiled by hipcc); every fetch of model results goes through settle_pass (job_run.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "api_job.h"
#include "chop_plan.h"
#include "fasta_dev.h"

using namespace herro;

// herro_debug_job_array: n elements of a job's device array, behind everything the device has in flight, into the debug vector v
template <class T>
static int64_t debug_fetch(herro_job* job, std::vector<T>& v, const void* d_src, size_t n, const void** ptr) {
  v.resize(n);
  if (hipSetDevice(job->ctx->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
      (n && hipMemcpy(v.data(), d_src, n * sizeof(T), hipMemcpyDeviceToHost) != hipSuccess)) return HERRO_E_NO_DEVICE;
  *ptr = v.data();
  return (int64_t)n;
}

extern "C" {

uint32_t herro_job_n_windows(const herro_job* job) { return job ? (uint32_t)job->win.size() : 0; }

int herro_job_window_info(herro_job* job, uint32_t w, herro_window_info* info) {
  if (!job || !info || w >= job->win.size()) return HERRO_E_INVALID;
  int rc = job_sync(job);
  if (rc) return rc;
  const WinDesc& wd = job->win[w];
  info->rid = wd.rid; info->wid = wd.wid; info->n_total_wins = wd.n_wids;
  info->length = job->h_Lf[w];
  info->n_overlaps = job->h_nkept[w];
  info->n_alns = window_alns(job, w);
  info->n_supported = job->h_nsup[w];
  info->win_len = wd.win_len;
  return HERRO_OK;
}

static int fetch_planes(herro_job* job, uint32_t w, std::vector<uint8_t>& pb, std::vector<uint8_t>* pq) {
  herro_ctx* ctx = job->ctx;
  const WinDesc& wd = job->win[w];
  const size_t bytes = (size_t)HERRO_ROWS * wd.lub;
  pb.resize(bytes);
  if (!job->tokens_full) {  // a lean featurize pass wrote no planes: build them (and the row map the quality planes need) for whoever asks
    launch_full_tokens(job->J, ctx->stream, nullptr);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    job->tokens_full = true;
  }
  HIP_TRY(ctx, hipMemcpy(pb.data(), job->J.fin_b + wd.fin_off, bytes, hipMemcpyDeviceToHost));
  if (pq) {
    if (!job->quals_full) {  // featurize leaves the quality planes to whoever asks for them
      launch_full_quals(job->J, ctx->stream);
      HIP_TRY(ctx, hipGetLastError());
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      job->quals_full = true;
    }
    pq->resize(bytes);
    HIP_TRY(ctx, hipMemcpy(pq->data(), job->J.fin_q + wd.fin_off, bytes, hipMemcpyDeviceToHost));
  }
  return HERRO_OK;
}

int herro_job_window_copy(herro_job* job, uint32_t w, int encoded, uint8_t* bases, uint8_t* quals,
                          uint16_t* sup_pos, uint8_t* sup_ins, uint32_t* qids) {
  if (!job || w >= job->win.size()) return HERRO_E_INVALID;
  int rc = job_sync(job);
  if (rc) return rc;
  herro_ctx* ctx = job->ctx;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const WinDesc& wd = job->win[w];
  const uint32_t L = job->h_Lf[w];
  if (bases || quals) {
    std::vector<uint8_t> pb, pq;
    rc = fetch_planes(job, w, pb, quals ? &pq : nullptr);
    if (rc) return rc;
    for (uint32_t r = 0; r < L; r++)
      for (uint32_t c = 0; c < HERRO_ROWS; c++) {
        if (bases) {
          const uint8_t t = pb[(size_t)c * wd.lub + r];
          bases[(size_t)r * HERRO_ROWS + c] = encoded ? t : (uint8_t)TOK_ASCII[t < 12 ? t : 12 - 1];
        }
        if (quals) quals[(size_t)r * HERRO_ROWS + c] = pq[(size_t)c * wd.lub + r];
      }
  }
  const uint32_t ns = job->h_nsup[w];
  if ((sup_pos || sup_ins) && ns) {
    std::vector<uint32_t> pi(ns);
    HIP_TRY(ctx, hipMemcpy(pi.data(), job->J.sup_pi + wd.row_off, ns * 4ull, hipMemcpyDeviceToHost));
    for (uint32_t k = 0; k < ns; k++) {
      if (sup_pos) sup_pos[k] = (uint16_t)(pi[k] & 0xffffu);
      if (sup_ins) sup_ins[k] = (uint8_t)(pi[k] >> 16);
    }
  }
  if (qids && job->h_nkept[w])
    HIP_TRY(ctx, hipMemcpy(qids, job->J.rank_qid + wd.ow_begin, job->h_nkept[w] * 4ull, hipMemcpyDeviceToHost));
  return HERRO_OK;
}

static int logits_to_host(herro_job* job) {
  herro_ctx* ctx = job->ctx;
  if (!job->inferred) { ctx->err = "herro_job_infer has not run"; return HERRO_E_STATE; }
  if (job->logits_on_host) return HERRO_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const uint64_t tot = job->sup_off.back();
  job->h_info.resize(tot);
  job->h_base.resize(tot * 5);
  if (const int rc = settle_pass(job)) return rc;
  if (tot) {
    HIP_TRY(ctx, hipMemcpy(job->h_info.data(), job->d_info, tot * 4, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(job->h_base.data(), job->d_base, tot * 20, hipMemcpyDeviceToHost));
  }
  job->logits_on_host = true;
  return HERRO_OK;
}

int herro_job_window_logits(herro_job* job, uint32_t w, float* info_logits, float* bases_logits) {
  if (!job || w >= job->win.size()) return HERRO_E_INVALID;
  int rc = logits_to_host(job);
  if (rc) return rc;
  const uint64_t o = job->sup_off[w], n = job->h_nsup[w];
  if (info_logits) std::memcpy(info_logits, job->h_info.data() + o, n * 4);
  if (bases_logits) std::memcpy(bases_logits, job->h_base.data() + o * 5, n * 20);
  return HERRO_OK;
}

// corrected bases of every window (device consensus) -> host, once per consensus pass
static int consensus_to_host(herro_job* job) {
  herro_ctx* ctx = job->ctx;
  if (job->consensus_on_host) return HERRO_OK;
  const uint32_t n = job->J.n_win;
  // device -> the job's pinned arena: no staging copy, no page pinning by the runtime at call time (a pageable destination
  // made the runtime lock user pages under the mm lock, which stalled the page faults of whoever was building the next job:
  // 40 ms spikes in the other feeder's herro_job_create)
  // The copies are queued in front of the wait of settle_pass, so a clean pass costs one synchronisation; after a repeat they are queued again, for what the
  // second pass decoded, and settled without a further repeat.
  auto queue_copies = [&]() -> int {
    if (n) HIP_TRY(ctx, hipMemcpyAsync(job->h_cons_len, job->J.cons_len, n * 4ull, hipMemcpyDeviceToHost, ctx->stream));
    if (job->row_elems) HIP_TRY(ctx, hipMemcpyAsync(job->h_cons_seq, job->J.cons_seq, job->row_elems, hipMemcpyDeviceToHost, ctx->stream));
    return HERRO_OK;
  };
  bool repeated = false;
  int rc = queue_copies();
  if (rc || (rc = settle_pass(job, &repeated))) return rc;
  if (repeated && ((rc = queue_copies()) || (rc = settle_model(ctx, job)))) return rc;
  job->consensus_on_host = true;
  return HERRO_OK;
}

// Brings the corrected bases of the whole job to the host (what crosses PCIe on the way out: ~4 KB per window) and
// returns their number; herro_job_consensus_fasta afterwards only assembles text.  Requires herro_job_consensus.
int herro_job_consensus_fetch(herro_job* job, uint64_t* n_bases) {
  if (!job) return HERRO_E_INVALID;
  herro_ctx* ctx = job->ctx;
  if (!job->consensus_done) { ctx->err = "herro_job_consensus has not run"; return HERRO_E_STATE; }
  ProfSpan span_(ctx, "fetch");
  (void)hipSetDevice(ctx->device);
  int rc = consensus_to_host(job);
  if (rc) return rc;
  uint64_t tot = 0;
  for (uint32_t w = 0; w < job->J.n_win; w++) tot += job->h_cons_len[w];
  if (n_bases) *n_bases = tot;
  return HERRO_OK;
}

// FASTA records of target t from the device consensus (corrected bases of every window on the host already): windows are
// concatenated, the read is split where a window has fewer than two alignments (consensus.rs:90-111, lib.rs:282-317).
// out == nullptr: only the size is computed.  Returns the bytes the records take.
static uint64_t fasta_from_device_consensus(const herro_job* job, uint32_t t, const char* id, const char* desc, char* out) {
  uint32_t st = 0, en = 0;
  if (!corrected_span(job, t, &st, &en)) return 0;
  // segments: maximal runs of corrected windows; empty segments are dropped like empty strings in the reference
  struct Seg { uint32_t a, b; uint64_t len; };
  Seg segs_small[8];
  std::vector<Seg> segs_big;
  uint32_t n_seg = 0;
  auto push = [&](uint32_t a, uint32_t b, uint64_t len) {
    if (n_seg < 8) segs_small[n_seg] = Seg{a, b, len};
    else { if (n_seg == 8) segs_big.assign(segs_small, segs_small + 8); segs_big.push_back(Seg{a, b, len}); }
    n_seg++;
  };
  uint32_t run0 = st;
  uint64_t run_len = 0;
  for (uint32_t w = st; w < en; w++) {
    if (!window_corrected(job, w)) {
      if (run_len) push(run0, w, run_len);
      run0 = w + 1; run_len = 0;
      continue;
    }
    run_len += job->h_cons_len[w];
  }
  if (run_len) push(run0, en, run_len);
  const Seg* segs = n_seg > 8 ? segs_big.data() : segs_small;
  const size_t id_len = strlen(id), desc_len = desc ? strlen(desc) : 0;
  uint64_t o = 0;
  char num[16];
  for (uint32_t i = 0; i < n_seg; i++) {
    int nd = 0;
    if (n_seg > 1) nd = snprintf(num, sizeof num, ":%u", i);
    const uint64_t head = 1 + id_len + (uint64_t)nd + 1 + desc_len + 1;   // '>' id [:i] ' ' [desc] '\n'
    if (out) {
      char* p = out + o;
      *p++ = '>';
      memcpy(p, id, id_len); p += id_len;
      memcpy(p, num, (size_t)nd); p += nd;
      *p++ = ' ';
      if (desc_len) { memcpy(p, desc, desc_len); p += desc_len; }
      *p++ = '\n';
      for (uint32_t w = segs[i].a; w < segs[i].b; w++) {
        if (!window_corrected(job, w)) continue;
        memcpy(p, job->h_cons_seq + job->win[w].row_off, job->h_cons_len[w]);
        p += job->h_cons_len[w];
      }
      *p++ = '\n';
    }
    o += head + segs[i].len + 1;
  }
  return o;
}

// consensus.rs:86-227 + lib.rs:282-317 on the host, from device results.
int64_t herro_job_consensus_fasta(herro_job* job, uint32_t t, const char* id, const char* desc, char* out,
                                  uint64_t cap) {
  if (!job || t >= job->n_targets || !id || !out) return HERRO_E_INVALID;
  herro_ctx* ctx = job->ctx;
  int rc = job_sync(job);
  if (rc) return rc;
  const uint32_t w0 = job->tgt_win_off[t], w1 = job->tgt_win_off[t + 1];
  bool need_logits = false;
  for (uint32_t w = w0; w < w1; w++) need_logits |= job->h_nsup[w] > 0 && window_corrected(job, w);
  if (need_logits && (rc = logits_to_host(job))) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  uint32_t st = 0, en = 0;
  if (!corrected_span(job, t, &st, &en)) return 0;
  std::vector<std::string> seqs;
  std::string cur;
  if (job->consensus_done) {  // device consensus: concatenate the windows' corrected bases
    if ((rc = consensus_to_host(job))) return rc;
    const uint64_t need = fasta_from_device_consensus(job, t, id, desc, nullptr);
    if (need > cap) { ctx->err = "output buffer too small"; return HERRO_E_INVALID; }
    fasta_from_device_consensus(job, t, id, desc, out);
    return (int64_t)need;
  }
  static const char UP[10] = {'A', 'C', 'G', 'T', '*', 'A', 'C', 'G', 'T', '*'};
  static const int CNT[10] = {0, 1, 2, 3, 4, 0, 1, 2, 3, 4};
  std::vector<uint8_t> pb;
  for (uint32_t w = st; w < en; w++) {
    const uint32_t n_alns = window_alns(job, w);
    if (!window_corrected(job, w)) {
      if (!cur.empty()) { seqs.push_back(cur); cur.clear(); }
      continue;
    }
    const WinDesc& wd = job->win[w];
    const uint32_t L = job->h_Lf[w], ns = job->h_nsup[w], n_rows = n_alns + 1;
    if ((rc = fetch_planes(job, w, pb, nullptr))) return rc;
    std::vector<uint32_t> srow(ns);
    if (ns) HIP_TRY(ctx, hipMemcpy(srow.data(), job->J.sup_row + wd.row_off, ns * 4ull, hipMemcpyDeviceToHost));
    const float* bl = ns ? job->h_base.data() + job->sup_off[w] * 5 : nullptr;
    uint32_t k = 0;  // informative rows are sorted by row, so one cursor replaces the hash map
    for (uint32_t r = 0; r < L; r++) {
      char base;
      if (k < ns && srow[k] == r) {
        const float* b = bl + (size_t)k * 5;
        int arg = 0;  // max_by_key: the LAST maximum wins; NaN is the greatest (consensus.rs:136-141)
        for (int c = 1; c < 5; c++) {
          const float v = b[c], m = b[arg];
          const bool ge = std::isnan(v) ? true : (std::isnan(m) ? false : v >= m);
          if (ge) arg = c;
        }
        base = "ACGT*"[arg];
        k++;
      } else {
        uint8_t counts[5] = {0, 0, 0, 0, 0};
        for (uint32_t c = 0; c < n_rows; c++) {
          const uint8_t tk = pb[(size_t)c * wd.lub + r];
          if (tk != TOK_NONE) {
            if (tk >= 10) { ctx->err = "token >= 10 in consensus"; return HERRO_E_REFERENCE_PANIC; }
            counts[CNT[tk]]++;
          }
        }
        int ord[5] = {0, 1, 2, 3, 4};
        std::stable_sort(ord, ord + 5, [&](int a, int b) { return counts[a] > counts[b]; });
        const uint8_t c0 = counts[ord[0]], c1 = counts[ord[1]];
        const char b0 = UP[ord[0]], b1 = UP[ord[1]];
        const uint8_t t0 = pb[r];
        if (t0 >= 10) { ctx->err = "target token >= 10 in consensus"; return HERRO_E_REFERENCE_PANIC; }
        const char tb = UP[t0];
        base = (c0 < 2 || (c0 == c1 && (b0 == tb || b1 == tb))) ? tb : b0;
      }
      if (base != '*') cur.push_back(base);
    }
  }
  if (!cur.empty()) seqs.push_back(cur);
  std::string fa;
  for (size_t i = 0; i < seqs.size(); i++) {  // lib.rs:282-317
    fa += ">";
    fa += id;
    if (seqs.size() == 1) fa += " ";
    else fa += ":" + std::to_string(i) + " ";
    if (desc) fa += desc;
    fa += "\n";
    fa += seqs[i];
    fa += "\n";
  }
  if (fa.size() > cap) { ctx->err = "output buffer too small"; return HERRO_E_INVALID; }
  std::memcpy(out, fa.data(), fa.size());
  return (int64_t)fa.size();
}

int64_t herro_job_fasta(herro_job* job, const char* const* ids, const char* const* descs, char* out, uint64_t cap,
                        uint64_t* rec_end) {
  if (!job || (job->n_targets && !ids)) return HERRO_E_INVALID;
  herro_ctx* ctx = job->ctx;
  if (!job->consensus_done) { ctx->err = "herro_job_consensus has not run"; return HERRO_E_STATE; }
  int rc = job_sync(job);
  if (rc) return rc;
  (void)hipSetDevice(ctx->device);
  if ((rc = consensus_to_host(job))) return rc;
  const uint32_t nt = job->n_targets;
  // sizes first (cheap: sums of window lengths), then every target's text straight into the caller's buffer by the pool
  std::vector<uint64_t> end(nt + 1, 0);
  for (uint32_t t = 0; t < nt; t++) end[t + 1] = end[t] + (ids[t] ? fasta_from_device_consensus(job, t, ids[t], descs ? descs[t] : nullptr, nullptr) : 0);
  const uint64_t tot = end[nt];
  if (rec_end) for (uint32_t t = 0; t < nt; t++) rec_end[t] = end[t + 1];
  if (!out) return (int64_t)tot;
  if (tot > cap) { ctx->err = "output buffer too small (" + std::to_string(tot) + " bytes needed)"; return HERRO_E_INVALID; }
  host_pool(ctx).run((nt + 63) / 64, [&](uint32_t b) {
    for (uint32_t t = b * 64; t < std::min(nt, (b + 1) * 64); t++)
      if (ids[t]) fasta_from_device_consensus(job, t, ids[t], descs ? descs[t] : nullptr, out + end[t]);
  });
  return (int64_t)tot;
}

// ---- the corrected reads as FASTA formed on the device, chopped for the assembler (fasta_dev.hip, chop_plan.h) ----------------
// herro_job_fasta's records (consensus.rs:90-111, lib.rs:282-317) and scripts/postprocess_corrected.sh behind them (`seqkit sliding -s 30000 -W 30000
// -g`, `seqkit seq -m 10000`), written by kernels from the bases the consensus pass left on the device: no padded window slot crosses PCIe and the
// host pool assembles nothing.  The text is copied chunk by chunk to its place in ONE pinned block that the handle owns until it is freed.
// consensus_on_host is neither read nor set: herro_job_fasta of the same job still fetches and assembles as before.
struct herro_fasta_text {
  std::shared_ptr<PinPool> pool;   // the text lies in a pinned block of the context's pool (api_ctx.h) and goes back there
  Arena block{};
  uint64_t len = 0;
  std::vector<uint64_t> target_end;
  herro::FastaStats st;
  ~herro_fasta_text() { if (pool) pool->release(block); }
};

int herro_job_fasta_dev(herro_job* job, const char* const* ids, const char* const* descs, const herro_chop_params* params, herro_fasta_text** out) {
  if (!job || !out) return HERRO_E_INVALID;
  *out = nullptr;
  herro_ctx* ctx = job->ctx;
  const char* const who = "herro_job_fasta_dev";
  if (job->n_targets && !ids) { ctx->err = std::string(who) + ": ids is NULL"; return HERRO_E_INVALID; }
  herro::ChopRule R;
  {
    std::string why;
    if (const int rc = herro::chop_check(who, params, R, why)) { ctx->err = why; return rc; }
  }
  if (!job->consensus_done) { ctx->err = "herro_job_consensus has not run"; return HERRO_E_STATE; }
  // window slots below 2^32 bytes: the base prefixes are 32-bit, and a piece has at least one base, so there are never more than 2^32 - 1 pieces
  if (job->row_elems > herro::FASTA_MAX_ROW_ELEMS) { ctx->err = std::string(who) + ": a job of 2^32 corrected bases or more (more than 2^32 - 1 pieces at chop_len 1)"; return HERRO_E_UNSUPPORTED; }
  int rc = job_sync(job);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const uint32_t nt = job->n_targets;
  herro::FastaNames names;
  names.off.assign(2ull * nt + 1, 0);
  names.present.assign(nt, 0);
  for (uint32_t t = 0; t < nt; t++) {
    names.off[2ull * t] = names.blob.size();
    if (ids[t]) { names.present[t] = 1; names.blob += ids[t]; }
    names.off[2ull * t + 1] = names.blob.size();
    if (ids[t] && descs && descs[t]) names.blob += descs[t];
  }
  names.off[2ull * nt] = names.blob.size();
  // the settle of consensus_to_host, in front of the kernels instead of behind the copy: a pass that is repeated (once) is repeated before any text is
  // formed, so the text is the second pass's
  if ((rc = settle_pass(job))) return rc;
  uint64_t chunk = ctx->debug_fasta_chunk;
  if (!chunk) chunk = std::max<uint64_t>(scratch_budget("HERRO_FASTA_SCRATCH_MB", 1024) / 16, 16);   // the two device halves stay an eighth of the budget (the division of herro_pairs_paf's chunks)
  std::unique_ptr<herro_fasta_text> h(new herro_fasta_text());
  h->pool = ctx->text_pin;
  // recycled memory: the device blocks go back to the context's list when the call is over (the stream is idle then), the pinned block with the handle
  std::vector<Arena> dev_blocks;
  herro::FastaMem mem;
  mem.dev = [&](uint64_t bytes) -> void* { dev_blocks.push_back(small_acquire(ctx, bytes)); return dev_blocks.back().p; };
  mem.text = [&](uint64_t bytes) -> char* { h->block = h->pool->acquire(bytes); return (char*)h->block.p; };
  std::string msg;
  char* text = nullptr;
  const int frc = herro::fasta_text_dev(job->J, job->row_elems, job->tgt_win_off.data(), nt, names, R, chunk, ctx->stream, mem, &text, &h->len, h->target_end, h->st, msg);
  for (Arena& a : dev_blocks) small_release(ctx, a);
  if (frc != herro::FASTA_OK) {
    ctx->err = msg;
    return HERRO_E_NO_DEVICE;
  }
  const char* e = getenv("HERRO_FASTA_STATS");   // (tools/fastarate.py): one line on stderr
  if (e && atoi(e))
    fprintf(stderr, "FASTA targets=%llu segments=%llu pieces=%llu dropped=%llu bytes=%llu chunks=%llu seg_ms=%.3f piece_ms=%.3f write_ms=%.3f\n",
            (unsigned long long)h->st.n_targets, (unsigned long long)h->st.segments, (unsigned long long)h->st.records, (unsigned long long)h->st.dropped,
            (unsigned long long)h->st.bytes, (unsigned long long)h->st.chunks, h->st.seg_ms, h->st.piece_ms, h->st.write_ms);
  *out = h.release();
  return HERRO_OK;
}

const char* herro_fasta_text_data(const herro_fasta_text* t) { return t && t->len ? (const char*)t->block.p : nullptr; }
uint64_t herro_fasta_text_len(const herro_fasta_text* t) { return t ? t->len : 0; }
const uint64_t* herro_fasta_text_target_end(const herro_fasta_text* t) { return t ? t->target_end.data() : nullptr; }
int herro_fasta_text_stats(const herro_fasta_text* t, uint64_t out[6]) {
  if (!t || !out) return HERRO_E_INVALID;
  out[0] = t->st.records; out[1] = t->st.bases; out[2] = t->st.dropped; out[3] = t->st.bases_dropped; out[4] = t->st.segments; out[5] = t->st.targets;
  return HERRO_OK;
}
void herro_fasta_text_free(herro_fasta_text* t) { delete t; }
int herro_debug_set_fasta_chunk(herro_ctx* ctx, uint64_t bytes) {
  if (!ctx) return HERRO_E_INVALID;
  ctx->debug_fasta_chunk = bytes;
  return HERRO_OK;
}

int64_t herro_job_write_features(herro_job* job, const char* base_dir, const char* const* read_names) {
  if (!job || !base_dir || !read_names) return HERRO_E_INVALID;
  herro_ctx* ctx = job->ctx;
  int rc = job_sync(job);
  if (rc) return rc;
  int64_t n = 0;
  std::vector<uint8_t> bases, quals, sins;
  std::vector<uint16_t> spos;
  std::vector<uint32_t> qids;
  std::vector<const char*> ids;
  for (uint32_t t = 0; t < job->n_targets; t++) {
    for (uint32_t w = job->tgt_win_off[t]; w < job->tgt_win_off[t + 1]; w++) {
      const WinDesc& wd = job->win[w];
      const uint32_t L = job->h_Lf[w], ns = job->h_nsup[w], nk = job->h_nkept[w];
      bases.resize((size_t)L * HERRO_ROWS); quals.resize(bases.size());
      spos.resize(ns); sins.resize(ns); qids.resize(nk); ids.resize(nk);
      if ((rc = herro_job_window_copy(job, w, 0, bases.data(), quals.data(), spos.data(), sins.data(), qids.data()))) return rc;
      for (uint32_t k = 0; k < nk; k++) {
        if (qids[k] >= ctx->n_reads || !read_names[qids[k]]) { ctx->err = "read name missing"; return HERRO_E_INVALID; }
        ids[k] = read_names[qids[k]];
      }
      if (wd.rid >= ctx->n_reads || !read_names[wd.rid]) { ctx->err = "read name missing"; return HERRO_E_INVALID; }
      const std::string dir = std::string(base_dir) + "/" + read_names[wd.rid];
      if ((rc = herro_write_window_features(dir.c_str(), wd.wid, ids.data(), nk, bases.data(), quals.data(), L, spos.data(), sins.data(), ns))) {
        ctx->err = "cannot write features under " + dir;
        return rc;
      }
      n++;
    }
  }
  return n;
}

int herro_job_stats(herro_job* job, uint64_t* out) {
  if (!job || !out) return HERRO_E_INVALID;
  int rc = job_sync(job);
  if (rc) return rc;
  uint64_t sumL = 0, sumS = 0, nz = 0;
  for (size_t w = 0; w < job->win.size(); w++) { sumL += job->h_Lf[w]; sumS += job->h_nsup[w]; nz += job->h_nsup[w] > 0; }
  out[0] = job->alg_read_bytes; out[1] = job->alg_op_bytes; out[2] = 2ull * HERRO_ROWS * sumL;
  out[3] = sumL; out[4] = sumS; out[5] = nz;
  return HERRO_OK;
}

// the directory words k_cols wrote for overlap-window `ow` (JobDev::cwd: one per word of 32 window positions; read-only, valid once herro_job_featurize
// has run, and meaningful for a slice the long-indel filter kept — a dropped slice's words are never written)
int64_t herro_debug_job_cwd(herro_job* job, uint32_t ow, uint32_t* out, uint64_t cap) {
  if (!job || !out) return HERRO_E_INVALID;
  herro_ctx* ctx = job->ctx;
  if (ctx->host_only || !job->featurized) { ctx->err = "herro_job_featurize has not run"; return HERRO_E_STATE; }
  if (ow >= job->J.n_ow || cap < job->J.nw) { ctx->err = "overlap-window index out of range or output buffer too small"; return HERRO_E_INVALID; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  HIP_TRY(ctx, hipMemcpy(out, job->J.cwd + (uint64_t)ow * job->J.nw, (size_t)job->J.nw * 4, hipMemcpyDeviceToHost));
  return (int64_t)job->J.nw;
}

// the base logits of every informative row of the job (job order, n_rows x 5) replace the model's, on the device and in the host copy; the consensus
// is dropped, so the next herro_job_consensus / herro_job_consensus_fasta decodes these (tests plant ties, infinities and NaNs for the argmax)
int herro_debug_job_set_base_logits(herro_job* job, const float* base, uint64_t n_rows) {
  if (!job || (n_rows && !base)) return HERRO_E_INVALID;
  herro_ctx* ctx = job->ctx;
  int rc = job_sync(job);
  if (rc) return rc;
  if (!job->inferred) { ctx->err = "herro_job_infer has not run"; return HERRO_E_STATE; }
  const uint64_t tot = job->sup_off.back();
  if (n_rows != tot) { ctx->err = "n_rows " + std::to_string(n_rows) + " != the job's informative rows " + std::to_string(tot); return HERRO_E_INVALID; }
  if ((rc = logits_to_host(job))) return rc;   // the model pass is settled (and its info logits on the host) before its base logits are replaced
  if (tot) {
    std::memcpy(job->h_base.data(), base, tot * 20);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpy(job->d_base, base, tot * 20, hipMemcpyHostToDevice));
  }
  job->consensus_done = false;
  job->consensus_on_host = false;
  return HERRO_OK;
}

// which: 0 ops (u32), 1 OwDesc, 2 WinDesc, 3 tile_win (u32), 4 tile_r0 (u32), 5 tgt_win_off (u32).
// Returns the element count, *ptr the array, *elem_bytes the element size.
int64_t herro_debug_job_array(herro_job* job, int which, const void** ptr, uint32_t* elem_bytes) {
  if (!job || !ptr || !elem_bytes) return HERRO_E_INVALID;
  switch (which) {
    case 0:
      *elem_bytes = 4;
      // ops written by the device scan: the whole (gapped) op array, so that OwDesc::op_begin indexes it
      if (job->scan.p) return debug_fetch(job, job->dbg_ops, job->scan.p, job->scan_ops, ptr);
      *ptr = job->ops.data();
      return (int64_t)job->ops.size();
    case 1:
      *elem_bytes = sizeof(OwDesc);
      if (job->dev_built) return debug_fetch(job, job->dbg_ow, job->J.ow, job->J.n_ow, ptr);
      *ptr = job->ow.data();
      return (int64_t)job->ow.size();
    case 2: *ptr = job->win.data(); *elem_bytes = sizeof(WinDesc); return (int64_t)job->win.size();
    case 3:
    case 4:
      *elem_bytes = 4;
      if (job->dev_built) return debug_fetch(job, which == 3 ? job->dbg_tw : job->dbg_tr, which == 3 ? job->J.tile_win : job->J.tile_r0, job->J.n_tiles, ptr);
      *ptr = which == 3 ? job->tile_win.data() : job->tile_r0.data();
      return (int64_t)(which == 3 ? job->tile_win.size() : job->tile_r0.size());
    case 5: *ptr = job->tgt_win_off.data(); *elem_bytes = 4; return (int64_t)job->tgt_win_off.size();
    default: return HERRO_E_INVALID;
  }
}

// Host-only test hook: the position-space rules of k_rows (pileup_core.h: sat2_add, sat2_merge, base_row_votes) on n count vectors.
// counts[i][5] = occurrences of A C G T * on a base row (the target's own base included), target[i] = the target's base 0..3; the
// counts are fed column by column into the saturating bit-sliced counters — split[i][5] of them into a second set that is merged in,
// as the two halves of k_rows' workgroup do — and the planes are read back: sup[i] = informative, vote[i] = the decoder's call 0..4.
int herro_debug_base_row_votes(const uint8_t* counts, const uint8_t* split, const uint8_t* target, uint32_t n, uint8_t* sup, uint8_t* vote) {
  if (!counts || !target || !sup || !vote) return HERRO_E_INVALID;
  for (uint32_t g0 = 0; g0 < n; g0 += 32) {
    const uint32_t m = std::min(32u, n - g0);
    uint32_t a0[5] = {0, 0, 0, 0, 0}, a1[5] = {0, 0, 0, 0, 0}, b0[5] = {0, 0, 0, 0, 0}, b1[5] = {0, 0, 0, 0, 0}, tsym[4] = {0, 0, 0, 0};
    const uint32_t vm = m == 32 ? 0xffffffffu : ((1u << m) - 1u);
    for (uint32_t i = 0; i < m; i++) {
      if (target[g0 + i] > 3) return HERRO_E_INVALID;
      tsym[target[g0 + i]] |= 1u << i;
    }
    for (int q = 0; q < 5; q++)
      for (uint32_t k = 0; k < 255; k++) {   // column k shows symbol q where the count exceeds k
        uint32_t xa = 0, xb = 0;
        for (uint32_t i = 0; i < m; i++) {
          const uint32_t c = counts[(size_t)(g0 + i) * 5 + q], s = split ? std::min<uint32_t>(split[(size_t)(g0 + i) * 5 + q], c) : 0u;
          if (k < c - s) xa |= 1u << i;
          if (k < s) xb |= 1u << i;
        }
        if (!xa && !xb) break;
        sat2_add(a0[q], a1[q], xa);
        sat2_add(b0[q], b1[q], xb);
      }
    for (int q = 0; q < 5; q++) sat2_merge(a0[q], a1[q], b0[q], b1[q]);
    const RowVotes r = base_row_votes(a0, a1, tsym, vm);
    for (uint32_t i = 0; i < m; i++) {
      sup[g0 + i] = (uint8_t)((r.sup >> i) & 1u);
      vote[g0 + i] = (uint8_t)(((r.v0 >> i) & 1u) | (((r.v1 >> i) & 1u) << 1) | (((r.v2 >> i) & 1u) << 2));
    }
  }
  return HERRO_OK;
}

// the decoder's vote on exact counts (insertion rows of k_rows; pileup_core.h vote5)
uint32_t herro_debug_vote5(const uint32_t* c5, uint32_t tb) {
  const uint32_t c[5] = {c5[0], c5[1], c5[2], c5[3], c5[4]};
  return vote5(c, tb);
}

}  // extern "C"
