/* herro_amd.h — C ABI of the MI355X-native HERRO hot path (libherro_amd.so).
 *
 * Scope: the per-window pileup feature generation (reference src/features.rs) and the
 * correction-model forward (reference src/inference.rs) of lbcb-sci/herro v0.1.1, as
 * hand-written HIP kernels for gfx950.  The reference has no FFI of its own; the entry
 * points below are what a cgo/Rust-FFI binding for this path would bind — each one cites
 * the reference interface it replaces.  Plain pointers and sizes only; no torch types.
 *
 * Conventions: every function returning int returns HERRO_OK (0) or a negative error code;
 * the text of the last error is available from herro_last_error().  Where the reference
 * would panic (Cargo.toml:18 panic = "abort") this library returns HERRO_E_REFERENCE_PANIC.
 * Nothing here ever falls back to a CPU implementation: without a HIP device every
 * device-touching call fails with HERRO_E_NO_DEVICE.
 */
#ifndef HERRO_AMD_H
#define HERRO_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HERRO_OK 0
#define HERRO_E_INVALID (-1)          /* bad argument */
#define HERRO_E_NO_DEVICE (-2)        /* no HIP device / HIP runtime error */
#define HERRO_E_REFERENCE_PANIC (-3)  /* input on which the reference itself panics */
#define HERRO_E_UNSUPPORTED (-4)      /* legal for the reference, not supported here */
#define HERRO_E_NO_MODEL (-5)
#define HERRO_E_STATE (-6)            /* call order violated */

#define HERRO_ROWS 31      /* target + TOP_K_SORT(30) overlaps — features.rs:22 */
#define HERRO_N_CLASSES 5  /* A C G T * — consensus.rs:142-149 */

typedef struct herro_ctx herro_ctx;
typedef struct herro_job herro_job;

/* One PAF record + its cg:Z: CIGAR — reference overlaps.rs:45-55 (Overlap) and :92-95
 * (Alignment).  strand: 0 = '+', 1 = '-'.  cigar: ASCII "\d+[MID]" (aligners.rs:252-293). */
typedef struct {
  uint32_t qid, qlen, qstart, qend;
  uint32_t strand;
  uint32_t tid, tlen, tstart, tend;
  uint32_t cigar_len;
  const uint8_t* cigar;
} herro_alignment;

/* Per-window result header — the fields of WindowExample / ConsensusWindow that the path
 * hands on (inference.rs:270-278, consensus.rs:22-33). */
typedef struct {
  uint32_t rid;          /* target read */
  uint32_t wid;          /* window index within the read */
  uint32_t n_total_wins; /* windows of that read */
  uint32_t length;       /* L' — rows after all-gap-row removal (features.rs:531-556) */
  uint32_t n_alns;       /* min(#ranked overlaps, 30) (features.rs:877) */
  uint32_t n_overlaps;   /* #ranked overlaps ("ids", features.rs:569) */
  uint32_t n_supported;  /* informative positions (features.rs:558) */
  uint32_t win_len;      /* target bases in the window */
} herro_window_info;

/* ---- library / context ------------------------------------------------------------------ */
const char* herro_version(void);
/* One context per GPU (the reference runs one worker set per `-d` device, lib.rs:154-200). */
herro_ctx* herro_create(int device_id);
void herro_destroy(herro_ctx* ctx);
const char* herro_last_error(const herro_ctx* ctx); /* ctx may be NULL (creation errors) */
/* Run all subsequent work of this context — every kernel and every copy of every entry below — on an externally owned hipStream_t.
 *   - NULL restores the context's own stream (created hipStreamNonBlocking with the context).
 *   - The legacy default stream cannot be named: its handle IS 0, which reads as NULL.  torch's current stream is that stream unless the
 *     caller entered another one, so a torch caller passes a stream it created (torch.cuda.Stream().cuda_stream, never 0); handing over
 *     torch.cuda.current_stream().cuda_stream == 0 silently selects the context's own stream, which is not ordered with torch's work.
 *   - A switch orders: the call returns once everything this context had queued on the stream it leaves is complete (it waits for that
 *     stream), so work queued before the switch — herro_job_featurize and herro_job_infer return with kernels queued — is seen by whatever
 *     runs after it, and memory recycled after it is no longer in use.  Naming the stream already in force does nothing.
 *   - The stream must outlive every job and handle of the context, or be switched away from (to NULL or another stream) before it is
 *     destroyed.
 *   - Stream capture (hipStreamBeginCapture, hipGraph) is not supported: the entries synchronise, allocate and read results back.
 * HERRO_E_INVALID for a NULL context. */
int herro_set_stream(herro_ctx* ctx, void* hip_stream);
int herro_synchronize(herro_ctx* ctx);

/* ---- 2-bit codec — haec_io.rs:121-173 (host utility, no device) --------------------------- */
/* words must hold (n+31)/32 u64.  Returns word count, or HERRO_E_REFERENCE_PANIC for a
 * byte >= 128 (the reference indexes a 128-entry table). */
int64_t herro_encode_2bit(const uint8_t* seq, uint64_t n, uint64_t* words);
int herro_decode_2bit(const uint64_t* words, uint64_t length, uint64_t start, uint64_t end,
                      int reverse_complement, uint8_t* out);

/* ---- device-resident read store — replaces `reads: &[HAECRecord]` (lib.rs:133, haec_io.rs:19-24).
 * Read i: bases seq[off[i]..off[i+1]) (ASCII; packed to 2 bit on the host exactly as
 * haec_io.rs:121-136 incl. the non-ACGT quirk), quals the same slice of `qual` (phred+33 bytes).
 * name_class (nullable): name_class[i] == name_class[j] iff reads i and j have the same id
 * string (the reference keys the haplotype ratios by read *name*, features.rs:494); NULL means
 * all names are distinct. */
int herro_set_reads(herro_ctx* ctx, uint32_t n_reads, const uint8_t* seq, const uint8_t* qual,
                    const uint64_t* off, const uint32_t* name_class);
/* Same, from already packed words (HAECSeq.data, haec_io.rs:78-81): word_off[n_reads+1]. */
int herro_set_reads_packed(herro_ctx* ctx, uint32_t n_reads, const uint64_t* words,
                           const uint64_t* word_off, const uint8_t* qual, const uint64_t* qual_off,
                           const uint32_t* name_class);
/* One read store per DEVICE: `ctx` adopts the store `from` holds (same device) instead of packing and uploading its own copy —
 * the reference's `reads: &[HAECRecord]` is likewise shared read-only by all feature threads (lib.rs:159-187).  The device memory
 * is reference-counted and freed with its last holder; a later herro_set_reads on either context gives that context a store of
 * its own again.  Jobs of `ctx` built on its previous store refuse to run, as after herro_set_reads. */
int herro_share_reads(herro_ctx* ctx, const herro_ctx* from);

/* ---- model ----------------------------------------------------------------------------------
 * Flat little-endian weight file written by tools/export_weights.py (stands in for
 * tch::CModule::load_on_device, inference.rs:185). */
int herro_load_model(herro_ctx* ctx, const char* path);
/* Operand format of the model GEMMs (accumulation is f32 in every mode; the contract is |logit error| <= 1e-3):
 *   0  f32 MFMA (exact f32)                                   2  f32 VALU (debug reference)
 *   1  bf16 hi/lo split of both operands, 3 MFMAs per product (~1e-5), transformer stack fused into one kernel
 *   3  the same arithmetic, layer by layer (what windows with > 64 informative rows run in mode 1, and windows with > 512 in modes 4, 5)
 *   4  f16: conv2 / FC / attention / QKV on single f16 operands, proj / FF1 / FF2 of every encoder layer on activation
 *      hi + lo (2 MFMAs), heads on three terms — 5.9e-4 max on 36 k rows; the DEFAULT when the model has the tuned shapes.
 *      Windows of 65 .. 512 informative rows stay on the fused stack (sibling tiles of 64 rows that exchange their K / V).
 *   5  f16, single terms everywhere but the heads (8.3e-4 end to end on random-init weights)
 *   6  as 4, with the activation remainder of proj / FF1 / FF2 as OCP e4m3 against an e4m3 copy of the weight on the K = 128 scaled MFMA
 *      (v_mfma_scale_f32_16x16x128_f8f6f4; 6.1e-4 end to end; 26 % less matrix-pipe time in those GEMMs and no faster on an MI355X — DESIGN.md §5 —
 *      so never chosen by the library; calibrated on demand)
 *   7  as 4 with FF1 / FF2 on single terms (proj keeps its two): 13 MFMA call-terms per encoder layer instead of 21
 *   8  as 4 with proj on a single term (FF1 / FF2 keep two): 20 call-terms
 * herro_load_model picks the mode itself unless this was called before: 1 when the model's shapes have no f16 kernels or
 * a weight lies outside the f16 range; otherwise it runs a calibration batch of 256 pileup-shaped rows in mode 0 (f32 MFMA) and in
 * the f16 tiers 5, 7, 8, 4 — cheapest first — and keeps the FIRST whose logits are finite and within 5e-4 (half the 1e-3 contract)
 * of mode 0; none: mode 1.  The margin of the f16 formats was measured on random-init weights; a trained model decides for itself.
 * herro_set_precision(4 .. 8) is held to the same bound — the mode is calibrated here if the load did not measure it — and refused
 * above it (HERRO_E_UNSUPPORTED; HERRO_FORCE_PRECISION=1 in A/B builds overrides); a mode set BEFORE herro_load_model is calibrated by
 * the load and replaced by mode 1 when it fails.  herro_model_describe reports the outcome, herro_precision the mode in force,
 * herro_calibration_error what a mode measured (-1: not measured). */
int herro_set_precision(herro_ctx* ctx, int mode);
int herro_precision(const herro_ctx* ctx);
/* Measurement aid: the shader clock (MHz) the device runs at right behind the work queued on the context's stream — one wave reads the
 * shader-clock and the constant-rate counters around ~40 us of dependent adds (synchronises the stream).  bench.py's `sustained` leg samples it. */
int herro_clock_probe(herro_ctx* ctx, double* shader_mhz);
float herro_calibration_error(const herro_ctx* ctx, int mode);

/* Text description of the loaded model: hyper-parameters, receptive field of an informative row (rows the conv stack
 * evaluates per token), GEMM FLOP per token and per 4096-bp window at 15 informative rows, the precision mode in force and
 * the calibration result of herro_load_model.  Returns the length of the text (truncated to cap - 1 bytes + NUL). */
int64_t herro_model_describe(const herro_ctx* ctx, char* out, uint64_t cap);

/* ---- job = a set of target reads with their alignments -------------------------------------
 * herro_job_create replaces the front half of `extract_features` (features.rs:326-361): `extract_windows`
 * (windowing.rs:44-273) for every alignment.  The CIGAR text is staged in pinned memory and decoded ON THE DEVICE (one
 * kernel, a workgroup per alignment: binary ops into the job's op array + the ops that reach a window boundary back to the
 * host); the host cuts the windows from those records, validates, and uploads the descriptors (one pinned block, one
 * asynchronous copy).  The call waits for that one short kernel on a separate high-priority stream of the context, not
 * for the context's execution stream.  Job memory is recycled through per-context arenas; the host work runs on a
 * per-context thread pool of HERRO_HOST_THREADS, default min(hardware threads / 4, 64, the cgroup CPU quota).
 * HERRO_HOST_SCAN=1 decodes the text on the host instead (same results; the device-free hook below always does).
 * Threading: a context's execution calls (featurize / infer / consensus / accessors) belong to one thread; herro_job_create
 * (host work + one asynchronous upload) may run on a SECOND thread of the same context at the same time, so that the next
 * job is built while the current one executes (bench.py end_to_end does this).
 * Alignments of target t are
 * alns[aln_off[t] .. aln_off[t+1]); every alignment must have tid == rids[t] (overlaps.rs:189-192).
 * window_size: the `-w` flag (main.rs:69-74); 16 <= window_size <= 8192 here. */
herro_job* herro_job_create(herro_ctx* ctx, uint32_t n_targets, const uint32_t* rids,
                            const uint64_t* aln_off, const herro_alignment* alns,
                            uint32_t window_size);
void herro_job_free(herro_job* job);
/* Zero-copy job creation.  herro_job_create has to get the CIGAR text of a job's alignments to the GPU; by default it gathers the texts
 * into a pinned staging block first.  A caller whose alignments' `cigar` pointers lie in ONE buffer — the PAF text behind
 * herro_paf_parse_view, a blob of CIGARs — registers that buffer once (it is pinned for the GPU, hipHostRegister): jobs whose texts lie
 * densely inside a registered range are then copied up straight from it, one copy, no pass over the bytes on the host.  Process-wide
 * and counted: several contexts may register the same range; unregister before the memory is freed (herro_host_unregister waits for the copies of
 * EVERY device and accepts ctx == NULL: the range outlives no particular context).  A range that cannot be pinned (the memlock limit) returns
 * HERRO_E_UNSUPPORTED and changes nothing: its jobs are staged.  (The reference has no counterpart:
 * its feature threads walk the CIGARs where the parser left them, features.rs:337-361.) */
int herro_host_register(herro_ctx* ctx, const void* p, uint64_t bytes);
int herro_host_unregister(herro_ctx* ctx, const void* p);
uint64_t herro_debug_zero_copy_jobs(void); /* test hook: jobs of this process created through the zero-copy path so far */
/* The HERRO_E_* code behind the last herro_job_create of this context that returned NULL (HERRO_OK after a successful one):
 * UNSUPPORTED / INVALID / STATE / NO_DEVICE / REFERENCE_PANIC — herro_last_error has the text. */
int herro_job_create_status(const herro_ctx* ctx);
uint32_t herro_job_n_windows(const herro_job* job);
/* Alignments herro_job_create left out instead of failing the call: exactly what parse_paf itself drops before extract_features
 * sees it — self overlaps and a second alignment of a (query, target) pair (overlaps.rs:175-185).  Everything else the reference
 * processes is processed (consecutive insertion ops, an alignment starting inside window 0 with an insertion, any number of
 * overlaps per window); *n_targets is always 0 since round 3 (no target is dropped any more) and kept for the binding.
 * herro_last_error() describes the first alignment left out.  Inputs on which the reference panics make herro_job_create
 * return NULL with the reference's message.  Callers that feed alignments straight from parse_paf / herro_paf_parse never see a
 * non-zero count; herro_amd/shard.py treats one as an error. */
int herro_job_skipped(const herro_job* job, uint32_t* n_alignments, uint32_t* n_targets);

/* GPU feature generation for all windows of the job — features.rs:364-580 (filter, accuracy
 * ranking, max-insertion map, pileup scatter, informative positions, haplotype-ratio re-ranking,
 * top-30 selection, all-gap-row removal, token encoding inference.rs:222).  Asynchronous on the
 * context stream; the accessors below synchronise. */
int herro_job_featurize(herro_job* job);

/* Model forward over the job's windows with >=1 informative position, batched in submission
 * order in chunks of batch_size (prepare_examples/collate/inference, inference.rs:73-175,214-253).
 * batch_mode 0: batches never span reads (the reference's grouping, features.rs:884-893);
 * batch_mode 1: windows of different reads share batches (BASELINE batch=64/128 configs). */
int herro_job_infer(herro_job* job, uint32_t batch_size, int batch_mode);

/* Results (synchronise first).  Window order = (target order, wid). */
int herro_job_window_info(herro_job* job, uint32_t w, herro_window_info* info);
/* bases/quals: [length, 31] row-major as the reference emits them (features.rs:547-556);
 * bases are ASCII when encoded == 0, BASES_MAP tokens (inference.rs:23-31) when encoded != 0.
 * sup_pos/sup_ins: SupportedPos (features.rs:896-900); qids: ranked overlap read ids.
 * Any output pointer may be NULL. */
int herro_job_window_copy(herro_job* job, uint32_t w, int encoded, uint8_t* bases, uint8_t* quals,
                          uint16_t* sup_pos, uint8_t* sup_ins, uint32_t* qids);
/* Logits of window w after herro_job_infer: info[n_supported], bases[n_supported*5]. */
int herro_job_window_logits(herro_job* job, uint32_t w, float* info_logits, float* bases_logits);

/* Consensus on the device (consensus.rs:86-227): per window, the corrected bases (informative rows:
 * argmax of the base logits; other rows: majority vote with target tie-break; '*' dropped) are left in
 * HBM; herro_job_consensus_fasta then only concatenates windows.  Optional: without it the FASTA call
 * decodes on the host from the planes.  Requires herro_job_infer if any window has informative rows. */
int herro_job_consensus(herro_job* job);

/* After herro_job_consensus: copy the corrected bases of every window to the host (the only result traffic of the
 * corrected-reads path, ~4 KB per window) and return how many there are; herro_job_consensus_fasta then only assembles
 * text.  Optional (the FASTA call fetches on demand). */
int herro_job_consensus_fetch(herro_job* job, uint64_t* n_bases);

/* Consensus + FASTA text for target t (consensus.rs:86-227, lib.rs:282-317); id/desc are the
 * read's id and optional description (NULL: none).  Returns bytes written (0: read not
 * emitted), or a negative error.  Host-side integer decode of device results. */
int64_t herro_job_consensus_fasta(herro_job* job, uint32_t t, const char* id, const char* desc,
                                  char* out, uint64_t cap);

/* The FASTA records of ALL targets of the job in one call, target order (the consensus worker's output for a batch of
 * reads, consensus.rs:229-263 + lib.rs:282-317): ids[t] / descs[t] (descs or descs[t] NULL: none) as above.  Requires
 * herro_job_consensus.  out == NULL: returns the number of bytes the records take; otherwise writes them (at most cap
 * bytes) and returns the bytes written, or a negative error.  rec_end, if not NULL, receives for every target the end
 * offset of its records in out ([n_targets]; equal ends: the read was not emitted). */
int64_t herro_job_fasta(herro_job* job, const char* const* ids, const char* const* descs, char* out, uint64_t cap,
                        uint64_t* rec_end);

/* ---- stand-alone model entry (parity checks) — mirrors `inference` (inference.rs:147-175):
 * bases u8 tokens [B,L,31], quals raw u8 [B,L,31] (normalised on device, :153), lens [B],
 * indices flat [sum(lens)].  Outputs info_logits [N], bases_logits [N,5] (host). */
int herro_model_forward(herro_ctx* ctx, uint32_t B, uint32_t L, const uint8_t* bases,
                        const uint8_t* quals, const int32_t* lens, const int32_t* indices,
                        float* info_logits, float* bases_logits);

/* ---- measurement hooks (bench.py) -------------------------------------------------------- */
/* Per-kernel GPU time accumulated with HIP events on the context stream since the last reset.
 * names: '\n'-separated kernel-group names; ms/calls: arrays of n entries. */
int herro_timing_enable(herro_ctx* ctx, int on);
int herro_timing_reset(herro_ctx* ctx);
int herro_timing_get(herro_ctx* ctx, char* names, uint64_t names_cap, double* ms, uint64_t* calls,
                     uint32_t* n);
/* Algorithmic bytes of the job's featurisation (SURVEY.md §8 d formula), measured on the data:
 * out[0]=2-bit+qual bytes read, out[1]=cigar-op bytes, out[2]=model-ready bytes written,
 * out[3]=sum L', out[4]=sum n_supported, out[5]=windows with n_supported>0. */
int herro_job_stats(herro_job* job, uint64_t* out);

/* ---- host-only test hook: the library's windowing (windowing.rs:44-273 restated on binary ops)
 * for one alignment; needs no device.  out rows of 8 u64: window, tstart, qstart, qend, op_lo,
 * op_hi (op-index slice), cigar_start_offset, cigar_end_offset.  Returns row count or <0. */
int64_t herro_debug_extract_windows(const herro_alignment* a, uint32_t n_windows, uint32_t window_size,
                                    uint64_t* out, uint64_t cap, char* err, uint64_t err_cap);

/* Host-only test hooks for the host half of herro_job_create (CIGAR parsing, windowing, validation, descriptor
 * layout): herro_debug_host_ctx makes a context without a device from the read lengths (name_class may be NULL);
 * herro_job_create on it returns a job that holds the descriptors only (free it with herro_job_free, the context with
 * herro_destroy; no other call is valid on them); herro_debug_job_array exposes them: which = 0 binary ops (u32),
 * 1 overlap-window descriptors, 2 window descriptors (layouts: csrc/pileup_core.h), 3 / 4 tile -> window / first row,
 * 5 first window of every target.  Returns the element count (<0: error). */
herro_ctx* herro_debug_host_ctx(uint32_t n_reads, const uint32_t* read_len, const uint32_t* name_class);
int64_t herro_debug_job_array(herro_job* job, int which, const void** ptr, uint32_t* elem_bytes);

/* Test hooks for the two feature-generation paths.  herro_job_featurize runs the LEAN path by default (round 5): informative rows,
 * decoder votes and the model's receptive fields are derived from the column bit planes in position space and the [31][L'] token
 * planes (features.rs:547-556) are only built when somebody asks for them (herro_job_window_copy, the features writer, a model
 * whose receptive field exceeds 8 rows).  herro_debug_set_featurize_planes(ctx, 1) selects the planes path of rounds 3-4 for the
 * jobs featurized from then on (environment: HERRO_FEATURIZE_PLANES=1) — two independent derivations of the same results, compared
 * by tests/test_gpu_lean.py.  herro_debug_job_rf copies the 16-byte receptive-field records of window w (after herro_job_infer:
 * n_supported x 31 records, bytes 0..7 tokens / 8..15 qualities of rows sup_row - half .. ) and returns their number (<0: error). */
int herro_debug_set_featurize_planes(herro_ctx* ctx, int on);
/* Test hook for the two front ends of the f16 model (precisions 4 .. 8; csrc/model_h.hip): the conv stack and the FC projection as two kernels with the conv
 * output in HBM between them (k_conv_m, k_fc_r), or as one kernel that keeps it in LDS (k_conv_fc).  Both give the same bits.  mode -1 (default): chosen per
 * launch from the launch size (conv_fc_faster); 0: two kernels; 1: one kernel wherever the model's shapes allow it (another conv stack keeps its own path). */
int herro_debug_set_conv_fc(herro_ctx* ctx, int mode);
/* Test hooks for what the front end of a model launch decides from the launch's tokens and the compute units of the device (csrc/infer_plan.h, front_end_plan):
 * k_conv_fc or k_conv_m + k_fc_r, the grid of k_conv_m's stride loop (three workgroups per unit), the tile height of k_fc_r (64 .. 128 rows), and the grid of
 * k_conv_w for a conv stack the f16 kernels do not serve (two workgroups per unit).  herro_debug_set_front_cu: the front end plans for n_cu compute units from
 * now on (0: the device's own count), so that a launch of a few hundred tokens takes the kernels and loop trips of a large one; the encoder stack's tile plan
 * never sees the number.  herro_debug_front_last: out[5] = fused (1: k_conv_fc), FC tile rows, FC grid, conv grid, conv units (blocks of 16 pairs of k_conv_m,
 * tiles of k_conv_w) of the context's last model launch (all 0: a path that plans nothing from the compute units).  herro_debug_front_end_plan: the same five
 * numbers for each of the `count` launches of n_tok, n_tok + 1, ... tokens on n_cu units (out[count][5]), without a device; mode as herro_debug_set_conv_fc. */
int herro_debug_set_front_cu(herro_ctx* ctx, uint32_t n_cu);
int herro_debug_front_last(const herro_ctx* ctx, uint32_t* out);
int herro_debug_front_end_plan(uint32_t n_tok, uint32_t count, uint32_t n_cu, int mode, uint32_t* out);
/* Test hooks for the two ways a job's windows and descriptors are built (herro_job_create): on the device behind the CIGAR scan (csrc/build_dev.hip, the
 * default since round 6) or by the host from the scan's cut records (rounds 3-5; still what runs when the device meets anything it does not settle itself —
 * a text the scan kernel flags, an input the reference panics on — and what words the error).  herro_debug_set_host_build(ctx, 1) selects the host build for
 * the jobs created from then on; herro_debug_job_dev_built says which one built a job (for a job of
 * herro_job_create_aligned: 1 when its direct path built it, 0 when it went through the text of its ops).  tests/test_gpu_build_dev.py compares their descriptor arrays. */
int herro_debug_set_host_build(herro_ctx* ctx, int on);
int herro_debug_job_dev_built(const herro_job* job);
/* Host-only test hooks for the rules k_rows applies in position space (csrc/pileup_core.h): n count vectors counts[i][5] (A C G T * on a base row, the
 * target's base included; split[i][5] of them, or NULL, go through a second counter set that is merged in) with target[i] in 0..3 -> sup[i] (informative:
 * two symbols reach 3, features.rs:558,712) and vote[i] (consensus.rs:178-200; meaningful where sup[i] == 0); herro_debug_vote5: the vote on exact counts. */
int herro_debug_base_row_votes(const uint8_t* counts, const uint8_t* split, const uint8_t* target, uint32_t n, uint8_t* sup, uint8_t* vote);
uint32_t herro_debug_vote5(const uint32_t* c5, uint32_t tb);
int64_t herro_debug_job_rf(herro_job* job, uint32_t w, uint8_t* out, uint64_t cap);
/* The directory words of overlap-window `ow` (job order, herro_debug_job_array which = 1) as the featurize pass wrote them: one u32 per 32 window
 * positions, query index | insertion events in front << 20, 0xffffffff where either does not fit its field (csrc/job_dev.h, JobDev::cwd).  Read-only;
 * valid after herro_job_featurize for a slice the long-indel filter kept.  Returns the number of words (ceil(window_size / 32); <0: error). */
int64_t herro_debug_job_cwd(herro_job* job, uint32_t ow, uint32_t* out, uint64_t cap);
int herro_debug_job_rf_fused(const herro_job* job);  /* 1: the last herro_job_infer read records k_rows gathered itself; 0: k_rfq's */
int herro_debug_job_rf_left(const herro_job* job);    /* ... of which this many windows (above the 256 informative rows k_rows stages) were filled by k_rfq behind it, the others staying fused */
uint32_t herro_debug_e4m3(float x);                   /* host f32 -> OCP e4m3 (round to nearest even, saturating) as used for the precision-6 weight copies */
/* Host-only test hook of the model loader: reads `path` through herro_load_model's reader and packs the [N][K] tensor named `tensor` through its
 * packers; no device, no context.  form: 0 / 1 bf16 hi / lo in MFMA fragment order, 2 f16 hi in fragment order, 3 / 4 f16 hi / lo row-major,
 * 5 e4m3 in fragment order (*s8 = the E8M0 scale byte), 6 the conv1 GEMM matrix in fragment order (from t1 / wq1 / b1; tensor, K, N ignored).
 * Returns the bytes written to out (cap: its room), or a negative HERRO_E_* (NO_MODEL: malformed file, tensor missing or mis-sized). */
int64_t herro_debug_model_pack(const char* path, const char* tensor, uint32_t K, uint32_t N, int form, void* out, uint64_t cap, uint32_t* s8);
int herro_debug_sib_fault(herro_ctx* ctx);            /* raises the context's sibling-tile error word as a tile that timed out would: the next fetch repeats its job's model pass without sibling tiles */
int herro_debug_force_precision(herro_ctx* ctx, int on); /* tests: herro_set_precision / herro_load_model skip the calibration gate (to MEASURE a mode the model's calibration refuses) */
int herro_debug_sib_retries(const herro_ctx* ctx);    /* model passes repeated that way on this context */
/* tests: replaces the base logits of the job's informative rows (after herro_job_infer; n_rows must be all of them, job order, 5 floats each) on the device and
 * in the host copy, and drops the consensus: the next herro_job_consensus or herro_job_consensus_fasta decodes these */
int herro_debug_job_set_base_logits(herro_job* job, const float* base, uint64_t n_rows);

/* Host-only test hook for the token-tile plan of the fused transformer stack (herro_job_infer): n windows of cnt[i]
 * informative rows (1..64) -> order[k] = the window that is k-th in the launch's token stream; returns the number of
 * 64-token tiles of whole windows at the head of the stream.  packed bit 0: the best-fit-decreasing order herro_job_infer
 * uses (0: the given order); bits 1-2: 0 = 64-token tiles only; 1 = the f16 stack's default: when the last round of n_cu
 * tiles (one per compute unit) would be at most half full, its windows go into 32-token tiles instead (half the cost each);
 * 2 = every window of <= 32 rows in 32-token tiles, a window of 33..64 rows opens a 64-token tile and takes the best-fitting
 * small windows along.  *n_half (may be null) receives the number of 32-token tiles; tile_tok (capacity n + 1, may be null)
 * the first token of every tile, the 64-token ones first, then the end of the stream. */
int64_t herro_debug_tile_plan(const uint32_t* cnt, uint32_t n, int packed, uint32_t n_cu, uint32_t* order, uint32_t* n_half, uint32_t* tile_tok);
/* The same with windows above 64 informative rows admitted (cnt[i] in 1..512).  The f16 stack keeps such a window fused: on
 * ceil(rows / 64) consecutive 64-token tiles at the head of the stream — sibling tiles, which exchange the K / V fragments of
 * their heads layer by layer (inference.rs:134-141 takes any `lens`; windows above 512 rows run layer by layer).  The window's
 * last tile is filled up with the best-fitting small windows (packed plans only).  n_tiles[3] = sibling tiles, 64-token tiles,
 * 32-token tiles; tile_tok (capacity sum(ceil(cnt / 64)) + 2, may be null) the first token of every tile in stream order + end;
 * grp (capacity = the sibling tiles, may be null): first tile of the window's group | tiles in it << 20 | tokens of the window
 * in the group's last tile << 24.  The sibling tiles count as busy compute units when the last round is sized. */
int herro_debug_tile_plan_sib(const uint32_t* cnt, uint32_t n, int packed, uint32_t n_cu, uint32_t* order, uint32_t* n_tiles,
                              uint32_t* tile_tok, uint32_t* grp);
/* Host-only test hook for the whole launch plan of herro_job_infer (needs no context): a job of n_win windows with nsup[w] informative rows and L' = Lf[w],
 * tgt_win_off[n_targets + 1] the first window of each target.  batch_size / batch_mode as herro_job_infer takes them; fused != 0: a precision with a fused
 * stack, whose windows of more than fused_rows informative rows leave for a launch of their own; packed and n_cu as herro_debug_tile_plan.  Per window:
 * launch[w] = index of the launch that takes it (0xffffffff: no informative rows, it is in none), pos[w] = its position in that launch's window stream,
 * lmax[w] = the padding length it carries (the longest window of its batch).  Returns the number of launches. */
int64_t herro_debug_launch_plan(const uint32_t* nsup, const uint32_t* Lf, uint32_t n_win, const uint32_t* tgt_win_off, uint32_t n_targets, uint32_t batch_size,
                                int batch_mode, int fused, uint32_t fused_rows, int packed, uint32_t n_cu, uint32_t* launch, uint32_t* pos, uint32_t* lmax);

/* ---- PAF / .oec.zst ingest on the host (needs no device) ---------------------------------------
 * herro_paf_parse replaces `parse_paf` (overlaps.rs:117-202): one overlap per line, tab separated
 *   qname qlen qstart qend strand tname tlen tstart tend ... cg:Z:<CIGAR>   (CIGAR in the LAST column),
 * lines with unknown names, self overlaps and every (query, target) pair after its first occurrence are
 * dropped; the rest is grouped by target.  Quirks kept: the last byte of every line is dropped whether or
 * not it is a newline; numbers wrap in u32; malformed numbers / strand / CIGAR column are the reference's
 * panics (NULL is returned, `err` carries the message and the line).  `names` + `name_off[n_reads+1]` give
 * the read ids (index = read id of the read store; a repeated name maps to its last index, like the
 * reference's HashMap).  `core` (optional, one byte per read) replaces the `core` name set: targets with a 0
 * are skipped.  Targets come out in order of first appearance (the reference iterates a HashMap).
 * herro_oec_read replaces `read_batches` for one file (overlaps.rs:292-323): zstd stream holding
 * "<n_targets>\n", n_targets id lines (ignored, as in the reference), then PAF lines.
 * The result feeds herro_job_create directly: rids = herro_paf_target_ids, aln_off, alns.  The CIGAR
 * pointers stay valid until herro_paf_free. */
typedef struct herro_paf herro_paf;
/* The name -> read id index of a read set, built once (the reference's `name_to_id`, lib.rs:136-140) and shared by any number
 * of parses, also concurrent ones; herro_paf_parse / herro_oec_read build a temporary one per call (fine for one batch,
 * wasteful for a thousand batch files over millions of reads). */
typedef struct herro_name_index herro_name_index;
herro_name_index* herro_name_index_create(uint32_t n_reads, const char* names, const uint64_t* name_off);
void herro_name_index_free(herro_name_index* index);
herro_paf* herro_paf_parse_indexed(const char* text, uint64_t len, const herro_name_index* index, const uint8_t* core,
                                   int n_threads, char* err, uint64_t err_cap);
herro_paf* herro_oec_read_indexed(const char* path, const herro_name_index* index, const uint8_t* core, int n_threads,
                                  char* err, uint64_t err_cap);
/* herro_paf_parse_indexed without the copy: the result (its CIGAR pointers) refers to `text` itself — a buffer or file mapping
 * the caller keeps alive and unchanged until herro_paf_free. */
herro_paf* herro_paf_parse_view(const char* text, uint64_t len, const herro_name_index* index, const uint8_t* core,
                                int n_threads, char* err, uint64_t err_cap);
herro_paf* herro_paf_parse(const char* text, uint64_t len, uint32_t n_reads, const char* names,
                           const uint64_t* name_off, const uint8_t* core, int n_threads, char* err,
                           uint64_t err_cap);
herro_paf* herro_oec_read(const char* path, uint32_t n_reads, const char* names, const uint64_t* name_off,
                          const uint8_t* core, int n_threads, char* err, uint64_t err_cap);
/* PAF without CIGARs (`minimap2 -x ava-ont`, no -c: mm2.rs:15-30 then asks for -c): every rule of herro_paf_parse_indexed — self overlaps
 * and repeated (query, target) pairs dropped, grouping and order by first appearance, u32 wrap, the reference's messages on malformed
 * numbers or strand — but no CIGAR column is needed or read; the records carry cigar = NULL, cigar_len = 0 and go to herro_align_overlaps. */
herro_paf* herro_paf_parse_coords(const char* text, uint64_t len, const herro_name_index* index, const uint8_t* core, int n_threads,
                                  char* err, uint64_t err_cap);
uint32_t herro_paf_n_targets(const herro_paf* p);
const uint32_t* herro_paf_target_ids(const herro_paf* p);
const uint64_t* herro_paf_aln_off(const herro_paf* p);        /* [n_targets + 1] */
const herro_alignment* herro_paf_alignments(const herro_paf* p);
void herro_paf_free(herro_paf* p);

/* ---- base-level alignment on the device (csrc/align_dev.hip) ------------------------------------------------------------------
 * Stands in for the base-level step `herro inference` asks of minimap2 when it is not given --read-alns (`minimap2 -cx ava-ont`,
 * mm2.rs:15-30; the -c), followed by the reference's fix_cigar (aligners.rs:138-250): every record's query region is aligned to its
 * target region on the context's read store — banded Gotoh (+2 / -4, gaps 4 + 2k), HERRO_ALIGN_BAND cells per anti-diagonal, the
 * band following the better of its two edge cells — then indels are left-shifted and a leading and a trailing indel dropped, so
 * every CIGAR starts and ends with M.  The exact specification is DESIGN.md section 9.  A record fails (no CIGAR) when its end cell
 * leaves the band or nothing but indels would remain.  Runs on the context's execution stream and returns when done (threading as
 * herro_job_featurize).  Scratch: (n + m + 1) x 72 bytes per record, in chunks of HERRO_ALIGN_SCRATCH_MB (default 4096).
 * HERRO_E_STATE: no reads; HERRO_E_INVALID: a read id outside the store or coordinates outside a read (message names the record). */
#define HERRO_ALIGN_BAND 128
typedef struct herro_aligned herro_aligned;
/* Base-level alignment of n overlaps given by coordinates only (cigar / cigar_len ignored), on the context's read store. */
int herro_align_overlaps(herro_ctx* ctx, uint32_t n, const herro_alignment* in, herro_aligned** out);
/* n records in input order: coordinates after the trim; cigar points into the handle's text (cigar_len 0 = failed). */
const herro_alignment* herro_aligned_alignments(const herro_aligned* a);
const int32_t* herro_aligned_scores(const herro_aligned* a);   /* INT32_MIN for failed records */
uint32_t herro_aligned_failed(const herro_aligned* a);
void herro_aligned_free(herro_aligned* a);

/* ---- device-resident hand-off: aligner -> job builder without CIGAR text ---------------------------------
 * k_align's final ops and herro_job_create's op array use one encoding, `len << 2 | type` with type 0 M, 1 I, 2 D.
 * herro_align_overlaps_dev is herro_align_overlaps — same validation, chunking, error codes and messages, same coordinates, scores and
 * failed records — but every record's ops stay in a store on the device: behind each chunk the host reads the chunk's op total and its
 * per-record results, nothing else.  herro_job_create_aligned builds a job from records of such a handle: the binary sibling of the
 * CIGAR scan (k_ops_scan, csrc/cigar_dev.hip) reads the store where it is.  No text is printed, staged, uploaded or decoded. */
typedef struct herro_aligned_dev herro_aligned_dev;
int herro_align_overlaps_dev(herro_ctx* ctx, uint32_t n, const herro_alignment* in, herro_aligned_dev** out);
/* A handle over the caller's own binary CIGARs: record r has ops[op_off[r] .. op_off[r + 1]), each `len << 2 | type`; the coordinates
 * are taken as given; a record without ops counts as failed.  Also made on a device-free context (herro_debug_host_ctx), for the host
 * half of herro_job_create_aligned.  Ops herro_job_create would refuse as text (length 0, type 3) are refused by herro_job_create_aligned. */
int herro_aligned_dev_from_ops(herro_ctx* ctx, uint32_t n, const herro_alignment* alns, const uint64_t* op_off /* [n + 1] */,
                               const uint32_t* ops, herro_aligned_dev** out);
/* Every record of src and, behind them, its mirror — the alignment of the same two reads with query and target exchanged, derived from
 * the record's final ops on the device (k_mirror, csrc/align_dev.hip; DESIGN.md section 9, "Mirrored records") instead of a second
 * alignment: out holds 2n records, record r (r < n) is src's record r, record n + r its mirror.  The mirror's coordinates are src's with
 * the two reads swapped (same strand); its ops are src's with I and D exchanged, in reverse order on strand 1, normalised again by
 * fix_cigar against the swapped sequences (a dropped leading / trailing indel moves the coordinates as in herro_align_overlaps); its
 * score is src's score + g(src's ops) - g(its ops), g the sum of 4 + 2 len over the I / D ops — the score of its CIGAR when src's is
 * the score of src's; for a handle of herro_aligned_dev_from_ops, whose scores are 0, the field is just that difference.  A failed
 * source, a source with an op of type 3 and a mirror that is empty or does not start and end with M after the normalisation are failed
 * records: n_ops 0, score INT32_MIN, the swapped coordinates untrimmed.  A host pairs its records (record B is record A's exact swap)
 * and aligns one of each pair; two directions that differ must both be aligned.
 * The new handle owns its store (src's ops copied on the device, the mirrors' behind them): src may be freed; every accessor and
 * herro_job_create_aligned work on it unchanged.  HERRO_E_INVALID: a null argument, a handle of another context, a source record outside
 * the read store (named); HERRO_E_NO_DEVICE: a device-free context or handle; HERRO_E_STATE: no reads set.  n = 0: an empty handle. */
int herro_aligned_dev_mirror(herro_ctx* ctx, const herro_aligned_dev* src, herro_aligned_dev** out);
uint32_t herro_aligned_dev_n(const herro_aligned_dev* a);
const herro_alignment* herro_aligned_dev_alignments(const herro_aligned_dev* a);   /* trimmed coordinates; cigar = NULL, cigar_len = 0 */
const int32_t* herro_aligned_dev_scores(const herro_aligned_dev* a);               /* INT32_MIN: failed */
const uint32_t* herro_aligned_dev_n_ops(const herro_aligned_dev* a);               /* per record; 0: failed */
uint32_t herro_aligned_dev_failed(const herro_aligned_dev* a);
/* One record's CIGAR text on demand (one copy per call; herro_aligned_dev_paf below brings all of them down at once): returns its length in bytes — 0 for a failed record — and
 * writes it, without a terminator, when out != NULL and cap is large enough; < 0: HERRO_E_*. */
int64_t herro_aligned_dev_cigar(const herro_aligned_dev* a, uint32_t r, char* out, uint64_t cap);
/* Safe once herro_job_create_aligned has returned: the job owns a copy of its ops. */
void herro_aligned_dev_free(herro_aligned_dev* a);
/* The job herro_job_create builds from the same records, in the same order, with the texts herro_align_overlaps returns for them
 * (windows, descriptors, skipped counts and message, every later result; only the op array is denser: exactly n_ops slots per record).
 * Alignments of target t are records rec[aln_off[t] .. aln_off[t + 1]) of the handle.  HERRO_E_INVALID (herro_job_create_status), with
 * a message that names the record: a failed record, an index outside the handle, a handle of another context.  When the device build
 * is not taken or does not settle the job — herro_debug_set_host_build, HERRO_HOST_SCAN=1, anything the device flags, a device-free
 * context — the job's ops come down, are formatted and go through herro_job_create itself: results and error texts are the text
 * path's.  herro_debug_job_dev_built is 1 for a job the direct path built.  Threading as herro_job_create. */
herro_job* herro_job_create_aligned(herro_ctx* ctx, uint32_t n_targets, const uint32_t* rids, const uint64_t* aln_off,
                                    const uint32_t* rec, const herro_aligned_dev* a, uint32_t window_size);

/* ---- extension of overlaps to the read ends (k_extend, csrc/align_dev.hip) ------------------------------------------------------
 * The third piece of what `minimap2 -cx ava-ont` does for `herro inference` (mm2.rs:15-30) next to seeding / chaining
 * (herro_find_overlaps) and base-level alignment (herro_align_overlaps): a chain's anchor span stops short of where the reads stop
 * agreeing, and the reference's windowing only takes whole windows from an overlap, so a few missing bases cost a window of
 * coverage.  Every record is extended at both ends, each side on its own: the aligner's recurrence, scores and band (+2 / -4, gaps
 * 4 + 2k, HERRO_ALIGN_BAND cells per anti-diagonal) swept ends-free over the bases beyond the span — at most max_ext of either read —
 * ending at the best-scoring cell (the earliest anti-diagonal, then the smallest query length, among equals), which is always a
 * matching pair; the sweep stops once the two latest anti-diagonals lie more than zdrop (minimap2's -z) below the best, looked at
 * every 16 anti-diagonals.  The exact specification is DESIGN.md section 11 and tests/extend_ref.py, which the kernel equals bit for
 * bit.  What this is not: minimap2's extension — no end bonus (a span that stops a few bases short of a read end on an error is
 * not pulled to the end), no two-piece gaps.  The two records of a pair are extended independently and need not mirror each other.
 * Parameters: a 0 field means its default — zdrop 400, max_ext 2048; max_ext above 2^20 is HERRO_E_INVALID (checked before anything
 * else).  Validation, codes and messages otherwise as herro_align_overlaps: HERRO_E_STATE without reads, HERRO_E_INVALID naming the
 * record, HERRO_E_NO_DEVICE on a context without a device.  Runs on the context's execution stream and returns when done; no
 * scratch memory. */
typedef struct { uint32_t zdrop, max_ext, reserved[2]; } herro_extend_params;
typedef struct herro_extended herro_extended;
int herro_extend_overlaps(herro_ctx* ctx, uint32_t n, const herro_alignment* in, const herro_extend_params* params /* NULL: defaults */,
                          herro_extended** out);
uint32_t herro_extended_n(const herro_extended* x);
/* n records in input order with the extended coordinates, cigar = NULL, cigar_len = 0: ready for herro_align_overlaps[_dev]. */
const herro_alignment* herro_extended_alignments(const herro_extended* x);
/* uint32 [n][4]: bases gained as t_left, q_left, t_right, q_right; the q lengths on the oriented query (strand 1: q_left is added
 * to qend, q_right taken from qstart). */
const uint32_t* herro_extended_ext(const herro_extended* x);
const int32_t* herro_extended_scores(const herro_extended* x);   /* int32 [n][2]: the left and the right side's score */
void herro_extended_free(herro_extended* x);

/* ---- overlap finding on the device (csrc/overlap_dev.hip) ------------------------------------------------------------------------
 * Stands in for the seeding and chaining half of the `minimap2 -x ava-ont` run `herro inference` starts itself without --read-alns
 * (AlnMode::None, overlaps.rs:340-344 -> generate_batches -> call_mm2, mm2.rs:15-30): which reads of the context's store overlap,
 * where, on which strand.  Not minimap2's output (no two-piece gaps, no z-drop extension, no secondary chains) but
 * a small specification of its own, DESIGN.md section 10 and tests/overlap_ref.py, which the kernels equal bit for bit: (k, w)
 * minimizers under minimap2's hash64 with every tied window minimum selected; hashes with more occurrences in the store than the
 * frequency cut dropped (max_occ, or a fraction of the distinct hashes: below); anchors between every two occurrences in different reads; per (t, q, strand) a chain over the 64 nearest
 * predecessors (gaps <= max_gap, diagonal drift <= bandwidth, minimap2's one-piece gap cost); kept with score >= min_score and
 * >= min_anchors anchors.  Coordinates are the anchor span of the chain: the finder itself does not extend it to the read ends —
 * herro_extend_overlaps (above) does, as a step of its own between this call and herro_align_overlaps.  One overlap per
 * read pair (overlaps.rs:181-185; the better strand, forward on a tie), no self overlaps (overlaps.rs:175-179), and every pair
 * yields two records, (t, q) and (q, t) — minimap2's --dual=yes.  Records come grouped by target in ascending read id, each
 * target's records in ascending qid, with cigar = NULL and cigar_len = 0: the shape herro_paf_parse_coords produces, so they go into
 * herro_align_overlaps unchanged.
 * Parameters: a 0 field means its default — k 25, w 17, bandwidth 150, min_score 2500 (the -k -w -r -m of mm2.rs:22-26), max_gap
 * 5000, min_anchors 3 (minimap2's -g, -n), max_occ 128.  5 <= k <= 31 and 1 <= w <= 64, else HERRO_E_INVALID (checked before
 * anything else).  min_score 2500 is a threshold for reads of ~10 kb and more; short reads need their own.  A fixed max_occ must stay
 * above the read depth: a true minimizer occurs once per read that covers it, and a cut below the depth removes the anchors of true
 * overlaps.
 * occ_frac_ppm (0: off, the fixed cut max_occ) takes the cut from the store's own index instead, as minimap2's -f does (mm2.rs:27 runs
 * -f0.005 = 5000): parts per million of the DISTINCT minimizer hashes that may lie above it.  With D distinct hashes (singletons included)
 * and c' = min(occurrences, 65535) per hash: drop = floor(D * ppm / 10^6); q = the least v with at most drop hashes of c' > v (the
 * (D - drop)-th smallest c'; every hash tied with it is kept); cut = max(q, 10), then min(cut, max_occ) if max_occ is not 0 — in this mode
 * max_occ is a ceiling and 0 means none, not 128 —, then min(cut, 65534): a hash of 65535 or more occurrences is never used.  A hash is
 * used iff it occurs 2 .. cut times.  1 <= occ_frac_ppm <= 999999, else HERRO_E_INVALID (checked with k and w).  The cut is that of the
 * whole store whatever the core mask and the scratch budget; herro_overlaps_occ_cut / herro_pairs_occ_cut return it (max_occ in the
 * fixed mode; 0 for a handle made by herro_pairs_from_table*), and HERRO_OVL_STATS=1 adds a line `OVLOCC cut= distinct= cut_runs=
 * cut_minimizers=` to its `OVL ` line.  Known limit: the chain looks back 64 ANCHORS, not bases — a tandem repeat that survives max_occ (a set of very few
 * reads) can put more than 64 off-diagonal anchors between two anchors of the true diagonal, and the overlap comes out shorter.
 * Limits (HERRO_E_UNSUPPORTED): 2^31 - 1 reads, reads of 2^31 - 1 bases, 2^32 k-mers in the store (with herro_set_index_params: in one
 * pair of read blocks), 2^32 anchors per target.
 * Scratch: 128 bytes per anchor, targets processed in read-id ranges that fit HERRO_OVL_SCRATCH_MB (default 4096; a target that
 * needs more runs alone) — the result is byte-identical for every budget — plus 40 bytes per minimizer of the store (60 with the rescue).
 * With herro_set_index_params, in place of the latter: 2 bytes per minimizer of the store (occ16), 8 bytes per 256 k-mers of the store (two
 * per-tile tables) and 4 per read, and beside them the arrays of ONE part at a time — 79 bytes per minimizer of a pair of read blocks (70
 * without the rescue), or 44 per minimizer of a hash range of the occurrence pass —, each with its sort histograms (1 KiB per 2048 elements).
 * Runs on the context's execution stream and returns when done.  HERRO_E_STATE: no reads; HERRO_E_NO_DEVICE: a context without
 * a device. */
typedef struct { uint32_t k, w, max_occ, bandwidth, max_gap, min_score, min_anchors, occ_frac_ppm; } herro_overlap_params;
typedef struct herro_overlaps herro_overlaps;
int herro_find_overlaps(herro_ctx* ctx, const herro_overlap_params* params /* NULL: defaults */, herro_overlaps** out);
uint32_t herro_overlaps_n(const herro_overlaps* o);                       /* records (two per pair) */
uint32_t herro_overlaps_n_targets(const herro_overlaps* o);
const uint32_t* herro_overlaps_target_ids(const herro_overlaps* o);
const uint64_t* herro_overlaps_aln_off(const herro_overlaps* o);          /* [n_targets + 1] */
const herro_alignment* herro_overlaps_alignments(const herro_overlaps* o);
const int32_t* herro_overlaps_scores(const herro_overlaps* o);            /* chain score per record */
uint32_t herro_overlaps_occ_cut(const herro_overlaps* o);                 /* the frequency cut the call used */
void herro_overlaps_free(herro_overlaps* o);
/* ---- pair overlaps: reads -> one record per read pair -> mirrored alignments -> job, in three calls ----------------------------------
 * herro_find_overlaps writes both directions of every pair; aligning each pair once and mirroring the alignment (herro_aligned_dev_mirror)
 * needs them paired again, and the extension between the two must see one direction only.  These entries keep that bookkeeping in the
 * library and the records on the device from the chains to the extension: the strand choice, the compaction of the chosen chains into
 * primaries, the table of the 2 P rows (sorted by target and query on the device) and the extension's side descriptors and fold are
 * kernels (csrc/overlap_dev.hip, csrc/align_dev.hip; DESIGN.md section 10, "Pairs on the device"); the host reads counts and, once, the
 * finished primaries and the table.
 * Specification: for the same reads and parameters the handle equals, field for field, what the stepwise chain gives —
 * herro_find_overlaps; its rows paired (row B is row A's exact swap; the first of the two is the primary: api.pair_rows of the Python
 * binding); herro_extend_overlaps over the primaries; the table of api.paired_job_args.  That is: P primaries in ascending (tid, qid)
 * with tid < qid, extended unless HERRO_PAIRS_NO_EXTEND; their chain scores; the extension's ext and scores (zeros with the flag); and
 * the finder's 2 P rows as target_ids / aln_off (grouped by target, ascending tid then qid) with rec_of_row[i] = p for the row that is
 * primary p and P + p for the row that is its mirror — the record indices of the handle herro_pairs_align returns.
 * herro_find_overlap_pairs: parameters as herro_find_overlaps and herro_extend_overlaps (NULL: defaults), checked first, then
 * HERRO_E_NO_DEVICE on a device-free context, then HERRO_E_STATE without reads; HERRO_E_UNSUPPORTED: the finder's limits and more than
 * 2^31 - 1 pairs.  Scratch and chunking as herro_find_overlaps (HERRO_OVL_SCRATCH_MB; the same bytes for every budget).
 * herro_pairs_from_table: a handle over a table the host built itself; works on a device-free context, as herro_aligned_dev_from_ops
 * does.  HERRO_E_INVALID naming the offending index: a primary that fails the record checks of herro_align_overlaps, an aln_off that does
 * not ascend from 0 to 2 P, a rec_of_row that does not hold every value of 0 .. 2 P - 1 once.  chain_scores may be NULL (zeros).
 * herro_pairs_align: herro_align_overlaps_dev over the primaries, then herro_aligned_dev_mirror — their codes and messages; out holds
 * 2 P records, primaries then mirrors.  HERRO_E_INVALID: a handle of another context.
 * herro_job_create_paired: herro_job_create_aligned over the table with every row whose record failed (no ops) dropped; a target all of
 * whose rows failed keeps its place.  m must hold exactly 2 P records and belong, like the pairs, to ctx: else NULL and HERRO_E_INVALID
 * through herro_job_create_status.  Everything else as herro_job_create_aligned.  Handles may be freed once the job exists. */
typedef struct herro_pairs herro_pairs;
#define HERRO_PAIRS_NO_EXTEND 1u
int herro_find_overlap_pairs(herro_ctx* ctx, const herro_overlap_params* params /* NULL: defaults */,
                             const herro_extend_params* extend_params /* NULL: defaults */, uint32_t flags, herro_pairs** out);
int herro_pairs_from_table(herro_ctx* ctx, uint32_t n_pairs, const herro_alignment* primaries, const int32_t* chain_scores, uint32_t n_targets,
                           const uint32_t* rids, const uint64_t* aln_off /* [n_targets + 1] */, const uint32_t* rec_of_row /* [2 n_pairs] */,
                           herro_pairs** out);
int herro_pairs_align(herro_ctx* ctx, const herro_pairs* pairs, herro_aligned_dev** out);
herro_job* herro_job_create_paired(herro_ctx* ctx, const herro_pairs* pairs, const herro_aligned_dev* m, uint32_t window_size);
uint32_t herro_pairs_n(const herro_pairs* pairs);                          /* P */
const herro_alignment* herro_pairs_primaries(const herro_pairs* pairs);    /* [P]; cigar = NULL, cigar_len = 0 */
const int32_t* herro_pairs_chain_scores(const herro_pairs* pairs);         /* [P] */
const uint32_t* herro_pairs_ext(const herro_pairs* pairs);                 /* [P][4]: t_left, q_left, t_right, q_right as herro_extended_ext */
const int32_t* herro_pairs_ext_scores(const herro_pairs* pairs);           /* [P][2]: left, right */
uint32_t herro_pairs_n_targets(const herro_pairs* pairs);
const uint32_t* herro_pairs_target_ids(const herro_pairs* pairs);          /* [n_targets] */
const uint64_t* herro_pairs_aln_off(const herro_pairs* pairs);             /* [n_targets + 1] */
const uint32_t* herro_pairs_rec_of_row(const herro_pairs* pairs);          /* [2 P]; [herro_pairs_n_rows] of a core handle */
void herro_pairs_free(herro_pairs* pairs);
/* ---- a core set of targets: overlaps found and aligned for the core reads only ---------------------------------------------------------
 * The PAF entries take `core` (one byte per read; overlaps.rs:154-159 drops the targets outside it, as `-c cluster` does: lib.rs:132-133,
 * haec_io.rs:62-68 — a store of a core set plus its neighbours).  These entries take the same mask for the device front end, so that N
 * ranks which hold the read store and correct 1/N of the reads each do not each chain, extend, align and mirror every pair of the store.
 * core: n_reads bytes, non-zero = the read is core, i.e. a target; NULL = every read is core, and exactly the entry without `_core`.
 *   A read pair is wanted iff at least one of its two reads is core; a row (target, query) is wanted iff its target is core.
 * The finder creates no anchor between two non-core reads (k_runs, k_expand in csrc/overlap_dev.hip), so the sorts, the groups, the
 * chains, the strand choice, the extension, the aligner and the mirror see wanted pairs only.  Chains are independent per (t, q, strand)
 * and the frequency cut (max_occ or occ_frac_ppm's) stays that of the whole store's index, so the result is a selection of the unmasked one.  With F the handle
 * herro_find_overlap_pairs returns for the same reads and parameters:
 *   primaries   those of F with core[tid] | core[qid], in F's order; chain_scores, ext and ext_scores the same selection; P' of them.
 *   rows        F's rows whose target is core, in F's order: target_ids is F's targets that are core, aln_off counts the kept rows,
 *               herro_pairs_n_rows = R' = sum over the kept primaries of core[tid] + core[qid] <= 2 P'.
 *   rec_of_row  the new index of its primary for a primary row, P' + that index for a mirror row.
 * herro_pairs_align is unchanged: 2 P' records, primaries then mirrors (the mirror kernel is ~1.5 % of the aligner: selecting mirrors is
 * not worth a second layout).  herro_job_create_paired wants 2 P' records in m, whatever the number of rows.
 * herro_find_overlaps_core: herro_find_overlaps' records whose tid is core, same order, same scores.
 * The `anchors` figure of HERRO_OVL_STATS=1 and the limits (2^32 anchors per target or chunk, 2^31 - 1 pairs) count the masked anchors
 * and pairs; chunking by HERRO_OVL_SCRATCH_MB stays byte-neutral.  Checks, codes and messages are those of the entries without `_core`.
 * herro_pairs_from_table_core: herro_pairs_from_table for a table of n_rows <= 2 P rows; works on a device-free context.  HERRO_E_INVALID
 * naming the index: aln_off does not ascend from 0 to n_rows, a rec_of_row value is >= 2 P or occurs twice; also n_rows > 2 P.
 * herro_pairs_from_table keeps its stricter rule (every record in exactly one row).
 * herro_pairs_n_rows: the rows of the table = entries of rec_of_row; 2 P for every handle made without a mask. */
int herro_find_overlaps_core(herro_ctx* ctx, const herro_overlap_params* params /* NULL: defaults */, const uint8_t* core /* [n_reads] or NULL */,
                             herro_overlaps** out);
int herro_find_overlap_pairs_core(herro_ctx* ctx, const herro_overlap_params* params /* NULL: defaults */,
                                  const herro_extend_params* extend_params /* NULL: defaults */, uint32_t flags,
                                  const uint8_t* core /* [n_reads] or NULL */, herro_pairs** out);
int herro_pairs_from_table_core(herro_ctx* ctx, uint32_t n_pairs, const herro_alignment* primaries, const int32_t* chain_scores, uint32_t n_targets,
                                const uint32_t* rids, const uint64_t* aln_off /* [n_targets + 1] */, uint64_t n_rows,
                                const uint32_t* rec_of_row /* [n_rows] */, herro_pairs** out);
uint64_t herro_pairs_n_rows(const herro_pairs* pairs);
uint32_t herro_pairs_occ_cut(const herro_pairs* pairs);                    /* the frequency cut the finder used; 0: a handle over a table */

/* ---- rescue of high-frequency minimizers (minimap2's -e, the reference's -e200: mm2.rs:24) ---------------------
 * Without it every hash above the frequency cut is dropped, so a read that lies inside a high-copy repeat gets no anchor at all.  With it,
 * of a stretch of a read whose minimizers all lie above the cut the least frequent ones stay, about one per occ_dist bases.  The rule is the
 * finder's own (tests/rescue_ref.py), all integer and independent of thread order; it does not reproduce minimap2's choice of seeds.
 *   occ(x) = occurrences of x's hash in the whole store; cut = the frequency cut the call uses anyway (max_occ or occ_frac_ppm's).
 *   x is U if 2 <= occ <= cut, H if cut < occ <= rescue_max_occ, transparent otherwise (singletons and hashes above rescue_max_occ
 *   neither end a streak nor are rescued).  Per read, over its U and H minimizers in ascending pos, a streak is a maximal run of H; ps = the
 *   pos of the U in front of it (0: none), pe = the pos of the U behind it (the read's length: none), m = (2 (pe - ps) + occ_dist) /
 *   (2 occ_dist).  The m members with the least (occ, pos) are rescued — all of them if m >= the streak's size.
 *   Two occurrences of one hash in reads t < q give an anchor iff 2 <= occ <= cut, or cut < occ <= rescue_max_occ and one of the two is
 *   rescued.  The core rule is applied on top; the selection itself sees neither the mask nor the scratch budget, so a masked result is a
 *   selection of the unmasked one and the bytes are the same for every HERRO_OVL_SCRATCH_MB.
 * herro_overlap_params has no spare field, so the switch is a setting of the context, as herro_set_precision is: it holds for every later
 * herro_find_overlaps[_core] and herro_find_overlap_pairs[_core].  params NULL or occ_dist 0: off — every call returns what it returned before
 * the setting existed and launches none of the rescue's kernels.  rescue_max_occ 0 = 4095.  occ_dist > 2^20, rescue_max_occ > 65534 or a
 * non-zero reserved field: HERRO_E_INVALID (checked here; works on a context without a device).  herro_overlaps_rescued / herro_pairs_rescued:
 * the minimizers the call rescued (0: off, or a handle made by herro_pairs_from_table*).  HERRO_OVL_STATS=1 adds a line `OVLRESC high=
 * rescued= anchors=`: the H minimizers, the rescued ones, the anchors of the hashes above the cut.  Known interaction: rescued hashes inside a
 * tandem repeat add off-diagonal anchors, and the 64-anchor look-back limit above applies to them too (herro_set_chain_params lifts it to
 * 1024). */
typedef struct { uint32_t occ_dist, rescue_max_occ, reserved[2]; } herro_seed_rescue_params;
int herro_set_seed_rescue(herro_ctx* ctx, const herro_seed_rescue_params* params /* NULL: off */);
uint32_t herro_overlaps_rescued(const herro_overlaps* o);
uint32_t herro_pairs_rescued(const herro_pairs* pairs);

/* ---- a longer chain look-back ("A longer look-back"; minimap2's max_chain_iter, 5000 there) -------------------------
 * A chain step looks at the 64 nearest predecessors of an anchor.  Where a tandem repeat survives the frequency cut — a cut taken from the
 * index (occ_frac_ppm) or the rescue above keeps its minimizers on purpose — more than 64 off-diagonal anchors can lie between two anchors of
 * the true diagonal: the chain breaks there and the overlap comes out short, silently.  lookback = H, a multiple of 64 in 64 .. 1024, makes every
 * later herro_find_overlaps[_core] and herro_find_overlap_pairs[_core] of the context chain over the H nearest predecessors instead.  The
 * specification is otherwise unchanged (tests/overlap_ref.py::chain(..., lookback=H)): the same conditions and cost, the nearest predecessor
 * wins ties, the chain ends at the smallest anchor that holds the maximum; the records equal the reference's bit for bit and are the same
 * bytes for every HERRO_OVL_SCRATCH_MB.  params NULL or lookback 0: 64, the default, which runs exactly the kernels that ran before the setting
 * existed; any other H runs k_chain_far, whose cost per anchor grows with H where predecessors lie within max_gap.  A look-back that is no
 * multiple of 64 in 64 .. 1024, or a non-zero reserved field: HERRO_E_INVALID with the legal values in the message, and the setting stays as it
 * was (checked here; works on a context without a device).  HERRO_OVL_STATS=1 adds a line `OVLCHAIN lookback= chained=` when H is not 64.
 * What remains: an array with more than 1024 anchors between diagonal neighbours still breaks the chain. */
typedef struct { uint32_t lookback, reserved[3]; } herro_chain_params;   /* lookback 0 = 64; reserved: 0 */
int herro_set_chain_params(herro_ctx* ctx, const herro_chain_params* params /* NULL: defaults */);

/* ---- an index in parts ("An index in parts"; minimap2's -I, the reference's 50 000-read target batches) ---------------
 * The finder's index arrays are 32-bit indexed and sized by the minimizers of the whole store: a store of more than 2^32 - 4096 k-mers is
 * HERRO_E_UNSUPPORTED, and well below that the index no longer fits beside the store.  max_kmers != 0 makes every later
 * herro_find_overlaps[_core] and herro_find_overlap_pairs[_core] of the context build its index in parts of at most max_kmers k-mers; the records,
 * the cut and the rescue's figures are byte for byte those of the unpartitioned call, for every max_kmers, occ_ranges, option and scratch budget
 * (tests/index_parts_ref.py).  Two facts carry it: the whole store enters the specification only through occ(hash), the occurrences of a
 * minimizer's hash in the store, and chains are independent per (t, q, strand).
 *   pass A   occ16 = min(occ, 65535) of every minimizer of the store, by hash range: the 2k-bit hash space is cut into occ_ranges equal ranges
 *            (0: as many as keep a range near the minimizers max_kmers k-mers give, a range that still overflows is halved), the minimizers of a
 *            range are sorted by hash, and a run's length is the store's occ, since a run lies in one range.  The census of occ_frac_ppm is taken
 *            here, in 64-bit bins.  A forced occ_ranges one of whose ranges holds more than 2^32 - 4096 minimizers: HERRO_E_UNSUPPORTED.
 *   blocks   nk[r] = len[r] - k + 1 if len[r] >= k + w - 1, else 0; cap = max(max_kmers / 2, 1); reads in ascending id, acc = 0: a new block
 *            opens in front of read r iff nk[r] > 0, acc > 0 and acc + nk[r] > cap (acc restarts at 0), then acc += nk[r].  A read of more
 *            than cap k-mers is a block alone, reads without k-mers never open one, a non-empty store has at least one block.
 *   pass B   the block pairs (i, j), i <= j, ascending: the minimizers of the two blocks with their occ16, sorted by hash.  A hash is used iff
 *            2 <= occ <= cut — occ, not its occurrences in the pair —, the rescue's classes are taken from occ likewise; for i < j an anchor
 *            (t, q) exists iff t lies in block i and q in block j, for i = j iff t < q.  Chunks, sorts, chains and the strand pick are those of
 *            the unpartitioned call; the records of all pairs are put into target order by one stable sort.  A pair of two blocks without a
 *            core read is skipped.  Two blocks of more than 2^32 - 4096 k-mers together (only reads longer than cap): HERRO_E_UNSUPPORTED,
 *            naming the first read of each.
 * The cost: a block is sketched and sorted again for every pair it is in.  params NULL or max_kmers 0: off, the default — the calls launch exactly
 * the kernels they launched before the setting existed and keep their limits.  max_kmers > 2^32 - 4096, occ_ranges > 65536 or a non-zero reserved
 * field: HERRO_E_INVALID, and the setting stays as it was (checked here; works on a context without a device).  HERRO_OVL_STATS=1 adds a line
 * `OVLPART blocks= pairs= ranges= peak_bytes=` — the read blocks, the block pairs run, the hash ranges run, the most device scratch the finder held
 * at once —; the other lines' figures are the sums over the parts and equal the unpartitioned call's, `chunks` excepted.
 * herro_overlaps_index_blocks / herro_pairs_index_blocks: the read blocks of the call; 0: the setting was off (or a handle over a table).
 * herro_index_plan: the block rule alone (csrc/index_plan.h: host code, also on a context without a device) — writes the n_blocks + 1 cuts,
 * ascending read ids from 0 to n_reads, where cuts is not NULL and cap holds them, and returns n_blocks (0: an empty store).  HERRO_E_INVALID:
 * k, w or max_kmers out of range (max_kmers 0 is max_kmers 1); HERRO_E_UNSUPPORTED: two blocks exceed 2^32 - 4096 k-mers together. */
typedef struct { uint64_t max_kmers; uint32_t occ_ranges, reserved; } herro_index_params;
int herro_set_index_params(herro_ctx* ctx, const herro_index_params* params /* NULL or max_kmers 0: off */);
uint32_t herro_overlaps_index_blocks(const herro_overlaps* o);   /* 0: the setting was off */
uint32_t herro_pairs_index_blocks(const herro_pairs* pairs);     /* 0: off, or a handle over a table */
int64_t herro_index_plan(herro_ctx* ctx, uint64_t n_reads, const uint32_t* read_len, uint32_t k, uint32_t w, uint64_t max_kmers, uint64_t* cuts,
                         uint64_t cap);

/* ---- found alignments as PAF / .oec.zst --------------------------------------------------------------------
 * What `herro inference --write-alns DIR` keeps of a batch (AlnMode::Write, overlaps.rs:248-286; the lines, 349-352), for the alignments this
 * library found itself: herro_oec_read / herro_paf_parse* read the result back, and so does the reference's --read-alns.  One line per row,
 *   qname qlen qstart qend +|- tname tlen tstart tend mbases blocklen 255 cg:Z:<cigar>
 * tab separated, closed by a newline: the nine coordinate fields are the record's herro_aligned_dev_alignments entry (trimmed), decimal;
 * <cigar> is byte for byte what herro_aligned_dev_cigar returns ('?' for type 3 of a caller's own ops); a record without ops (failed) gives NO
 * line.  mbases is the sum of the record's M op lengths and blocklen the sum of all its op lengths (64 bits) — NOT minimap2's residue matches
 * and alignment block length; the reference reads nine fields and the last one (overlaps.rs:135-172) and ignores columns 10 to 12.
 * names / name_off[n_reads + 1]: the read names as herro_name_index_create takes them, index = read id.  An empty name or one with a tab or a
 * newline is HERRO_E_INVALID naming the read, checked before anything else.
 * On a device handle the text is formed on the GPU (k_paf_len, k_paf_write) in chunks that fit HERRO_PAF_SCRATCH_MB of device memory (MiB,
 * default 1024; the same bytes for every budget) and comes down through two pinned buffers; HERRO_PAF_STATS=1 prints `PAF rows= lines= bytes=
 * chunks=` on stderr.  On a handle of a device-free context the same lines come from the host formatter: the specification of the kernels.
 * HERRO_E_INVALID: a null argument, a handle of another context, rec[i] >= the handle's records (names i), an aligned handle that does not
 * hold exactly 2 P records (pair entries), a bad name, a row whose qid or tid is outside the read store, an unknown flag; HERRO_E_STATE: no
 * reads set; HERRO_E_UNSUPPORTED: more than 2^31 - 1 rows, a line of 2^32 bytes or more, HERRO_ALNS_OEC without libzstd.so.1.  The file entry
 * also answers HERRO_E_INVALID when the file cannot be created, written or renamed or the compressor reports an error (a full disk as much as a
 * bad path): the message begins "herro_pairs_write_alns: cannot create / cannot write / cannot rename / zstd:" and tells them apart.  An error
 * leaves no handle and no file.  n_rows = 0: an empty text. */
typedef struct herro_paf_text herro_paf_text;
/* rows: n_rows record indices of `a` in output order (NULL: row i is record i, n_rows of them) */
int herro_aligned_dev_paf(herro_ctx* ctx, const herro_aligned_dev* a, uint64_t n_rows, const uint32_t* rec, const char* names,
                          const uint64_t* name_off /* [n_reads + 1] */, herro_paf_text** out);
/* the rows of the table in its order (target ascending, query ascending), rec = rec_of_row: exactly the alignments herro_job_create_paired
 * builds its job from */
int herro_pairs_paf(herro_ctx* ctx, const herro_pairs* pairs, const herro_aligned_dev* m, const char* names,
                    const uint64_t* name_off /* [n_reads + 1] */, herro_paf_text** out);
const char* herro_paf_text_data(const herro_paf_text* text);   /* herro_paf_text_len bytes, no terminator promised */
uint64_t herro_paf_text_len(const herro_paf_text* text);
uint64_t herro_paf_text_lines(const herro_paf_text* text);
void herro_paf_text_free(herro_paf_text* text);
/* The same lines streamed to a file chunk by chunk (the whole text is never resident): written to path + ".tmp" and renamed.  Without a flag
 * plain PAF; HERRO_ALNS_OEC: the reference's batch file (overlaps.rs:270-282) — ONE zstd frame at level 0 (through libzstd.so.1, loaded as the
 * reader loads it) holding "<n_targets>" and a newline, the name of every target of the table and a newline each, then the lines.  The frame is
 * decodable by any zstd; it is not byte-equal to the reference encoder's.  lines / bytes (NULL: not wanted): lines written, bytes of the file. */
#define HERRO_ALNS_OEC 1u
int herro_pairs_write_alns(herro_ctx* ctx, const herro_pairs* pairs, const herro_aligned_dev* m, const char* names,
                           const uint64_t* name_off /* [n_reads + 1] */, const char* path, uint32_t flags, uint64_t* lines, uint64_t* bytes);

/* Test hook: the census and the pick of occ_frac_ppm alone (occ_frac_ppm 0: HERRO_E_INVALID).  hist: the 65536 bins of min(occurrences,
 * 65535) over the distinct hashes; out = {cut, distinct hashes, hashes above the cut, minimizers in them}. */
int herro_debug_occ_census(herro_ctx* ctx, const herro_overlap_params* params, uint32_t* hist /* [65536] or NULL */, uint64_t out[4]);
/* Test hook: the rescue alone, under the context's herro_set_seed_rescue setting (off: no flag is set).  For the minimizers in
 * herro_debug_sketch's (rid, pos) order: occ = min(occurrences of the hash in the store, 65535), rescued = 1 where the minimizer is rescued.
 * Returns their number (nothing is written when cap is smaller) or a negative error. */
int64_t herro_debug_seed_rescue(herro_ctx* ctx, const herro_overlap_params* params, uint32_t* occ, uint8_t* rescued, uint64_t cap);
/* Test hook: the chain stage alone, on anchor groups the caller gives, under the context's herro_set_chain_params setting.  Group g is
 * tpos / qpos [group_off[g], group_off[g + 1]): not empty, strictly ascending by (tpos, qpos) — what the finder's sort leaves —, coordinates
 * below 2^31.  Runs exactly what a finder call runs behind its groups: they are ordered largest first, chained by k_chain (look-back 64) or
 * k_chain_far, and walked back by k_walk.  Of params it reads k, bandwidth and max_gap (0 / NULL: the defaults).  out[g] = {score, first anchor,
 * last anchor, anchors in the chain}, the anchors as indices into their group: tests/overlap_ref.py::chain.  HERRO_E_INVALID for a null
 * argument, group_off[0] != 0, or a group that is empty, not ascending or holds a coordinate >= 2^31 (the message names the first such group);
 * HERRO_E_UNSUPPORTED for 2^31 groups or anchors or more; then HERRO_E_NO_DEVICE on a context without a device.  No reads are needed. */
int herro_debug_chain(herro_ctx* ctx, uint64_t n_groups, const uint64_t* group_off /* [n_groups + 1] */, const uint32_t* tpos,
                      const uint32_t* qpos, const herro_overlap_params* params, int32_t* out /* [n_groups][4] */);
/* Test hook: stage 1 alone — the store's minimizers sorted by (rid, pos); pos = index of the k-mer's last base on the forward
 * read, strand = 1 when the reverse complement is the canonical k-mer.  Returns their number (nothing is written when cap is
 * smaller) or a negative error. */
int64_t herro_debug_sketch(herro_ctx* ctx, const herro_overlap_params* params, uint64_t* hash, uint32_t* rid, uint32_t* pos,
                           uint8_t* strand, uint64_t cap);

/* ---- reads and the `herro features` sink -----------------------------------------------------
 * herro_fastx_read = get_reads (haec_io.rs:37-75) over needletail's parse_fastx_file: FASTA or FASTQ by the first byte,
 * gzip by magic, multi-line records, '\r' dropped; records shorter than min_length dropped; header split at the first blank
 * or tab into id / description (NULL: none); qualities mandatory (a FASTA record fails with "Qualities should be
 * present."); keep_ids (NULL: keep all) = the union of the reference's core and neighbour sets, which it applies only
 * when both are given (haec_io.rs:63-69).  Returns NULL and a message in err on the inputs the reference panics on.
 * Sequence and quality bytes of read i are [off[i], off[i+1]) of herro_reads_seq / herro_reads_qual — the arguments
 * of herro_set_reads.  Pointers stay valid until herro_reads_free.  A plain regular file is read by byte ranges on
 * HERRO_FASTX_THREADS threads (default min(hardware threads, 16); ~9 GB/s on 8 cores, 1.4 GB/s on one), gzip and pipes as one
 * stream; the result is the same either way. */
typedef struct herro_reads herro_reads;
herro_reads* herro_fastx_read(const char* path, uint32_t min_length, const char* const* keep_ids, uint64_t n_keep, char* err,
                              uint64_t err_cap);
uint32_t herro_reads_count(const herro_reads* r);
const uint8_t* herro_reads_seq(const herro_reads* r);
const uint8_t* herro_reads_qual(const herro_reads* r);
const uint64_t* herro_reads_off(const herro_reads* r);            /* [n + 1] */
const char* const* herro_reads_ids(const herro_reads* r);         /* [n] */
const char* const* herro_reads_descs(const herro_reads* r);       /* [n], NULL entries: no description */
void herro_reads_free(herro_reads* r);
/* The same handle over the caller's own arrays (copied): n reads, sequence and quality bytes of read i at [off[i], off[i+1]), ids[i] a C string,
 * descs NULL or its entries NULL: no description.  NULL and a message in err: a null argument, off that does not ascend from 0, a null id. */
herro_reads* herro_reads_create(uint32_t n, const uint8_t* seq, const uint8_t* qual, const uint64_t* off /* [n + 1] */, const char* const* ids,
                                const char* const* descs, char* err, uint64_t err_cap);

/* ---- adapters: found in the resident reads on the device, trimmed and split on the host ---------------------------
 * The step the reference leaves to scripts/preprocess.sh (porechop, duplex_tools split_on_adapter, seqkit seq -m): adapters at the read ends
 * are trimmed, a chimera is split at an adapter in its middle, short pieces are dropped.  The path is herro_fastx_read, herro_set_reads,
 * herro_find_adapters, herro_trim_plan, herro_reads_cut, herro_set_reads with the cut reads (or herro_store_cut, below, in place of the last
 * two: the store cut on the device), then the finder as before.  The specification is
 * the library's own (tests/adapter_ref.py), all integer; it does not reproduce porechop's or duplex_tools' choices, and no adapter list is
 * built in: the caller supplies the sequences.
 *
 * herro_find_adapters: approximate matches of every adapter in every read of the store (k_adapt_scan, k_adapt_start in csrc/adapter_dev.hip).
 *   Patterns.  Adapter a is seq[off[a], off[a+1]), m bases, 8 <= m <= 64, 1 <= n_adapters <= 32, bases A, C, G or T in either case.  Strand 0
 *   searches the adapter as given, strand 1 its reverse complement (not with HERRO_ADAPTERS_FORWARD_ONLY).  k = floor(m * max_err_pm / 1000),
 *   max_err_pm <= 500 and 0 = the default 250 (k = 0: any max_err_pm below 1000 / m, e.g. 1).
 *   Text.  A read's 2-bit codes as the store holds them — a byte that is not ACGT as herro_encode_2bit codes it.
 *   Score.  For an end position j in 1 .. len, E(j) = min over i <= j of the edit distance (unit costs) of the pattern and T[i, j); the empty
 *   substring is included, so E <= m.
 *   Hit.  A maximal run of consecutive j with E(j) <= k.  end = the j of the least E in the run, the smallest such j on ties; errors = that E;
 *   start = the largest i <= end with edit distance of the pattern and T[i, end) == errors.  start and end are forward read coordinates on
 *   either strand.  Runs of different patterns are different hits, even where they overlap (a palindromic adapter hits on both strands).
 *   Order.  Ascending (rid, end, start, adapter, strand); off[r] .. off[r + 1] are read r's hits.  The bytes depend neither on thread order
 *   nor on the segment length (HERRO_ADAPT_SEG, bases per lane, 8 .. 65536, default 256: a setting of the kernel's work split only).
 *   The hits are appended to a buffer of max(65536, segments / 8) entries; a scan that finds more is run a second time at the counted size
 *   (herro_debug_set_adapter_cap, a test hook, sets the first buffer's entries for the context's later calls; 0: the default).  HERRO_ADAPT_STATS=1 prints `ADAPT seg= segments= patterns= hits= scans= scan_ms=
 *   start_ms= host_ms=` on stderr.
 * Checks: parameters and adapters first (HERRO_E_INVALID naming the adapter; works on a context without a device), then HERRO_E_NO_DEVICE,
 * then HERRO_E_STATE without reads; more than 2^32 - 1 hits or segments: HERRO_E_UNSUPPORTED.  The call runs on the context's execution stream
 * and returns when it is done. */
typedef struct { uint32_t max_err_pm, flags, reserved[2]; } herro_adapter_params;   /* 0 = the field's default; reserved: 0 */
#define HERRO_ADAPTERS_FORWARD_ONLY 1u
typedef struct { uint32_t rid, start, end; uint16_t adapter; uint8_t strand, errors; } herro_adapter_hit;   /* 16 bytes */
typedef struct herro_adapter_hits herro_adapter_hits;
int herro_find_adapters(herro_ctx* ctx, uint32_t n_adapters, const char* seq, const uint64_t* off /* [n_adapters + 1] */,
                        const herro_adapter_params* params /* NULL: defaults */, herro_adapter_hits** out);
uint64_t herro_adapter_hits_n(const herro_adapter_hits* hits);
const herro_adapter_hit* herro_adapter_hits_data(const herro_adapter_hits* hits);
const uint64_t* herro_adapter_hits_off(const herro_adapter_hits* hits);      /* [n_reads + 1] */
void herro_adapter_hits_free(herro_adapter_hits* hits);
int herro_debug_set_adapter_cap(herro_ctx* ctx, uint64_t cap);               /* test hook, see above */
/* herro_trim_plan: the pieces of every read that stay, from a hit table (csrc/trim_plan.h: host code, no device).  0 in a field = its default:
 * end_window 150, end_max_err_pm 250, mid_max_err_pm 100, min_length 0 (preprocess.sh keeps reads of 10000 bases and more).
 *   Per read of length L, a hit of an adapter of m bases is a START hit if start < end_window and errors <= floor(m * end_max_err_pm / 1000);
 *   otherwise an END hit if end + end_window > L under the same bound; otherwise a MIDDLE hit if errors <= floor(m * mid_max_err_pm / 1000);
 *   otherwise it is ignored.  lo = the largest end of the start hits (0: none), hi = the smallest start of the end hits (L: none).  lo >= hi:
 *   the read gives no piece.  Middle hits are clipped to [lo, hi), overlapping or touching ones merged; the pieces are what is left of
 *   [lo, hi), ascending.  With HERRO_TRIM_DISCARD_CHIMERAS a read with any middle hit gives no piece.  Pieces shorter than
 *   max(min_length, 1) are dropped.
 * pieces are grouped by read: piece_off[r] .. piece_off[r + 1].  herro_trim_stats: reads trimmed (lo > 0 or hi < L), reads split (more than one
 * piece), reads dropped (no piece), bases removed (the reads' bases minus the pieces').
 * HERRO_E_INVALID and a message in err: a null argument, a hit outside its read, start > end, a hit whose rid is not its group's read, an
 * adapter index out of range, hits_off that does not ascend from 0, a non-zero reserved field, an unknown flag. */
typedef struct { uint32_t end_window, end_max_err_pm, mid_max_err_pm, min_length, flags, reserved[3]; } herro_trim_params;
#define HERRO_TRIM_DISCARD_CHIMERAS 1u
typedef struct { uint32_t rid, start, end; } herro_piece;
typedef struct herro_trim herro_trim;
int herro_trim_plan(uint32_t n_reads, const uint32_t* read_len, uint32_t n_adapters, const uint32_t* adapter_len, const herro_adapter_hit* hits,
                    const uint64_t* hits_off /* [n_reads + 1] */, const herro_trim_params* params /* NULL: defaults */, herro_trim** out,
                    char* err, uint64_t err_cap);
uint64_t herro_trim_n_pieces(const herro_trim* t);
const herro_piece* herro_trim_pieces(const herro_trim* t);
const uint64_t* herro_trim_piece_off(const herro_trim* t);                   /* [n_reads + 1] */
int herro_trim_stats(const herro_trim* t, uint64_t out[4]);                  /* reads trimmed, reads split, reads dropped, bases removed */
void herro_trim_free(herro_trim* t);
/* herro_reads_cut: a new handle whose read x is piece x of r — sequence and quality are the slices [start, end) of read rid, in the order of
 * `pieces` (any order).  A read with exactly one piece in the table keeps its id; one with n > 1 pieces gives <id>_1 .. <id>_n in the table's
 * order; the description is kept.  The result goes into herro_set_reads unchanged.  NULL and a message in err: a null argument, a rid outside
 * r, start > end, end beyond the read. */
herro_reads* herro_reads_cut(const herro_reads* r, uint64_t n_pieces, const herro_piece* pieces, char* err, uint64_t err_cap);
/* herro_reads_cut_names: the handle herro_reads_cut returns WITHOUT its bases, from the ids alone — ids and descriptions by the naming rule
 * above (the one implementation of it; both calls run it), herro_reads_off = the running sum of the piece lengths, herro_reads_seq / _qual
 * not to be read.  The caller of herro_store_cut names its pieces with it.  Read i has off[i + 1] - off[i] bases (off need not start at 0),
 * id ids[i], description descs[i] (descs NULL or an entry NULL: none).  NULL and a message in err as herro_reads_cut. */
herro_reads* herro_reads_cut_names(uint32_t n, const uint64_t* off /* [n + 1] */, const char* const* ids, const char* const* descs, uint64_t n_pieces,
                                   const herro_piece* pieces, char* err, uint64_t err_cap);

/* ---- the cut on the device: herro_store_cut replaces the context's read store by pieces of it (csrc/store_dev.hip) ---
 * Read x of the new store is bases [start, end) of read pieces[x].rid of the current store, in the table's order; any order, repeats and empty
 * pieces (start == end) are allowed, as in herro_reads_cut.  It stands for herro_reads_cut + herro_set_reads of the cut reads: the host
 * computes the new offset tables from the piece lengths and uploads them with the piece table, a few bytes per piece; no base and no quality
 * byte crosses PCIe in either direction (k_store_cut_words, k_store_cut_qual).
 * Specification (tests/cut_ref.py states it in numpy):
 *   Codes.  Code i of new read x is code start + i of the old read AS THE STORE HOLDS IT — including what a byte that is not ACGT smeared over
 *   its neighbours when the old store was encoded (herro_encode_2bit): a piece inherits the codes the adapters were found in.
 *   Words.  A new read starts at a word boundary, 32 codes per 64-bit word, LSB first; the bits above a read's last base in its last word are
 *   zero; one zero pad word follows the last read.
 *   Planes.  p0 / p1 are the even / odd bits of every new word, compacted as herro_set_reads compacts them, with its two zero pad entries.
 *   Qualities and offsets.  The qualities are the byte slice; word_off / qual_off are the running sums of ceil(len / 32) and len.
 *   Against the host path.  For reads whose bytes are all ACGT / acgt the new store equals, byte for byte in all six arrays, the one that
 *   herro_reads_cut + herro_set_reads builds.  For other reads it may differ: the host path re-encodes the ASCII slice, so a non-ACGT byte
 *   smears from the NEW word boundaries (and herro_encode_2bit can leave smear bits above a read's end), while the device path moves the old
 *   codes and zeroes the tail.  herro_set_reads_packed of the sliced codes is the exact equivalent in every case.
 * Afterwards the context is in the state herro_set_reads leaves it in: the reads are the pieces, name_class as given (NULL: x), jobs created on
 * the old store refuse with HERRO_E_STATE, and the store has a fresh owner — contexts that share the OLD store (herro_share_reads) keep it
 * until they call herro_share_reads again, and it is freed when its last holder lets go.  The new store is built beside the old one: peak
 * device memory is the old store plus the new one.
 * Checks, all before anything is touched (the store is unchanged on any error): HERRO_E_INVALID for a null table with n_pieces > 0, rid >=
 * n_reads, start > end, end beyond the read — the message names the first offending piece —, HERRO_E_UNSUPPORTED for more than 2^31 - 1
 * pieces; then HERRO_E_NO_DEVICE on a context without a device, then HERRO_E_STATE without reads.  A HIP call that fails while the new store
 * is built — device memory that runs out included, as everywhere in this library — is HERRO_E_NO_DEVICE with the call's name in the message,
 * and host memory that runs out is HERRO_E_UNSUPPORTED; what was allocated is freed and the store is unchanged in both cases.  Runs on the
 * context's execution stream and returns when it is done.  HERRO_CUT_STATS=1 prints `CUT pieces= words= qual_bytes= words_ms= qual_ms= copy_words_ms= copy_qual_ms=` on stderr
 * (the kernels between events; 2: also a device-to-device hipMemcpyAsync of the new word array and of the new quality array, the yardstick). */
int herro_store_cut(herro_ctx* ctx, uint64_t n_pieces, const herro_piece* pieces, const uint32_t* name_class /* [n_pieces] or NULL */);
/* Test hook: one array of the current store copied to the host.  which: 0 words (u64 [n_words + 1], the pad word included), 1 word_off (u64
 * [n_reads + 1]), 2 qualities (qual_bytes bytes, not the pad), 3 qual_off (u64 [n_reads + 1]), 4 p0, 5 p1 (u32 [n_words + 2]).  Returns the
 * array's size in bytes (out NULL: nothing is copied), or a negative error: cap smaller than the array, no device, no reads. */
int64_t herro_debug_store_copy(herro_ctx* ctx, int which, void* out, uint64_t cap);
/* Test hooks: the two device primitives every stage of the front end stands on (csrc/scan_sort_dev.hip: the exclusive scan of u32 and the stable
 * LSD radix sort of 64-bit keys with 64-bit payloads) and the 64-bit offset join of the device FASTA (csrc/fasta_dev.hip), on host arrays.  Each
 * call allocates ONE device block, lays its arrays in it exactly as large as a client sizes them — the scan's scratch dev_scan_partials(n) entries,
 * the sort's dev_sort_scratch(n) —, with 64 u32 words of a fixed pattern directly behind every array, runs the product's own code on the
 * context's execution stream and copies the result back.  *guard_hits: how many of those words no longer hold the pattern afterwards (a plain
 * memory comparison; 0 unless something wrote past an array's end).
 *   herro_debug_scan_u32    out[0 .. n] = the running sums of in[0 .. n) modulo 2^32, out[0] = 0, out[n] the total.
 *   herro_debug_radix_sort  keys / pays [n] are sorted in place, stably, by the 8-bit digits (key >> shifts[i]) & 255 in the order of the list
 *                           (ascending significance: LSD); what comes back is what (*k0, *p0) name after dev_radix_sort's pointer swaps.
 *                           An empty list moves nothing.
 *   herro_debug_offsets64   off[0 .. n] = the running sums of bytes[0 .. n) in 64 bits, formed as herro_job_fasta_dev forms its text offsets:
 *                           two 32-bit scans and a carry where the low prefix falls.  Exact while the total is below 2^64.
 * HERRO_E_INVALID for a null argument (in / keys / pays / shifts / bytes may be NULL where their count is 0) or a shift above 63,
 * HERRO_E_UNSUPPORTED for n above 2^31 - 1, HERRO_E_NO_DEVICE on a context without a device or when a HIP call fails.  No reads are needed. */
int herro_debug_scan_u32(herro_ctx* ctx, const uint32_t* in, uint64_t n, uint32_t* out /* [n + 1] */, uint32_t* guard_hits);
int herro_debug_radix_sort(herro_ctx* ctx, uint64_t* keys, uint64_t* pays, uint64_t n, const uint32_t* shifts, uint32_t n_shifts, uint32_t* guard_hits);
int herro_debug_offsets64(herro_ctx* ctx, const uint64_t* bytes, uint64_t n, uint64_t* off /* [n + 1] */, uint32_t* guard_hits);

/* ---- clusters: the reads partitioned by their overlap graph (csrc/cluster_dev.hip, csrc/cluster_plan.h) -------------------
 * The reference's workflow runs scripts/create_clusters.py between the batched alignments and `herro inference -c <cluster>`: METIS cuts the
 * overlap graph into k parts and every part becomes a file of `0\t<name>` lines for its core reads and `1\t<name>` lines for their neighbours,
 * which read_cluster takes apart again (lib.rs:208-239; haec_io.rs:62-68 keeps the reads of either set, overlaps.rs:154-159 the overlaps whose
 * target is core).  The entries below make those clusters on the device, as core masks (1 core, 2 neighbour, 0 neither) in the shape the
 * `core` arguments of the finder above take.  This is NOT METIS: it is a small specification of our own, all integer and independent of any
 * thread order (tests/cluster_ref.py states it in numpy), and its masks are exact whatever its quality — the corrected reads do not depend
 * on the partition, only the amount of work does.
 * Specification.  n reads with weights w (u32, NULL: all 1), E undirected edges (a, b, span) (span NULL: every edge is strong), n_parts k, min_span:
 *   1. Strong edges: span >= min_span (min_span 0: all).  Weak edges count in steps 6 and 7 only.
 *   2. comp[v]: the least read id reachable from v over strong edges.
 *   3. d1[v]: the BFS distance over strong edges from comp[v]; far[c]: the read of component c with the greatest d1, the least id among equals;
 *      level[v]: the BFS distance from far[comp[v]] — two sweeps from a pseudo-peripheral read, all components at once.
 *   4. Order: ascending (comp, level, v); rank[v] is its position.
 *   5. Cut: S[v] = the sum of w over the reads before v in the order, T the total; part[v] = min(k - 1, S[v] * k / T) in 64-bit integers, part 0
 *      for all when T == 0.  Hence |weight of a part - T / k| < max w.
 *   6. Mask of part p, over ALL edges (a rank needs every query of its targets): 1 where part[v] == p, 2 where v is not core and adjacent to a core
 *      read of p, 0 otherwise.
 *   7. Statistics.  Per part: n_core, weight, n_neighbours, pairs_inside (both ends in p), pairs_touching (at least one end in p: what the rank of
 *      p aligns).  Global: n_components, n_levels (greatest level + 1), strong_edges, edge_cut (edges whose ends differ in part; duplicates count
 *      as given).
 * a > b, duplicate edges and k > n_reads are legal.  Checks, in this order: HERRO_E_INVALID — params NULL, n_parts outside 1 .. 65535, a reserved
 * field not 0, an edge with a == b or a read id >= n_reads; the message names the first offending edge —, HERRO_E_UNSUPPORTED — n_reads or n_edges
 * above 2^31 - 1, T >= 2^32 —, then HERRO_E_NO_DEVICE on a context without a device.  A HIP call that fails is HERRO_E_NO_DEVICE with its name,
 * host memory that runs out HERRO_E_UNSUPPORTED; no handle is made in either case.
 * The calls run on the context's execution stream and return when the results are on the host; the graph (edges, parts) stays on the device
 * inside the handle, so that a mask costs two kernels and one download.  The handle needs its context until it is freed, nothing else: not the
 * arrays it was made from, not the pairs handle.  HERRO_CLUSTER_STATS=1 prints `CLUSTER reads= edges= ... arcs_ms= comp_ms= bfs_ms= order_ms=
 * stats_ms= hook_rounds= bfs_launches= host_reads=` on stderr (the stages between events). */
typedef struct {
  uint32_t n_parts;      /* k: 1 .. 65535 */
  uint32_t min_span;     /* edges with span below it are weak; 0: every edge is strong */
  uint32_t reserved[2];  /* 0 */
} herro_cluster_params;
typedef struct herro_clusters herro_clusters;
/* herro_cluster_graph: the clusters of a graph given as host arrays — what create_clusters.py reads from its edge list; it needs no read store. */
int herro_cluster_graph(herro_ctx* ctx, uint64_t n_reads, const uint32_t* weights /* [n_reads] or NULL */, uint64_t n_edges, const uint32_t* a,
                        const uint32_t* b, const uint32_t* span /* [n_edges] or NULL */, const herro_cluster_params* params, herro_clusters** out);
/* herro_pairs_cluster: the graph is the handle's P primaries (tid, qid), span = min(tend - tstart, qend - qstart) as the handle holds them (the
 * chains' spans with HERRO_PAIRS_NO_EXTEND), n_reads the store's; weights [n_reads] or NULL (the Python layer passes windows per read).  The
 * primaries go up from the handle's host copy: herro_pairs keeps none on the device.  A handle of another context is HERRO_E_INVALID. */
int herro_pairs_cluster(herro_ctx* ctx, const herro_pairs* pairs, const uint32_t* weights, const herro_cluster_params* params, herro_clusters** out);
uint32_t herro_clusters_n_parts(const herro_clusters* cl);
uint64_t herro_clusters_n_reads(const herro_clusters* cl);
const uint32_t* herro_clusters_part(const herro_clusters* cl);    /* [n_reads]; these four stay valid until the handle is freed */
const uint32_t* herro_clusters_rank(const herro_clusters* cl);
const uint32_t* herro_clusters_comp(const herro_clusters* cl);
const uint32_t* herro_clusters_level(const herro_clusters* cl);
int herro_clusters_stats(const herro_clusters* cl, uint64_t out[4]);                  /* n_components, n_levels, strong_edges, edge_cut */
int herro_clusters_part_stats(const herro_clusters* cl, uint32_t p, uint64_t out[5]); /* n_core, weight, n_neighbours, pairs_inside, pairs_touching */
/* The mask of part p (step 6) — the `core` and `neighbour` sets of read_cluster (lib.rs:208-239) as one byte per read: a non-zero byte marks a read
 * the rank of p loads, a 1 a read it corrects.  Made on the device from the resident graph on every call. */
int herro_clusters_mask(const herro_clusters* cl, uint32_t p, uint8_t* out /* [n_reads] */);
void herro_clusters_free(herro_clusters* cl);

/* ---- corrected reads as FASTA formed on the device, chopped for the assembler (csrc/fasta_dev.hip, csrc/chop_plan.h) -------
 * The reference's workflow runs scripts/postprocess_corrected.sh behind `herro inference`: `seqkit sliding -s 30000 -W 30000 -g` cuts every corrected
 * read into pieces of 30000 bases (the last one shorter) and `seqkit seq -m 10000` drops the pieces below 10000; the result is what hifiasm is given.
 * herro_job_fasta_dev writes that file's text — or, with all-zero parameters, herro_job_fasta's, byte for byte — on the device, from the bases
 * herro_job_consensus left there: records are segmented, chopped, filtered, named and written by kernels, and the host receives finished text,
 * copied to its place in one pinned block that the handle owns.  herro_job_fasta downloads every padded window slot and assembles on the host
 * pool; it stays the default path.
 * Specification (tests/chop_ref.py states it as a function of herro_job_fasta's text; all integer, independent of any thread order or chunk size):
 *   Segments (consensus.rs:90-111, lib.rs:282-317, as herro_job_fasta).  Window w is corrected iff min(n_overlaps kept, 30) >= 2.  The maximal runs of
 *   corrected windows of a target are its segments; a segment's sequence is its windows' corrected bases in order; segments of length 0 are dropped,
 *   the rest numbered i = 0 .. n_seg - 1; the name is id if n_seg == 1, else id:i.  A target with ids[t] == NULL gives nothing.
 *   Pieces.  A segment of n bases with chop_len C: C == 0 gives one piece [0, n) without suffix; C > 0 gives pieces k = 0 .. ceil(n / C) - 1 =
 *   [kC, min((k + 1)C, n)), each with the suffix `_sliding:<kC + 1>-<min((k + 1)C, n)>` (1-based, inclusive, decimal, as seqkit names them; also
 *   when there is one piece).  This is `seqkit sliding -s C -W C -g`; unequal step and window are not offered.  A piece is kept iff
 *   end - start >= min_length.  The `:i` numbering is that of the segments, before any piece is dropped.
 *   Record.  '>' name suffix ' ' [desc] '\n' body '\n'; the space is always there, as in herro_job_fasta.  line_width L > 0: a '\n' behind every L
 *   bases of the body except at its end; 0: one line.  Order: target, segment, piece, ascending.
 * herro_fasta_text_target_end: [n_targets], the offset behind every target's records, as herro_job_fasta's rec_end.  herro_fasta_text_stats: records
 * written, bases written, pieces dropped, bases dropped, segments (non-empty), targets that gave at least one record.  The pointers stay valid
 * until herro_fasta_text_free; the text lies in page-locked host memory that is recycled through the context (up to four blocks are kept), so a
 * caller that keeps many texts copies them out.  A handle may be freed after its context.
 * Checks, in this order: HERRO_E_INVALID — job or out NULL, ids NULL with targets, a parameter herro_chop_plan refuses —, HERRO_E_STATE —
 * herro_job_consensus has not run —, HERRO_E_UNSUPPORTED — window slots of 2^32 bytes or more in the job, which keeps bases and pieces below 2^32.
 * A HIP call that fails is HERRO_E_NO_DEVICE with the call's name; nothing stays allocated.  The call checks the sibling tiles of the job's model
 * pass as the fetch of herro_job_fasta does, and forms the text from the repeated pass if that check repeats it.  It runs on the context's execution
 * stream and returns when the text is on the host.  The text is formed in chunks of a sixteenth of HERRO_FASTA_SCRATCH_MB (default 1024) in two
 * device buffers, each copied down behind its kernel;
 * herro_debug_set_fasta_chunk, a test hook, sets the chunk's bytes for the context's later calls (0: the default) — the bytes of the text do not
 * depend on it.  HERRO_FASTA_STATS=1 prints `FASTA targets= segments= pieces= dropped= bytes= chunks= seg_ms= piece_ms= write_ms=` on stderr. */
typedef struct { uint32_t chop_len, min_length, line_width, flags, reserved[4]; } herro_chop_params;   /* 0 = off; reserved, flags: 0 */
typedef struct herro_fasta_text herro_fasta_text;
int herro_job_fasta_dev(herro_job* job, const char* const* ids, const char* const* descs /* NULL or entries NULL: none */,
                        const herro_chop_params* params /* NULL: all zero */, herro_fasta_text** out);
const char* herro_fasta_text_data(const herro_fasta_text* t);
uint64_t herro_fasta_text_len(const herro_fasta_text* t);
const uint64_t* herro_fasta_text_target_end(const herro_fasta_text* t);     /* [n_targets] */
int herro_fasta_text_stats(const herro_fasta_text* t, uint64_t out[6]);      /* records, bases written, pieces dropped, bases dropped, segments, targets emitted */
void herro_fasta_text_free(herro_fasta_text* t);
int herro_debug_set_fasta_chunk(herro_ctx* ctx, uint64_t bytes);             /* test hook, see above */
/* herro_chop_plan: the piece rule alone, over sequence lengths (csrc/chop_plan.h: host code, no device) — the pieces {seq, start, end} that
 * herro_job_fasta_dev keeps of segments of these lengths, grouped by sequence (piece_off[s] .. piece_off[s + 1]), in a herro_trim handle (its
 * accessors above).  herro_trim_stats of it: pieces kept, pieces dropped, bases kept, bases dropped.  An empty sequence gives no piece with
 * chop_len > 0 and its one empty piece with chop_len == 0.  HERRO_E_INVALID and a message in err: a null argument, a non-zero reserved field or
 * flag, chop_len or line_width above 2^31 - 1; HERRO_E_UNSUPPORTED: a sequence of 2^32 bases or more, more than 2^32 - 1 sequences or pieces
 * (counted before the filter). */
int herro_chop_plan(uint64_t n_seqs, const uint64_t* len, const herro_chop_params* params /* NULL: all zero */, herro_trim** out, char* err,
                    uint64_t err_cap);

/* One window of `herro features` (output_features, features.rs:724-764): <dir>/<wid>.ids.txt (one id per line),
 * <wid>.features.npy = u8 [2, length, 31] (ASCII bases [length][31], then qualities), <wid>.supported.npy = records
 * {pos: <u2, ins: u1}.  NPY format 1.0, C order, header as numpy writes it (dict padded with spaces to a multiple of 64
 * bytes). */
int herro_write_window_features(const char* dir, uint32_t wid, const char* const* ids, uint32_t n_ids, const uint8_t* bases,
                                const uint8_t* quals, uint32_t length, const uint16_t* sup_pos, const uint8_t* sup_ins,
                                uint32_t n_sup);
/* `herro features` for a featurized job (FeatsGenOutput, features.rs:783-839): every window of every target into
 * <base_dir>/<read id of the target>/, read_names[rid] for all reads of the store.  Returns the number of windows
 * written or a negative error. */
int64_t herro_job_write_features(herro_job* job, const char* base_dir, const char* const* read_names);

/* ---- several contexts (GPUs) of ONE process fed from one queue (csrc/pool.cpp) --------------------------------------------------
 * Replaces the thread layout of lib.rs:154-200 (per device: `t` feature threads + one inference thread pulling from one MPMC
 * channel; one writer, lib.rs:267-291): herro_pool_create makes one context per entry of device_ids (several entries may name the
 * same device: its contexts share one read store) with a worker thread each; herro_pool_correct cuts the targets into groups of
 * `group_targets` reads and the workers PULL groups from one shared counter — whoever is free takes the next one — keeping two
 * jobs in flight per context (the next group is created while the GPU works on the current one).  The FASTA records of all
 * targets, in target order, stay with the pool until the next call: herro_pool_result returns the text and (via *rec_end) the
 * end offset of every target's records; the return value of herro_pool_correct is the text's length (< 0: HERRO_E_*, message in
 * herro_pool_last_error).  ids / descs: one C string per target (descs or its entries may be NULL), as for herro_job_fasta.
 * herro_pool_ctx exposes a context (e.g. for herro_set_precision, herro_model_describe); herro_pool_groups_taken says how many
 * groups context i took in the last call.  A client of this header only: every result is what the per-job calls give. */
typedef struct herro_pool herro_pool;
herro_pool* herro_pool_create(const int* device_ids, uint32_t n_ctx);
void herro_pool_destroy(herro_pool* pool);
const char* herro_pool_last_error(const herro_pool* pool);
uint32_t herro_pool_size(const herro_pool* pool);
herro_ctx* herro_pool_ctx(herro_pool* pool, uint32_t i);
int herro_pool_set_reads(herro_pool* pool, uint32_t n_reads, const uint8_t* seq, const uint8_t* qual, const uint64_t* off, const uint32_t* name_class);
int herro_pool_load_model(herro_pool* pool, const char* path);
int64_t herro_pool_correct(herro_pool* pool, uint32_t n_targets, const uint32_t* rids, const uint64_t* aln_off, const herro_alignment* alns,
                           uint32_t window_size, uint32_t batch_size, int batch_mode, uint32_t group_targets, const char* const* ids,
                           const char* const* descs);
const char* herro_pool_result(const herro_pool* pool, const uint64_t** rec_end);
uint32_t herro_pool_groups_taken(const herro_pool* pool, uint32_t i);
/* Alignments / targets the jobs of the last herro_pool_correct left out (herro_job_skipped summed over its groups). */
int herro_pool_skipped(const herro_pool* pool, uint64_t* n_alignments, uint64_t* n_targets);
/* Host-only test hook: a pool of n_ctx stand-in contexts that needs no device — context i "works" us_per_aln[i] microseconds per
 * alignment of a group, the FASTA of a target is ">id\n" + (rid % 7 + 1) bases; rid 0xfffffffe makes the group's herro_job_create fail
 * with HERRO_E_UNSUPPORTED, rid 0xfffffffd its herro_job_infer with HERRO_E_STATE; a target whose first alignment has qid == tid
 * counts as one skipped alignment.  Everything else (queue, two jobs in flight, merge, error paths) is herro_pool_correct's own code. */
herro_pool* herro_debug_pool_fake(uint32_t n_ctx, const uint32_t* us_per_aln);

#ifdef __cplusplus
}
#endif
#endif /* HERRO_AMD_H */
