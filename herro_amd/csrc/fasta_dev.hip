// fasta_dev.hip — FASTA text of a job's corrected reads, formed where the consensus kernel left the bases (fasta_dev.h; specification: DESIGN.md §15,
// tests/chop_ref.py; the piece rule and the byte counts: chop_plan.h).  Stages, every prefix by the shared scan (dev_scan_u32, scan_sort_dev.h):
//   segments   k_fa_win     one lane per window: its target (a search in tgt_win_off), corrected or not (consensus.rs:90-101: min(n_alns, 30) >= 2, and
//                           the target has an id), its bases, and whether it begins a run of corrected windows.
//              (scans)      base prefix of the windows; number of the run a window begins.
//              k_fa_ends    the window that begins run s writes its first window, the window that ends it its last: heads and tails alternate, so
//                           both know s from the scan and nobody searches or counts.
//              k_fa_run     one lane per run: its bases (a difference of prefixes), non-empty or not, and what the filter keeps of its pieces —
//                           arithmetic (chop_count), since only the last piece of a run can be short.  The statistics are integer sums.
//              (scans)      number of the non-empty runs (a target's segments are a difference of it: ':' i and n_seg); first kept piece of a run.
//   pieces     k_fa_piece   one lane per kept piece: its run (a search), its bounds and the bytes of its record (fa_piece: the layout k_fa_write uses).
//              (scans)      64-bit text offsets out of two 32-bit scans: the low words scan modulo 2^32, a lane that sees the low prefix fall adds
//                           the carry to its high word (k_fa_carry), the high words scan, k_fa_off joins them.
//              k_fa_tgt     per target: where its records end.
//   write      k_fa_write   one lane per 16 bytes of TEXT, aligned on the destination: the work is split by bytes, so a read of 500 kb is 30000 lanes
//                           like any other 500 kb.  A lane finds its piece (a search in the offsets) and, where its 16 bytes are bases of one window
//                           without a line break, takes them with three aligned 8-byte loads and a funnel shift (the scheme of store_cut_qual16) and
//                           stores them once; everywhere else — headers, line breaks, window and record seams — it forms the bytes one by one
//                           (fa_head_byte, fa_body_byte).  Every byte is a function of its offset alone: no atomics, no LDS, the same text for every chunk size.
#include "fasta_dev.h"

#include <algorithm>
#include <chrono>

#include "scan_sort_dev.h"

namespace herro {
namespace {

struct FaDev {
  // the job
  const WinDesc* win; const uint32_t* nkept; const uint32_t* cons_len; const uint8_t* cons_seq;
  uint64_t row_elems;
  uint32_t n_win, n_tgt;
  const uint32_t* two;        // [n_tgt + 1] first window of a target
  const uint8_t* present;     // [n_tgt]
  const char* blob; const uint64_t* noff;
  ChopRule R;
  // per window ([n_win], prefixes [n_win + 1])
  uint32_t *win_t, *wlen, *head, *wpre, *hidx;
  // per run (room for n_win; hidx[n_win] exist)
  uint32_t *run_a, *run_b, *run_t, *nonempty, *kept, *segpos, *piece_off;
  // per kept piece ([P], prefixes [P + 1])
  uint32_t P;
  uint32_t *piece_run, *lo_in, *lo, *hi_in, *hi;
  uint64_t* off;
  uint64_t* tgt_end;              // [n_tgt]
  unsigned long long* stats;      // [6] herro_fasta_text_stats
};

// largest i in [lo, hi) with a[i] <= v (a ascends, a[lo] <= v)
template <typename T>
__device__ inline uint32_t last_le(const T* __restrict__ a, uint32_t lo, uint32_t hi, T v) {
  while (hi - lo > 1) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] <= v) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ inline bool fa_corrected(const FaDev& D, uint32_t w, uint32_t t) { return D.present[t] && D.nkept[w] >= 2u; }   // min(n, 30) >= 2

__global__ __launch_bounds__(256) void k_fa_win(FaDev D) {
  const uint32_t w = blockIdx.x * 256u + threadIdx.x;
  if (w >= D.n_win) return;
  const uint32_t t = last_le(D.two, 0u, D.n_tgt, w);          // (two[0] = 0 <= w < two[n_tgt]; a target without windows is stepped over)
  const bool c = fa_corrected(D, w, t);
  D.win_t[w] = t;
  D.wlen[w] = c ? D.cons_len[w] : 0u;
  D.head[w] = c && (w == D.two[t] || !fa_corrected(D, w - 1, t));
}

__global__ __launch_bounds__(256) void k_fa_ends(FaDev D) {
  const uint32_t w = blockIdx.x * 256u + threadIdx.x;
  if (w >= D.n_win) return;
  const uint32_t t = D.win_t[w];
  if (!fa_corrected(D, w, t)) return;
  if (D.head[w]) { const uint32_t s = D.hidx[w]; D.run_a[s] = w; D.run_t[s] = t; }
  if (w + 1 == D.two[t + 1] || !fa_corrected(D, w + 1, t)) D.run_b[D.hidx[w + 1] - 1u] = w + 1;   // (hidx[w + 1] counts this run's head)
}

__global__ __launch_bounds__(256) void k_fa_run(FaDev D) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= D.n_win) return;
  uint32_t ne = 0, kept = 0;
  if (s < D.hidx[D.n_win]) {
    const uint64_t n = D.wpre[D.run_b[s]] - D.wpre[D.run_a[s]];
    if (n) {
      const ChopCount c = chop_count(n, D.R);
      const uint64_t all = chop_n_pieces(c), k = chop_n_kept(c);
      const uint64_t bases = (c.full_kept ? c.full * D.R.C : 0) + (c.rem_kept ? c.rem : 0);
      ne = 1; kept = (uint32_t)k;
      atomicAdd(&D.stats[1], (unsigned long long)bases);
      atomicAdd(&D.stats[2], (unsigned long long)(all - k));
      atomicAdd(&D.stats[3], (unsigned long long)(n - bases));
      atomicAdd(&D.stats[4], 1ull);
    }
  }
  D.nonempty[s] = ne;
  D.kept[s] = kept;
}

// Everything about kept piece p of run s: what k_fa_piece counts and k_fa_write writes.
struct FaPiece {
  uint64_t id0, idl, d0, dl;    // id and description in the blob
  uint32_t n_seg, seg;          // segments of the target, this one's number
  uint32_t a, b;                // windows of the run
  uint32_t start, end;          // the piece inside the run
  uint64_t gbase;               // base prefix of its first base
  uint64_t head, body;          // bytes
};
__device__ inline FaPiece fa_piece(const FaDev& D, uint32_t p, uint32_t s) {
  FaPiece I;
  const uint32_t t = D.run_t[s];
  const uint32_t r0 = D.hidx[D.two[t]], r1 = D.hidx[D.two[t + 1]];
  I.n_seg = D.segpos[r1] - D.segpos[r0];
  I.seg = D.segpos[s] - D.segpos[r0];
  I.a = D.run_a[s]; I.b = D.run_b[s];
  const uint64_t n = D.wpre[I.b] - D.wpre[I.a];
  uint64_t st, en;
  chop_bounds(n, D.R, chop_kept_index(chop_count(n, D.R), p - D.piece_off[s]), &st, &en);
  I.start = (uint32_t)st; I.end = (uint32_t)en;
  I.gbase = (uint64_t)D.wpre[I.a] + st;
  I.id0 = D.noff[2 * (uint64_t)t]; I.d0 = D.noff[2 * (uint64_t)t + 1];
  I.idl = I.d0 - I.id0; I.dl = D.noff[2 * (uint64_t)t + 2] - I.d0;
  I.head = chop_head_bytes(I.idl, I.dl, I.n_seg, I.seg, D.R, st, en);
  I.body = chop_body_bytes(en - st, D.R);
  return I;
}

__global__ __launch_bounds__(256) void k_fa_piece(FaDev D) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= D.P) return;
  const uint32_t s = last_le(D.piece_off, 0u, D.n_win, p);   // (a run that keeps nothing is stepped over: its successor has the same offset)
  const FaPiece I = fa_piece(D, p, s);
  const uint64_t bytes = I.head + I.body;
  D.piece_run[p] = s;
  D.lo_in[p] = (uint32_t)bytes;
  D.hi_in[p] = (uint32_t)(bytes >> 32);
}

__global__ __launch_bounds__(256) void k_fa_carry(FaDev D) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= D.P) return;
  D.hi_in[p] += D.lo[p + 1] < D.lo[p];        // the low prefix wrapped at this piece (at most once: one addend)
}

__global__ __launch_bounds__(256) void k_fa_off(FaDev D) {
  const uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (p > D.P) return;
  D.off[p] = (uint64_t)D.hi[p] << 32 | D.lo[p];
}

__global__ __launch_bounds__(256) void k_fa_tgt(FaDev D) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= D.n_tgt) return;
  const uint32_t p0 = D.piece_off[D.hidx[D.two[t]]], p1 = D.piece_off[D.hidx[D.two[t + 1]]];
  D.tgt_end[t] = D.off[p1];
  if (p1 > p0) atomicAdd(&D.stats[5], 1ull);
}

__device__ inline char fa_digit(uint64_t v, uint32_t nd, uint32_t e) {   // digit e of nd, the most significant first
  for (uint32_t i = e + 1; i < nd; i++) v /= 10;
  return (char)('0' + (uint32_t)(v % 10));
}

// byte r of the header (r < I.head)
__device__ inline char fa_head_byte(const FaDev& D, const FaPiece& I, uint64_t r) {
  if (r == 0) return '>';
  r -= 1;
  if (r < I.idl) return D.blob[I.id0 + r];
  r -= I.idl;
  if (I.n_seg > 1) {
    if (r == 0) return ':';
    r -= 1;
    const uint32_t nd = chop_digits(I.seg);
    if (r < nd) return fa_digit(I.seg, nd, (uint32_t)r);
    r -= nd;
  }
  if (D.R.C) {
    if (r < 9) return (char)(r < 8 ? (0x676e6964696c735full >> (8 * r)) & 0xff : ':');   // "_sliding" ':'
    r -= 9;
    uint32_t nd = chop_digits((uint64_t)I.start + 1);
    if (r < nd) return fa_digit((uint64_t)I.start + 1, nd, (uint32_t)r);
    r -= nd;
    if (r == 0) return '-';
    r -= 1;
    nd = chop_digits(I.end);
    if (r < nd) return fa_digit(I.end, nd, (uint32_t)r);
    r -= nd;
  }
  if (r == 0) return ' ';
  r -= 1;
  if (r < I.dl) return D.blob[I.d0 + r];
  return '\n';
}

// byte j of the body (j < I.body); w: the window the previous base came from (a hint)
__device__ inline char fa_body_byte(const FaDev& D, const FaPiece& I, uint64_t j, uint32_t& w) {
  if (j + 1 == I.body) return '\n';
  uint64_t q = j;
  if (D.R.L) {
    const uint64_t per = (uint64_t)D.R.L + 1;
    if (j % per == D.R.L) return '\n';
    q = j - j / per;
  }
  const uint32_t g = (uint32_t)(I.gbase + q);                    // (< wpre[b] <= 2^32 - 1)
  if (w < I.a || w >= I.b || D.wpre[w] > g || D.wpre[w + 1] <= g) w = last_le(D.wpre, I.a, I.b, g);
  const uint64_t src = D.win[w].row_off + (g - D.wpre[w]);
  return src < D.row_elems ? (char)D.cons_seq[src] : '?';
}

__global__ __launch_bounds__(256) void k_fa_write(FaDev D, uint64_t x0, uint64_t x1, char* __restrict__ text) {
  const uint64_t x = x0 + 16ull * ((uint64_t)blockIdx.x * 256u + threadIdx.x);
  if (x >= x1) return;                                              // (x0 is a multiple of 16 and text has room for whole 16-byte stores)
  uint32_t p = last_le(D.off, 0u, D.P, x);                          // (off[0] = 0 <= x < off[P]; records are never empty)
  FaPiece I = fa_piece(D, p, D.piece_run[p]);
  uint64_t o0 = D.off[p], o1 = D.off[p + 1];
  uint32_t w = I.a;
  uint64_t lo = 0, hi = 0;
  const uint64_t r = x - o0;
  bool fast = false;
  if (x + 16 <= x1 && r >= I.head) {
    const uint64_t j = r - I.head;
    uint64_t q = j;
    bool plain = j + 16 < I.body;                                   // bases only: the record's last byte is its '\n'
    if (plain && D.R.L) {
      const uint64_t per = (uint64_t)D.R.L + 1;
      plain = j % per + 16 <= D.R.L;
      q = j - j / per;
    }
    if (plain) {
      const uint32_t g = (uint32_t)(I.gbase + q);
      w = last_le(D.wpre, I.a, I.b, g);
      const uint64_t src = D.win[w].row_off + (g - D.wpre[w]);
      const uint8_t* const s = D.cons_seq + src;
      const uint32_t m = (uint32_t)((uintptr_t)s & 7u);
      if ((uint64_t)g + 16 <= D.wpre[w + 1] && src >= m && src - m + 24 <= D.row_elems) {   // one window, and the aligned loads stay inside the array
        const uint64_t* const a = (const uint64_t*)(s - m);
        const uint64_t w0 = a[0], w1 = a[1];
        if (!m) { lo = w0; hi = w1; }
        else { const uint64_t w2 = a[2]; lo = (w0 >> (8u * m)) | (w1 << (64u - 8u * m)); hi = (w1 >> (8u * m)) | (w2 << (64u - 8u * m)); }
        fast = true;
      }
    }
  }
  if (!fast) {
    for (uint32_t i = 0; i < 16; i++) {
      const uint64_t y = x + i;
      if (y >= x1) break;
      while (y >= o1) {                                             // (y < x1 <= off[P]: ends)
        p++;
        I = fa_piece(D, p, D.piece_run[p]);
        o0 = o1; o1 = D.off[p + 1]; w = I.a;
      }
      const uint64_t ry = y - o0;
      const uint64_t c = (uint8_t)(ry < I.head ? fa_head_byte(D, I, ry) : fa_body_byte(D, I, ry - I.head, w));
      if (i < 8) lo |= c << (8u * i); else hi |= c << (8u * (i - 8u));
    }
  }
  *(ulonglong2*)(text + (x - x0)) = make_ulonglong2(lo, hi);
}

double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

inline uint32_t blocks(uint64_t n) { return (uint32_t)((n + 255) / 256); }

// Arrays cut from one block, 256 bytes apart at least: run once without a base for the size, once more with the block.
struct Carver {
  char* base = nullptr;
  uint64_t at = 0;
  template <typename T>
  void take(T** out, uint64_t count) {
    at = (at + 255) & ~255ull;
    if (base) *out = (T*)(base + at);
    at += std::max<uint64_t>(count, 1) * sizeof(T) + 64;
  }
};

}  // namespace

#define FA_TRY(what, expr) do { const hipError_t _e = (expr); if (_e != hipSuccess) { (void)hipStreamSynchronize(st); err = std::string("herro_job_fasta_dev: ") + what + ": " + hipGetErrorString(_e); return FASTA_HIP; } } while (0)
#define FA_SCAN(in, n, out) do { if (dev_scan_u32(in, n, out, d_partial, st, err) != 0) { (void)hipStreamSynchronize(st); err = "herro_job_fasta_dev: " + err; return FASTA_HIP; } } while (0)
#define FA_MEM(ptr, what) do { if (!(ptr)) { (void)hipStreamSynchronize(st); err = std::string("herro_job_fasta_dev: out of memory for ") + what; return FASTA_HIP; } } while (0)

// The 64-bit offsets of D.P pieces out of two 32-bit scans (the stages' "(scans)" of the pieces): lo_in / hi_in hold the halves of every piece's
// bytes; hi_in takes the carries.  partial: dev_scan_partials(D.P) entries.  Queued on st.
static int offsets64(const FaDev& D, uint32_t* d_partial, hipStream_t st, std::string& err) {
  const uint32_t P = D.P;
  FA_SCAN(D.lo_in, P, D.lo);
  k_fa_carry<<<blocks(P), 256, 0, st>>>(D);
  FA_TRY("k_fa_carry launch", hipGetLastError());
  FA_SCAN(D.hi_in, P, D.hi);
  k_fa_off<<<blocks((uint64_t)P + 1), 256, 0, st>>>(D);
  FA_TRY("k_fa_off launch", hipGetLastError());
  return FASTA_OK;
}

int fasta_offsets64(uint32_t* lo_in, uint32_t* hi_in, uint32_t n, uint32_t* lo, uint32_t* hi, uint64_t* off, uint32_t* partial, hipStream_t st,
                    std::string& err) {
  FaDev D{};
  D.P = n; D.lo_in = lo_in; D.hi_in = hi_in; D.lo = lo; D.hi = hi; D.off = off;
  return offsets64(D, partial, st, err);
}

int fasta_text_dev(const JobDev& J, uint64_t row_elems, const uint32_t* tgt_win_off, uint32_t n_targets, const FastaNames& names, const ChopRule& R,
                   uint64_t chunk, hipStream_t st, const FastaMem& mem, char** text, uint64_t* text_len, std::vector<uint64_t>& target_end,
                   FastaStats& stats, std::string& err) {
  *text = nullptr;
  *text_len = 0;
  target_end.assign(n_targets, 0);
  stats = FastaStats{};
  stats.n_targets = n_targets;
  const uint32_t N = J.n_win;
  if (!N || !n_targets) return FASTA_OK;
  FaDev D{};
  D.win = J.win; D.nkept = J.win_nkept; D.cons_len = J.cons_len; D.cons_seq = J.cons_seq;
  D.row_elems = row_elems; D.n_win = N; D.n_tgt = n_targets; D.R = R;
  uint32_t* d_two = nullptr; uint8_t* d_present = nullptr; char* d_blob = nullptr; uint64_t* d_noff = nullptr;
  uint32_t* d_partial = nullptr;
  auto t0 = std::chrono::steady_clock::now();
  // ---- the first block: what is sized by windows, targets and names
  auto lay_a = [&](Carver& c) {
    c.take(&d_two, (uint64_t)n_targets + 1); c.take(&d_present, n_targets); c.take(&d_blob, names.blob.size()); c.take(&d_noff, names.off.size());
    uint32_t** const per_win[] = {&D.win_t, &D.wlen, &D.head, &D.wpre, &D.hidx, &D.run_a, &D.run_b, &D.run_t, &D.nonempty, &D.kept, &D.segpos, &D.piece_off};
    for (uint32_t** q : per_win) c.take(q, (uint64_t)N + 1);
    c.take(&D.tgt_end, n_targets); c.take(&D.stats, 6); c.take(&d_partial, (uint64_t)dev_scan_partials(N) + 1);
  };
  Carver ca;
  lay_a(ca);
  ca.base = (char*)mem.dev(ca.at);
  FA_MEM(ca.base, "the window arrays");
  ca.at = 0;
  lay_a(ca);
  FA_TRY("target offset upload", hipMemcpyAsync(d_two, tgt_win_off, 4ull * (n_targets + 1ull), hipMemcpyHostToDevice, st));
  FA_TRY("target flag upload", hipMemcpyAsync(d_present, names.present.data(), n_targets, hipMemcpyHostToDevice, st));
  if (!names.blob.empty()) FA_TRY("name upload", hipMemcpyAsync(d_blob, names.blob.data(), names.blob.size(), hipMemcpyHostToDevice, st));
  FA_TRY("name offset upload", hipMemcpyAsync(d_noff, names.off.data(), 8ull * names.off.size(), hipMemcpyHostToDevice, st));
  FA_TRY("statistics", hipMemsetAsync(D.stats, 0, 6 * 8, st));
  D.two = d_two; D.present = d_present; D.blob = d_blob; D.noff = d_noff;
  // ---- segments
  k_fa_win<<<blocks(N), 256, 0, st>>>(D);
  FA_TRY("k_fa_win launch", hipGetLastError());
  FA_SCAN(D.wlen, N, D.wpre);
  FA_SCAN(D.head, N, D.hidx);
  k_fa_ends<<<blocks(N), 256, 0, st>>>(D);
  FA_TRY("k_fa_ends launch", hipGetLastError());
  k_fa_run<<<blocks(N), 256, 0, st>>>(D);
  FA_TRY("k_fa_run launch", hipGetLastError());
  FA_SCAN(D.nonempty, N, D.segpos);
  FA_SCAN(D.kept, N, D.piece_off);
  uint32_t P = 0;
  FA_TRY("piece count", hipMemcpyAsync(&P, D.piece_off + N, 4, hipMemcpyDeviceToHost, st));
  FA_TRY("segments", hipStreamSynchronize(st));
  stats.seg_ms = ms_since(t0);
  t0 = std::chrono::steady_clock::now();
  unsigned long long h_stats[6] = {0, 0, 0, 0, 0, 0};
  if (!P) {   // nothing is kept: the counts of what was dropped are still the call's
    FA_TRY("statistics", hipMemcpyAsync(h_stats, D.stats, sizeof h_stats, hipMemcpyDeviceToHost, st));
    FA_TRY("statistics", hipStreamSynchronize(st));
    stats.dropped = h_stats[2]; stats.bases_dropped = h_stats[3]; stats.segments = h_stats[4];
    return FASTA_OK;
  }
  // ---- pieces: the second block, sized by the pieces
  D.P = P;
  auto lay_b = [&](Carver& c) {
    uint32_t** const per_piece[] = {&D.piece_run, &D.lo_in, &D.lo, &D.hi_in, &D.hi};
    for (uint32_t** q : per_piece) c.take(q, (uint64_t)P + 1);
    c.take(&D.off, (uint64_t)P + 1);
    if (dev_scan_partials(P) > dev_scan_partials(N)) c.take(&d_partial, (uint64_t)dev_scan_partials(P) + 1);
  };
  Carver cb;
  lay_b(cb);
  cb.base = (char*)mem.dev(cb.at);
  FA_MEM(cb.base, "the piece arrays");
  cb.at = 0;
  lay_b(cb);
  k_fa_piece<<<blocks(P), 256, 0, st>>>(D);
  FA_TRY("k_fa_piece launch", hipGetLastError());
  if (int rc = offsets64(D, d_partial, st, err)) return rc;
  k_fa_tgt<<<blocks(n_targets), 256, 0, st>>>(D);
  FA_TRY("k_fa_tgt launch", hipGetLastError());
  uint64_t T = 0;
  FA_TRY("text size", hipMemcpyAsync(&T, D.off + P, 8, hipMemcpyDeviceToHost, st));
  FA_TRY("target ends", hipMemcpyAsync(target_end.data(), D.tgt_end, 8ull * n_targets, hipMemcpyDeviceToHost, st));
  FA_TRY("statistics", hipMemcpyAsync(h_stats, D.stats, sizeof h_stats, hipMemcpyDeviceToHost, st));
  FA_TRY("pieces", hipStreamSynchronize(st));
  stats.records = P; stats.bases = h_stats[1]; stats.dropped = h_stats[2]; stats.bases_dropped = h_stats[3]; stats.segments = h_stats[4];
  stats.targets = h_stats[5];
  stats.piece_ms = ms_since(t0);
  t0 = std::chrono::steady_clock::now();
  // ---- write: chunk c is text [c * cs, (c + 1) * cs), formed in device half c & 1 and copied from there to its place in the pinned block.  The
  // stream orders everything: the kernel of chunk c + 2 starts behind the copy of chunk c, so the whole text is queued at once and awaited once.
  const uint64_t cs = (std::max<uint64_t>(chunk, 1) + 15) / 16 * 16;
  const uint64_t n_chunks = (T + cs - 1) / cs;
  const uint64_t half_bytes = std::min(cs, (T + 15) / 16 * 16);
  char* d_text[2] = {nullptr, nullptr};
  d_text[0] = (char*)mem.dev((n_chunks > 1 ? 2 : 1) * half_bytes);
  FA_MEM(d_text[0], "the text halves");
  d_text[1] = d_text[0] + half_bytes;
  char* const h_text = mem.text(T);
  FA_MEM(h_text, "the pinned text");
  for (uint64_t c = 0; c < n_chunks; c++) {
    const int b = (int)(c & 1);
    const uint64_t x0 = c * cs, x1 = std::min(T, x0 + cs);
    k_fa_write<<<blocks((x1 - x0 + 15) / 16), 256, 0, st>>>(D, x0, x1, d_text[b]);
    FA_TRY("k_fa_write launch", hipGetLastError());
    FA_TRY("text copy", hipMemcpyAsync(h_text + x0, d_text[b], x1 - x0, hipMemcpyDeviceToHost, st));
  }
  FA_TRY("k_fa_write", hipStreamSynchronize(st));
  *text = h_text;
  *text_len = T;
  stats.bytes = T; stats.chunks = n_chunks;
  stats.write_ms = ms_since(t0);
  return FASTA_OK;
}

}  // namespace herro
