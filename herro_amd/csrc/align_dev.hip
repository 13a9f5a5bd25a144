// align_dev.hip — banded Gotoh alignment of overlaps given by coordinates only, one wave64 per record.
//
// Stands in for the base-level step of `minimap2 -cx ava-ont` that `herro inference` runs when it is not given
// --read-alns (mm2.rs:15-30), then applies the reference's fix_cigar (aligners.rs:138-250) and drops a trailing indel.
// The exact specification (scores, band rule, tie order, normalisation) is DESIGN.md §9; tests/align_ref.py restates it
// in numpy and the kernel is held to it bit for bit.
//
// Layout.  The band has W = 128 cells per anti-diagonal d = i + j; lane L holds cells k = 2L and 2L + 1 (i = lo_d + k).
// Every lane keeps, re-indexed to the band of the diagonal being computed, H / I / D of diagonal d - 1, H of d - 2 and
// the two sequence codes of its cells.  A cell needs its neighbours at k - 1 (up, diagonal) and k (left): one DPP
// wave_shr:1 per array.  When the band moves (lo_{d+1} = lo_d + 1) the arrays and the query codes shift down one cell
// (DPP wave_shl:1, the new top query code enters in lane 63); otherwise the target codes shift up one cell (the new
// target code enters in lane 0).  The codes that may enter are read before the diagonal is computed (one uniform load
// each), so the read is off the decision's path.
//
// -inf is a sentinel NEG = -2^30.  No cell is masked: cells with i < 0 or j < 0 only ever see -inf-ish inputs and stay
// below NEG / 2 (n + m <= 2^25 keeps the drift inside int32), cells with i > n or j > m feed no cell of the matrix, and the
// band decision tests its two cells against the matrix explicitly.  Finite scores are >= -6 (n + m) > NEG / 2.
//
// Traceback bits per cell: bits 0-1 the source of H (0 diagonal, 1 I, 2 D), bit 2 "I opened" (from H), bit 3 "D opened";
// one byte per lane, one coalesced 64-byte row per anti-diagonal, plus lo_d (4 B) — written to the record's scratch.
// The walk back from (n, m) stages 64 rows at a time in the LDS; every lane walks the same path (uniform control flow,
// broadcast LDS reads) and lane 0 writes the ops.  fix_cigar, the trim and the score then stream once over the op list.
#include "align_dev.h"
#include "overlap_dev.h"

namespace herro {
namespace {

constexpr int W = ALIGN_W;
constexpr int32_t NEG = -(1 << 30);
constexpr int32_t FINITE = -(1 << 29);   // values below this are -inf

// lane L receives lane L - 1's v (lane 0: fill) / lane L + 1's v (lane 63: fill)
__device__ __forceinline__ int32_t from_below(int32_t v, int32_t fill) {
  return __builtin_amdgcn_update_dpp(fill, v, 0x138, 0xf, 0xf, false);   // wave_shr:1
}
__device__ __forceinline__ int32_t from_above(int32_t v, int32_t fill) {
  return __builtin_amdgcn_update_dpp(fill, v, 0x130, 0xf, 0xf, false);   // wave_shl:1
}
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// 2-bit codes of T or Q (strand 1: reversed and complemented, as k_cols stages a reverse-strand query)
struct Seq {
  const uint64_t* w;
  int32_t start, len;
  uint32_t rev;
  __device__ __forceinline__ uint32_t at(int32_t x) const {   // 0 outside [0, len): such cells never reach the matrix
    if (x < 0 || x >= len) return 0;
    const uint32_t p = (uint32_t)(rev ? start + len - 1 - x : start + x);
    return ((uint32_t)(w[p >> 5] >> ((p & 31u) * 2u)) & 3u) ^ (rev ? 3u : 0u);
  }
};

// one cell: returns H, writes I, D and the traceback nibble
__device__ __forceinline__ int32_t cell(int32_t up_h, int32_t up_i, int32_t left_h, int32_t left_d, int32_t diag_h,
                                        uint32_t qc, uint32_t tc, int32_t& I, int32_t& Dv, uint32_t& nib) {
  const int32_t io = up_h - 6, ie = up_i - 2, dop = left_h - 6, de = left_d - 2;
  I = max(io, ie);
  Dv = max(dop, de);
  const int32_t sd = diag_h + (qc == tc ? 2 : -4);
  const int32_t H = max(sd, max(I, Dv));
  const uint32_t src = H == sd ? 0u : (H == I ? 1u : 2u);
  nib = src | (io >= ie ? 4u : 0u) | (dop >= de ? 8u : 0u);
  return H;
}

// ---- fix_cigar (aligners.rs:138-250), the trailing-indel trim and the gap sums, streamed once over an op list -----------------------
// One definition for k_align (the ops its traceback left) and k_mirror (another record's ops, swapped and read backwards): F(j) is
// op j of cnt >= 1 ops, each fetched once and in order, two ahead of the op being looked at.
// Left shift: op j is final once op j + 1 has been looked at, so it goes straight on into the retain / merge stage, which writes the
// result to dst[0 ..): at most one op per op read, and op j is written only after F(j + 1) has been fetched.  Every lane runs the same
// stream (uniform control flow); lane 0 writes.
struct Fixed {
  uint32_t nout;                     // final ops in dst[0 .. nout)
  uint32_t first_t, last_t;          // their first and last type (3: there is none)
  uint32_t tsh0, qsh0, tsh1, qsh1;   // bases the dropped leading / trailing indel consumed
  int32_t gap_in, gap_fin;           // sum of 4 + 2 len over the I / D ops read / written
  bool type3;                        // an op of type 3 was read
};

template <class Fetch>
__device__ __forceinline__ Fixed fix_stream(Fetch F, uint32_t cnt, const Seq& T, const Seq& Q, uint32_t* dst, int L) {
  uint32_t nout = 0;
  bool is_start = true, have_last = false, type3 = false;
  uint32_t last = 0, first_t = 3, last_t = 3;
  uint32_t tsh0 = 0, qsh0 = 0, tsh1 = 0, qsh1 = 0;
  int32_t gap_in = 0, gap_fin = 0;
  auto write = [&](uint32_t op) {
    if (L == 0) dst[nout] = op;
    ++nout;
    const uint32_t t = op & 3u;
    if (first_t == 3) first_t = t;
    last_t = t;
    if (t) gap_fin += 4 + 2 * (int32_t)(op >> 2);
  };
  auto stage2 = [&](uint32_t op) {
    const uint32_t t = op & 3u, len = op >> 2;
    if (is_start) {
      if (t == 0 && len == 0) return;
      is_start = false;
      if (t == 1) { qsh0 = len; return; }
      if (t == 2) { tsh0 = len; return; }
    } else if (len == 0) {
      return;
    }
    if (have_last && (last & 3u) == t) { last += len << 2; return; }
    if (have_last) write(last);
    last = op; have_last = true;
  };
  int32_t tpos = 0, qpos = 0;
  uint32_t prev = 0, cur = F(0), nxt = cnt > 1 ? F(1) : 0u;
  for (uint32_t j = 0; j < cnt; ++j) {
    const uint32_t t = cur & 3u;
    const int32_t len = (int32_t)(cur >> 2);
    if (t == 0) {
      tpos += len; qpos += len;
    } else {
      type3 |= t == 3u;
      gap_in += 4 + 2 * len;
      if (j > 0 && j + 1 < cnt && (prev & 3u) == 0 && (nxt & 3u) == 0) {
        const int32_t prev_len = (int32_t)(prev >> 2);
        int32_t l = 0;
        if (t == 1) {
          while (l < prev_len && Q.at(qpos - 1 - l) == Q.at(qpos + len - 1 - l)) ++l;
        } else {
          while (l < prev_len && T.at(tpos - 1 - l) == T.at(tpos + len - 1 - l)) ++l;
        }
        if (l > 0) {
          prev -= (uint32_t)l << 2;
          nxt += (uint32_t)l << 2;
          tpos -= l; qpos -= l;
        }
      }
      if (t == 1) qpos += len; else tpos += len;
    }
    if (j > 0) stage2(prev);
    prev = cur; cur = nxt;
    nxt = j + 2 < cnt ? F(j + 2) : 0u;
  }
  stage2(prev);
  if (have_last) {   // a trailing indel is dropped too
    const uint32_t t = last & 3u;
    if (t == 1) qsh1 = last >> 2;
    else if (t == 2) tsh1 = last >> 2;
    else write(last);
  }
  return Fixed{nout, first_t, last_t, tsh0, qsh0, tsh1, qsh1, gap_in, gap_fin, type3};
}

__global__ __launch_bounds__(64) void k_align(const uint64_t* __restrict__ words, const AlignIn* __restrict__ in,
                                              AlignOut* __restrict__ out, uint8_t* __restrict__ scr,
                                              uint32_t* __restrict__ dense, uint32_t* __restrict__ count) {
  __shared__ __attribute__((aligned(16))) uint8_t s_rows[64 * 64];
  __shared__ int32_t s_lo[64];
  const uint32_t r = blockIdx.x;
  const int L = (int)threadIdx.x;
  const AlignIn a = in[r];
  const int32_t n = (int32_t)a.n, m = (int32_t)a.m, D = n + m;
  const Seq T{words + a.t_woff, (int32_t)a.t0, m, 0u}, Q{words + a.q_woff, (int32_t)a.q0, n, a.strand};
  uint8_t* rows = scr + a.scr_off;
  int32_t* lo_arr = (int32_t*)(rows + (size_t)(D + 1) * 64);
  uint32_t* ops = (uint32_t*)(lo_arr + (D + 1));
  const uint32_t C = (uint32_t)D + 1;
  auto fail = [&]() {
    if (L == 0) {
      AlignOut f{INT32_MIN, 0u, 0u, 1u, 0u, 0u, 0u, 0u};
      out[r] = f;
    }
  };
  if (D == 0) { fail(); return; }

  // ---- sweep ------------------------------------------------------------------------------------------------------
  int32_t lo = -W / 2;
  const int k0 = 2 * L, k1 = 2 * L + 1;
  // diagonal 0 (only (0, 0) is a cell: H = 0 at k = W / 2) and diagonal -1; the band does not move after d = 0 (both
  // decision cells lie outside the matrix)
  int32_t h1a = k0 == W / 2 ? 0 : NEG, h1b = NEG, i1a = NEG, i1b = NEG, d1a = NEG, d1b = NEG, h2a = NEG, h2b = NEG;
  if (L == 0) lo_arr[0] = lo;
  // (uniform) what lane 0 reads below the band's bottom cell: H / I of d - 1 and H of d - 2 at i = lo - 1.  That cell lay in the band of
  // its own diagonal if the band has moved since (it was the bottom cell then), and is outside it (-inf) otherwise.
  int32_t h1f = NEG, i1f = NEG, h2f = NEG;
  uint32_t qa = Q.at(lo + k0 - 1), qb = Q.at(lo + k1 - 1);   // Q[i - 1]
  uint32_t ta = T.at(-lo - k0), tb = T.at(-lo - k1);         // T[j - 1] on d = 1
  int32_t hend = NEG;
  bool in_band = false;
  for (int32_t d = 1; d <= D; ++d) {
    const uint32_t q_in = Q.at(lo + W - 1);   // enters at the top if the band moves
    const uint32_t t_in = T.at(d - lo);       // enters at the bottom if it does not
    const int32_t h1m = from_below(h1b, h1f), i1m = from_below(i1b, i1f), h2m = from_below(h2b, h2f);
    int32_t Ia, Da, Ib, Db;
    uint32_t na, nb;
    const int32_t Ha = cell(h1m, i1m, h1a, d1a, h2m, qa, ta, Ia, Da, na);
    const int32_t Hb = cell(h1a, i1a, h1b, d1b, h2a, qb, tb, Ib, Db, nb);
    rows[(size_t)d * 64 + L] = (uint8_t)(na | (nb << 4));
    if (L == 0) lo_arr[d] = lo;
    if (d == D) {
      const int32_t k = n - lo;
      in_band = k >= 0 && k < W;
      const int32_t sel = (k & 1) ? Hb : Ha;
      hend = __shfl(sel, in_band ? (k >> 1) : 0, 64);
      break;
    }
    const int32_t top = __builtin_amdgcn_readlane(Hb, 63), bot = __builtin_amdgcn_readlane(Ha, 0);
    const int32_t it = lo + W - 1, jt = d - it, ib = lo, jb = d - lo;
    const int32_t vt = (it >= 0 && it <= n && jt >= 0 && jt <= m && top >= FINITE) ? top : NEG;
    const int32_t vb = (ib >= 0 && ib <= n && jb >= 0 && jb <= m && bot >= FINITE) ? bot : NEG;
    if (vt > vb) {   // lo_{d+1} = lo_d + 1: every array moves down one cell
      h2f = __builtin_amdgcn_readlane(h1a, 0); h1f = bot; i1f = __builtin_amdgcn_readlane(Ia, 0);
      h2a = h1b; h2b = from_above(h1a, NEG);
      h1a = Hb; h1b = from_above(Ha, NEG);
      i1a = Ib; i1b = from_above(Ia, NEG);
      d1a = Db; d1b = from_above(Da, NEG);
      const uint32_t qn = (uint32_t)from_above((int32_t)qa, (int32_t)q_in);
      qa = qb; qb = qn;
      ++lo;
    } else {         // lo_{d+1} = lo_d: the target codes move up one cell
      h2f = h1f; h1f = NEG; i1f = NEG;
      h2a = h1a; h2b = h1b;
      h1a = Ha; h1b = Hb;
      i1a = Ia; i1b = Ib;
      d1a = Da; d1b = Db;
      const uint32_t tn = (uint32_t)from_below((int32_t)tb, (int32_t)t_in);
      tb = ta; ta = tn;
    }
  }
  if (!in_band || hend < FINITE) { fail(); return; }
  wave_sync();

  // ---- traceback: ops in reverse order into ops[C - 1 - cnt] ------------------------------------------------------
  int32_t d = D, i = n, mat = 0;
  uint32_t cnt = 0;
  int32_t run_t = -1, run_len = 0, gap_dp = 0;
  bool bad = false;
  auto emit = [&](int32_t t, int32_t len) {
    if (L == 0) ops[C - 1 - cnt] = ((uint32_t)len << 2) | (uint32_t)t;
    ++cnt;
    if (t) gap_dp += 4 + 2 * len;
  };
  while (d > 0 && !bad) {
    const int32_t blo = max(d - 63, 0);
    const int32_t rr = blo + L;
    if (rr <= d) {
      const uint4* src = (const uint4*)(rows + (size_t)rr * 64);
      uint4* dst = (uint4*)(s_rows + L * 64);
      const uint4 x0 = src[0], x1 = src[1], x2 = src[2], x3 = src[3];
      dst[0] = x0; dst[1] = x1; dst[2] = x2; dst[3] = x3;
      s_lo[L] = lo_arr[rr];
    }
    wave_sync();
    while (d >= blo && d > 0) {
      const int32_t k = i - s_lo[d - blo];
      if (k < 0 || k >= W) { bad = true; break; }
      const uint32_t nib = (s_rows[(d - blo) * 64 + (k >> 1)] >> ((k & 1) * 4)) & 15u;
      int32_t t;
      if (mat == 0) {
        const uint32_t s = nib & 3u;
        if (s) { mat = (int32_t)s; continue; }   // the same cell, in I or D
        t = 0; i -= 1; d -= 2;
      } else if (mat == 1) {
        t = 1; i -= 1; d -= 1;
        if (nib & 4u) mat = 0;
      } else {
        t = 2; d -= 1;
        if (nib & 8u) mat = 0;
      }
      if (t == run_t) ++run_len;
      else {
        if (run_len) emit(run_t, run_len);
        run_t = t; run_len = 1;
      }
    }
    wave_sync();   // every lane is done with this block before the next one overwrites it
  }
  if (bad || d != 0 || i != 0 || mat != 0) { fail(); return; }
  if (run_len) emit(run_t, run_len);
  wave_sync();

  // ---- fix_cigar (aligners.rs:138-250), streamed: F[j] = ops[C - cnt + j] --------------------------------------------
  // The result goes to ops[0 ..), never ahead of what is still to be read: nout <= j < C - cnt + j.
  const uint32_t* Fp = ops + (C - cnt);
  const Fixed fx = fix_stream([&](uint32_t j) { return Fp[j]; }, cnt, T, Q, ops, L);
  if (fx.nout == 0 || fx.first_t != 0 || fx.last_t != 0) { fail(); return; }
  const uint32_t nout = fx.nout;

  // ---- result: ops to the dense output, the record's header -------------------------------------------------------
  uint32_t base = 0;
  if (L == 0) base = atomicAdd(count, nout);
  base = (uint32_t)__shfl((int32_t)base, 0, 64);
  wave_sync();
  for (uint32_t x = (uint32_t)L; x < nout; x += 64) dense[base + x] = ops[x];
  if (L == 0) {
    AlignOut o{hend + gap_dp - fx.gap_fin, nout, base, 0u, fx.tsh0, fx.qsh0, fx.tsh1, fx.qsh1};
    out[r] = o;
  }
}

// ---- k_mirror: the alignment of (q, t) from the final ops of (t, q) (DESIGN.md §9 "Mirrored records"; tests/mirror_ref.py) ---------
// One wave64 per record, no sweep: the source's ops are read through F[j] = swap(src[strand ? c - 1 - j : j]) (I <-> D; backwards on the
// reverse strand, no reversed copy is made) and go through fix_stream against the swapped sequences — on the reverse strand the reversal
// turns left-most indels into right-most ones, and a target's pileup needs them placed by one rule.  The result goes to the record's own
// reservation of c slots (the host's prefix sum of the sources' n_ops; the final count may be smaller): no atomic counter, no LDS, no
// scratch, every loop bounded by c or by an op's length.  Ops that do not add up to the spans read codes of 0 (Seq::at) and give a
// meaningless but memory-safe result.
__global__ __launch_bounds__(64) void k_mirror(const uint64_t* __restrict__ words, const MirrorIn* __restrict__ in,
                                               AlignOut* __restrict__ out, uint32_t* store) {
  const uint32_t r = blockIdx.x;
  const int L = (int)threadIdx.x;
  const MirrorIn a = in[r];
  auto fail = [&]() {
    if (L == 0) {
      AlignOut f{INT32_MIN, 0u, 0u, 1u, 0u, 0u, 0u, 0u};
      out[r] = f;
    }
  };
  const uint32_t c = a.c, rev = a.strand;
  if (c == 0) { fail(); return; }   // a failed source
  const Seq T{words + a.t_woff, (int32_t)a.t0, (int32_t)a.m, 0u}, Q{words + a.q_woff, (int32_t)a.q0, (int32_t)a.n, rev};
  const uint32_t* src = store + a.src_off;
  const Fixed fx = fix_stream([&](uint32_t j) {
    const uint32_t op = src[rev ? c - 1 - j : j];
    const uint32_t t = op & 3u;
    return (t == 1u || t == 2u) ? op ^ 3u : op;
  }, c, T, Q, store + a.dst_off, L);
  if (fx.type3 || fx.nout == 0 || fx.first_t != 0 || fx.last_t != 0) { fail(); return; }
  if (L == 0) {
    AlignOut o{a.score + fx.gap_in - fx.gap_fin, fx.nout, 0u, 0u, fx.tsh0, fx.qsh0, fx.tsh1, fx.qsh1};
    out[r] = o;
  }
}

// ---- k_extend: ends-free extension of one end of an overlap (tests/extend_ref.py) -----------------------------
// One wave64 per (record, side).  The sweep is k_align's — the same registers, DPP neighbour reads, band decision and shifts,
// the same cell() (its traceback nibble is dropped) — over Q' x T', the bases behind (in front of) the aligned span read away
// from it.  Nothing is written per diagonal: no traceback rows, no LDS, no scratch.  Every lane keeps the best (H, d, i) of its
// own cells; a cell counts when 1 <= i <= n and 1 <= j <= m (cells past n or m hold finite garbage, k_align never masks them)
// and replaces the lane's best only when strictly greater — the best starts at 0, so a cell that wins is finite.  Per lane the
// lower cell is looked at first and diagonals come in order, so the lane holds the earliest diagonal and the smallest i of its
// maximum; the wave's result is max H, then min d, then min i over the lanes.
// Stop rule: after every diagonal with d % 16 == 0, stop when max(M_d, M_{d-1}) < best - zdrop, M_d the maximum over the band's
// in-matrix cells of diagonal d (0 <= i <= n, 0 <= j <= m; -inf cells are below FINITE and lose to every finite threshold).
// The lane maxima of diagonals 15 and 0 (mod 16) are the only ones taken, and the wave is reduced once per 16 diagonals.
__device__ __forceinline__ int32_t wave_max(int32_t v) {
  const int32_t ident = INT32_MIN;
  v = max(v, __builtin_amdgcn_update_dpp(ident, v, 0x111, 0xf, 0xf, false));   // row_shr:1
  v = max(v, __builtin_amdgcn_update_dpp(ident, v, 0x112, 0xf, 0xf, false));   // row_shr:2
  v = max(v, __builtin_amdgcn_update_dpp(ident, v, 0x114, 0xf, 0xf, false));   // row_shr:4
  v = max(v, __builtin_amdgcn_update_dpp(ident, v, 0x118, 0xf, 0xf, false));   // row_shr:8 -> lane 15 of a row holds the row
  v = max(v, __builtin_amdgcn_update_dpp(ident, v, 0x142, 0xa, 0xf, false));   // row_bcast:15 into rows 1 and 3
  v = max(v, __builtin_amdgcn_update_dpp(ident, v, 0x143, 0xc, 0xf, false));   // row_bcast:31 into rows 2 and 3
  return __builtin_amdgcn_readlane(v, 63);
}

__global__ __launch_bounds__(64) void k_extend(const uint64_t* __restrict__ words, const ExtIn* __restrict__ in,
                                               ExtOut* __restrict__ out, uint32_t zdrop) {
  const uint32_t r = blockIdx.x;
  const int L = (int)threadIdx.x;
  const ExtIn a = in[r];
  const int32_t n = (int32_t)a.n, m = (int32_t)a.m, D = n + m;
  int32_t bh = 0, bd = 0, bi = 0;   // this lane's best cell
  int32_t d_stop = 0;
  if (n > 0 && m > 0) {             // (uniform) an empty flank: zeros
    const Seq T{words + a.t_woff, (int32_t)a.t0, m, a.trev}, Q{words + a.q_woff, (int32_t)a.q0, n, a.qrev};
    const int32_t zd = (int32_t)min(zdrop, 1u << 29);   // finite H > -2^24: above 2^29 nothing finite is ever below best - zdrop
    int32_t lo = -W / 2;
    const int k0 = 2 * L, k1 = 2 * L + 1;
    int32_t h1a = k0 == W / 2 ? 0 : NEG, h1b = NEG, i1a = NEG, i1b = NEG, d1a = NEG, d1b = NEG, h2a = NEG, h2b = NEG;
    int32_t h1f = NEG, i1f = NEG, h2f = NEG;   // (uniform) below the band's bottom cell, as in k_align
    uint32_t qa = Q.at(lo + k0 - 1), qb = Q.at(lo + k1 - 1);   // Q'[i - 1]
    uint32_t ta = T.at(-lo - k0), tb = T.at(-lo - k1);         // T'[j - 1] on d = 1
    int32_t mprev = NEG;
    for (int32_t d = 1; d <= D; ++d) {
      const uint32_t q_in = Q.at(lo + W - 1);   // enters at the top if the band moves
      const uint32_t t_in = T.at(d - lo);       // enters at the bottom if it does not
      const int32_t h1m = from_below(h1b, h1f), i1m = from_below(i1b, i1f), h2m = from_below(h2b, h2f);
      int32_t Ia, Da, Ib, Db;
      uint32_t na, nb;
      const int32_t Ha = cell(h1m, i1m, h1a, d1a, h2m, qa, ta, Ia, Da, na);
      const int32_t Hb = cell(h1a, i1a, h1b, d1b, h2a, qb, tb, Ib, Db, nb);
      d_stop = d;
      // candidates of this diagonal: max(1, d - m) <= i <= min(n, d - 1)
      const int32_t c_lo = max(1, d - m);
      const uint32_t c_cnt = (uint32_t)max(min(n, d - 1) - c_lo + 1, 0);
      const uint32_t ca = (uint32_t)(lo + k0 - c_lo);
      if (ca < c_cnt && Ha > bh) { bh = Ha; bd = d; bi = lo + k0; }
      if (ca + 1u < c_cnt && Hb > bh) { bh = Hb; bd = d; bi = lo + k1; }
      const int32_t ph = d & 15;
      if (ph == 15 || ph == 0) {   // (uniform) the in-matrix cells of this diagonal: max(0, d - m) <= i <= min(n, d)
        const int32_t m_lo = max(0, d - m);
        const uint32_t m_cnt = (uint32_t)(min(n, d) - m_lo + 1);
        const uint32_t ma = (uint32_t)(lo + k0 - m_lo);
        const int32_t mx = max(ma < m_cnt ? Ha : NEG, ma + 1u < m_cnt ? Hb : NEG);
        if (ph == 15) {
          mprev = mx;
        } else if (wave_max(max(mx, mprev)) < wave_max(bh) - zd) {
          break;
        }
      }
      if (d == D) break;
      const int32_t top = __builtin_amdgcn_readlane(Hb, 63), bot = __builtin_amdgcn_readlane(Ha, 0);
      const int32_t it = lo + W - 1, jt = d - it, ib = lo, jb = d - lo;
      const int32_t vt = (it >= 0 && it <= n && jt >= 0 && jt <= m && top >= FINITE) ? top : NEG;
      const int32_t vb = (ib >= 0 && ib <= n && jb >= 0 && jb <= m && bot >= FINITE) ? bot : NEG;
      if (vt > vb) {   // lo_{d+1} = lo_d + 1: every array moves down one cell
        h2f = __builtin_amdgcn_readlane(h1a, 0); h1f = bot; i1f = __builtin_amdgcn_readlane(Ia, 0);
        h2a = h1b; h2b = from_above(h1a, NEG);
        h1a = Hb; h1b = from_above(Ha, NEG);
        i1a = Ib; i1b = from_above(Ia, NEG);
        d1a = Db; d1b = from_above(Da, NEG);
        const uint32_t qn = (uint32_t)from_above((int32_t)qa, (int32_t)q_in);
        qa = qb; qb = qn;
        ++lo;
      } else {         // lo_{d+1} = lo_d: the target codes move up one cell
        h2f = h1f; h1f = NEG; i1f = NEG;
        h2a = h1a; h2b = h1b;
        h1a = Ha; h1b = Hb;
        i1a = Ia; i1b = Ib;
        d1a = Da; d1b = Db;
        const uint32_t tn = (uint32_t)from_below((int32_t)tb, (int32_t)t_in);
        tb = ta; ta = tn;
      }
    }
  }
  // max H, then the earliest diagonal, then the smallest i (every lane starts from (0, 0, 0): no extension)
  const int32_t best = wave_max(bh);
  const int32_t dsel = -wave_max(bh == best ? -bd : INT32_MIN);
  const int32_t isel = -wave_max(bh == best && bd == dsel ? -bi : INT32_MIN);
  if (L == 0) {
    ExtOut o{best, (uint32_t)isel, (uint32_t)(dsel - isel), (uint32_t)d_stop, {0u, 0u, 0u, 0u}};
    out[r] = o;
  }
}

// ---- the extension of records that are on the device (herro_find_overlap_pairs): herro_extend_overlaps' two host loops, one thread per record ----
// left: the target below tstart read downwards; the oriented query in front of the span read backwards.  right: the target from tend upwards; the
// oriented query behind the span.  (T rev = 1, Q rev = !strand on the left; 0 and strand on the right.)
__global__ __launch_bounds__(256) void k_ext_sides(const OvlRec* __restrict__ rec, uint32_t n, const uint64_t* __restrict__ word_off,
                                                   const uint64_t* __restrict__ base_off, uint32_t max_ext, ExtIn* __restrict__ sides) {
  const uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (x >= n) return;
  const OvlRec a = rec[x];
  const uint64_t tw = word_off[a.tid], qw = word_off[a.qid];
  const uint32_t tlen = (uint32_t)(base_off[a.tid + 1] - base_off[a.tid]), qlen = (uint32_t)(base_off[a.qid + 1] - base_off[a.qid]);
  const uint32_t t_below = a.tstart, t_above = tlen - a.tend;
  const uint32_t q_below = a.qstart, q_above = qlen - a.qend;
  const uint32_t ml = min(t_below, max_ext), nl = min(a.strand ? q_above : q_below, max_ext);
  sides[2 * x] = ExtIn{tw, qw, a.tstart - ml, ml, a.strand ? a.qend : a.qstart - nl, nl, 1u, a.strand ? 0u : 1u};
  const uint32_t mr = min(t_above, max_ext), nr = min(a.strand ? q_below : q_above, max_ext);
  sides[2 * x + 1] = ExtIn{tw, qw, a.tend, mr, a.strand ? a.qstart - nr : a.qend, nr, 0u, a.strand};
}

// the two results of every record into its coordinates; ext[x] = t_left, q_left, t_right, q_right; scores[x] = left, right
__global__ __launch_bounds__(256) void k_ext_fold(OvlRec* __restrict__ rec, uint32_t n, const ExtOut* __restrict__ res, uint32_t* __restrict__ ext,
                                                  int32_t* __restrict__ scores) {
  const uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (x >= n) return;
  OvlRec a = rec[x];
  const ExtOut l = res[2 * x], r = res[2 * x + 1];
  a.tstart -= l.j; a.tend += r.j;
  if (a.strand == 0) { a.qstart -= l.i; a.qend += r.i; }
  else { a.qend += l.i; a.qstart -= r.i; }
  rec[x] = a;
  ext[4 * x] = l.j; ext[4 * x + 1] = l.i; ext[4 * x + 2] = r.j; ext[4 * x + 3] = r.i;
  scores[2 * x] = l.score;
  scores[2 * x + 1] = r.score;
}

}  // namespace

void launch_ext_sides(const OvlRec* d_rec, uint32_t n_rec, const uint64_t* d_word_off, const uint64_t* d_base_off, uint32_t max_ext, ExtIn* d_sides,
                      hipStream_t st) {
  if (n_rec == 0) return;
  hipLaunchKernelGGL(k_ext_sides, dim3((n_rec + 255) / 256), dim3(256), 0, st, d_rec, n_rec, d_word_off, d_base_off, max_ext, d_sides);
}

void launch_ext_fold(OvlRec* d_rec, uint32_t n_rec, const ExtOut* d_res, uint32_t* d_ext, int32_t* d_scores, hipStream_t st) {
  if (n_rec == 0) return;
  hipLaunchKernelGGL(k_ext_fold, dim3((n_rec + 255) / 256), dim3(256), 0, st, d_rec, n_rec, d_res, d_ext, d_scores);
}

void launch_extend(const uint64_t* d_words, const ExtIn* d_in, ExtOut* d_out, uint32_t zdrop, uint32_t n_sides, hipStream_t st) {
  if (n_sides == 0) return;
  hipLaunchKernelGGL(k_extend, dim3(n_sides), dim3(64), 0, st, d_words, d_in, d_out, zdrop);
}

void launch_mirror(const uint64_t* d_words, const MirrorIn* d_in, AlignOut* d_out, uint32_t* d_store, uint32_t n_rec, hipStream_t st) {
  if (n_rec == 0) return;
  hipLaunchKernelGGL(k_mirror, dim3(n_rec), dim3(64), 0, st, d_words, d_in, d_out, d_store);
}

void launch_align(const uint64_t* d_words, const AlignIn* d_in, AlignOut* d_out, uint8_t* d_scr, uint32_t* d_dense,
                  uint32_t* d_count, uint32_t n_rec, hipStream_t st) {
  if (n_rec == 0) return;
  hipLaunchKernelGGL(k_align, dim3(n_rec), dim3(64), 0, st, d_words, d_in, d_out, d_scr, d_dense, d_count);
}

}  // namespace herro
