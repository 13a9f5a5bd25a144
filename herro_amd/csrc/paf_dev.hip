// paf_dev.hip — PAF lines from device-resident ops (paf_dev.h; specification: DESIGN.md §12, tests/paf_ref.py and the host formatter of
// frontend_api.hip, which the kernels equal byte for byte).
//   k_paf_len    one wave64 per row: the lanes stride over the row's ops and sum digits(len) + 1, the M lengths and all lengths; lane 0 adds the
//                fixed part of the line and writes its byte count and the two sums.
//   (scan)       line offsets of a chunk: the shared exclusive scan of u32 (dev_scan_u32, scan_sort_dev.h), hence chunks below 2^32 bytes of text.
//   k_paf_write  one wave64 per row: the names by all lanes, the eight numbers by lanes 0 .. 7, the separators by lane 8, then the ops in blocks
//                of 64 — lane l takes op base + l, its place is a wave prefix sum of digits + 1 carried across blocks in a scalar — and every lane
//                stores its <= 11 bytes.  Plain byte stores; no LDS, no atomics.
// Both kernels derive a line's layout from head_of(), so the count and the text cannot disagree; k_paf_write also keeps every store inside
// [line_off[row], line_off[row + 1]).
#include "paf_dev.h"

namespace herro {
namespace {

__device__ inline uint32_t dec_digits(uint32_t v) {
  return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) + (v >= 100000000u) +
         (v >= 1000000000u);
}
__device__ inline uint32_t dec_digits64(uint64_t v) {
  if (v <= 0xffffffffull) return dec_digits((uint32_t)v);
  uint32_t k = 1;
  while (v >= 10) { v /= 10; k++; }
  return k;
}
__device__ inline void put_dec(char* p, uint32_t v, uint32_t nd) {
  for (uint32_t i = nd; i-- > 0;) { p[i] = (char)('0' + v % 10u); v /= 10u; }
}
__device__ inline void put_dec64(char* p, uint64_t v, uint32_t nd) {
  for (uint32_t i = nd; i-- > 0;) { p[i] = (char)('0' + (uint32_t)(v % 10ull)); v /= 10ull; }
}

// Where the fields of a line begin, from its start: qname at 0, then a tab behind every field.
struct Head {
  uint64_t q0, t0;          // the names' first bytes in the blob
  uint32_t qn, tn;          // their lengths
  uint32_t at_num[8];       // qlen qstart qend | tlen tstart tend mbases blocklen
  uint32_t nd[8];
  uint32_t at_strand, at_tname, at_255, at_cigar;
};
__device__ inline uint64_t head_of(const PafRow& r, const PafSums& s, const uint64_t* __restrict__ name_off, Head& h) {
  h.q0 = name_off[r.qid]; h.qn = (uint32_t)(name_off[r.qid + 1] - h.q0);
  h.t0 = name_off[r.tid]; h.tn = (uint32_t)(name_off[r.tid + 1] - h.t0);
  h.nd[0] = dec_digits(r.qlen); h.nd[1] = dec_digits(r.qstart); h.nd[2] = dec_digits(r.qend);
  h.nd[3] = dec_digits(r.tlen); h.nd[4] = dec_digits(r.tstart); h.nd[5] = dec_digits(r.tend);
  h.nd[6] = dec_digits64(s.mbases); h.nd[7] = dec_digits64(s.blocklen);
  uint64_t at = (uint64_t)h.qn + 1;
#pragma unroll
  for (int k = 0; k < 3; k++) { h.at_num[k] = (uint32_t)at; at += h.nd[k] + 1; }
  h.at_strand = (uint32_t)at; at += 2;
  h.at_tname = (uint32_t)at; at += (uint64_t)h.tn + 1;
#pragma unroll
  for (int k = 3; k < 8; k++) { h.at_num[k] = (uint32_t)at; at += h.nd[k] + 1; }
  h.at_255 = (uint32_t)at; at += 4;          // "255\t"
  h.at_cigar = (uint32_t)(at + 5);           // "cg:Z:"
  return at + 5;                             // (64 bits: two names of 2^32 - 1 bytes do not wrap the count)
}

template <typename T>
__device__ inline T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void k_paf_len(const PafRow* __restrict__ rows, const uint32_t* __restrict__ ops, const uint64_t* __restrict__ name_off,
                                                 uint32_t n, uint32_t* __restrict__ line_bytes, PafSums* __restrict__ sums) {
  const uint32_t row = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (row >= n) return;
  const PafRow r = rows[row];
  unsigned long long tb = 0, mb = 0, bl = 0;
  for (uint64_t x = lane; x < r.n_ops; x += 64) {
    const uint32_t op = ops[r.op_off + x], len = op >> 2;
    tb += dec_digits(len) + 1u;
    bl += len;
    if ((op & 3u) == 0) mb += len;
  }
  tb = wave_sum(tb); mb = wave_sum(mb); bl = wave_sum(bl);
  if (lane != 0) return;
  const PafSums s{mb, bl};
  sums[row] = s;
  if (r.n_ops == 0) { line_bytes[row] = 0; return; }
  Head h;
  const uint64_t total = head_of(r, s, name_off, h) + tb + 1;   // ... and the newline
  line_bytes[row] = total >= PAF_LINE_TOO_LONG ? PAF_LINE_TOO_LONG : (uint32_t)total;
}

__global__ __launch_bounds__(256) void k_paf_write(const PafRow* __restrict__ rows, const uint32_t* __restrict__ ops, const char* __restrict__ names,
                                                   const uint64_t* __restrict__ name_off, const uint32_t* __restrict__ line_off,
                                                   const PafSums* __restrict__ sums, uint32_t n, char* __restrict__ text, uint64_t cap) {
  const uint32_t row = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (row >= n) return;
  const PafRow r = rows[row];
  const uint32_t o0 = line_off[row], o1 = line_off[row + 1];
  if (r.n_ops == 0 || o1 <= o0 || o1 > cap) return;
  const uint32_t line = o1 - o0;
  const PafSums s = sums[row];
  Head h;
  if (head_of(r, s, name_off, h) + 1 > line) return;
  char* const p = text + o0;
  for (uint32_t i = lane; i < h.qn; i += 64) p[i] = names[h.q0 + i];
  for (uint32_t i = lane; i < h.tn; i += 64) p[h.at_tname + i] = names[h.t0 + i];
  if (lane < 8) {
    // (selects, not an indexed array: the fields stay in registers)
    const uint32_t at = lane == 0 ? h.at_num[0] : lane == 1 ? h.at_num[1] : lane == 2 ? h.at_num[2] : lane == 3 ? h.at_num[3] : lane == 4 ? h.at_num[4]
                        : lane == 5 ? h.at_num[5] : lane == 6 ? h.at_num[6] : h.at_num[7];
    const uint32_t nd = lane == 0 ? h.nd[0] : lane == 1 ? h.nd[1] : lane == 2 ? h.nd[2] : lane == 3 ? h.nd[3] : lane == 4 ? h.nd[4]
                        : lane == 5 ? h.nd[5] : lane == 6 ? h.nd[6] : h.nd[7];
    if (lane < 6) {
      const uint32_t v = lane == 0 ? r.qlen : lane == 1 ? r.qstart : lane == 2 ? r.qend : lane == 3 ? r.tlen : lane == 4 ? r.tstart : r.tend;
      put_dec(p + at, v, nd);
    } else {
      put_dec64(p + at, lane == 6 ? s.mbases : s.blocklen, nd);
    }
    p[at + nd] = '\t';
  } else if (lane == 8) {
    p[h.qn] = '\t';
    p[h.at_strand] = r.strand ? '-' : '+';
    p[h.at_strand + 1] = '\t';
    p[h.at_tname + h.tn] = '\t';
    p[h.at_255] = '2'; p[h.at_255 + 1] = '5'; p[h.at_255 + 2] = '5'; p[h.at_255 + 3] = '\t';
    p[h.at_255 + 4] = 'c'; p[h.at_255 + 5] = 'g'; p[h.at_255 + 6] = ':'; p[h.at_255 + 7] = 'Z'; p[h.at_255 + 8] = ':';
    p[line - 1] = '\n';
  }
  uint32_t carry = h.at_cigar;                                  // wave-uniform: bytes of the line in front of this block's ops
  for (uint64_t base = 0; base < r.n_ops; base += 64) {
    const uint64_t x = base + lane;
    const bool has = x < r.n_ops;
    const uint32_t op = has ? ops[r.op_off + x] : 0u, len = op >> 2;
    const uint32_t nb = has ? dec_digits(len) + 1u : 0u;
    uint32_t incl = nb;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t t = __shfl_up(incl, o, 64);
      if ((int)lane >= o) incl += t;
    }
    const uint32_t at = carry + incl - nb;
    if (has && (uint64_t)at + nb < line) {                      // (< : the newline is the line's last byte)
      put_dec(p + at, len, nb - 1);
      p[at + nb - 1] = (char)((0x3F44494Du >> ((op & 3u) * 8u)) & 0xffu);   // "MID?"
    }
    carry += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
  }
}

}  // namespace

void launch_paf_len(const PafRow* rows, const uint32_t* ops, const uint64_t* name_off, uint32_t n, uint32_t* line_bytes, PafSums* sums, hipStream_t st) {
  if (n) k_paf_len<<<(n + 3) / 4, 256, 0, st>>>(rows, ops, name_off, n, line_bytes, sums);
}

void launch_paf_write(const PafRow* rows, const uint32_t* ops, const char* names, const uint64_t* name_off, const uint32_t* line_off, const PafSums* sums,
                      uint32_t n, char* text, uint64_t cap, hipStream_t st) {
  if (n) k_paf_write<<<(n + 3) / 4, 256, 0, st>>>(rows, ops, names, name_off, line_off, sums, n, text, cap);
}

}  // namespace herro
