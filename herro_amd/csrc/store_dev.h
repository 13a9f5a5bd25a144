// store_dev.h — the read store cut to a piece table on the device (store_dev.hip): what herro_reads_cut + herro_set_reads build through the
// host, without a base or a quality byte leaving HBM.  The specification is include/herro_amd.h's, "herro_store_cut" (DESIGN.md §13,
// tests/cut_ref.py).  The host's share (store_cut_plan: validation and the new offset tables) knows no device and the per-element functions
// are __host__ __device__, so tools/store_cut_check.cpp runs all of it on the CPU against a base-by-base answer.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/herro_amd.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define STORE_HD __host__ __device__
#else
#define STORE_HD
#endif

namespace herro {

constexpr uint64_t STORE_CUT_MAX_PIECES = 0x7fffffffull;

// ---- the host's share ------------------------------------------------------------------------------------------------------------------------
// Checks the table against the read lengths and fills the offsets of the new store: word_off / qual_off [n_pieces + 1], the running sums of
// ceil(len / 32) and len.  HERRO_OK, or HERRO_E_INVALID / HERRO_E_UNSUPPORTED and a message that names the first offending piece; nothing
// else is looked at, so a refused table leaves the caller's store as it was.
inline int store_cut_plan(uint32_t n_reads, const uint32_t* read_len, uint64_t n_pieces, const herro_piece* pieces, std::vector<uint64_t>& word_off,
                          std::vector<uint64_t>& qual_off, std::string& err) {
  const char* const who = "herro_store_cut: ";
  if (n_pieces && !pieces) { err = std::string(who) + "null piece table"; return HERRO_E_INVALID; }
  if (n_pieces > STORE_CUT_MAX_PIECES) { err = std::string(who) + "more than 2^31 - 1 pieces"; return HERRO_E_UNSUPPORTED; }
  for (uint64_t x = 0; x < n_pieces; x++) {
    const herro_piece& p = pieces[x];
    const char* bad = p.rid >= n_reads ? "rid outside the reads" : p.start > p.end ? "start > end" : p.end > read_len[p.rid] ? "end beyond the read" : nullptr;
    if (bad) { err = std::string(who) + "piece " + std::to_string(x) + ": " + bad; return HERRO_E_INVALID; }
  }
  word_off.assign(n_pieces + 1, 0);
  qual_off.assign(n_pieces + 1, 0);
  for (uint64_t x = 0; x < n_pieces; x++) {
    const uint64_t len = pieces[x].end - pieces[x].start;
    word_off[x + 1] = word_off[x] + (len + 31) / 32;
    qual_off[x + 1] = qual_off[x] + len;
  }
  return HERRO_OK;
}

// ---- the per-element functions (host and device: the kernels are these behind an index computation) -------------------------------------------
// The piece that owns element e (a word, a quality byte) of the new store: the last x in [lo, hi] with off[x] <= e.  off[lo] <= e is the
// caller's; an empty piece shares its offset with its successor, which is the one found.
STORE_HD inline uint32_t store_piece_of(const uint64_t* __restrict__ off, uint32_t lo, uint32_t hi, uint64_t e) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo + 1) >> 1);
    if (off[mid] <= e) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// bits 0, 2, 4, ... of t -> bits 0, 1, 2, ... (the planes of upload_reads: p0 = store_compact(word), p1 = store_compact(word >> 1))
STORE_HD inline uint32_t store_compact(uint64_t t) {
  t &= 0x5555555555555555ull;
  t = (t | (t >> 1)) & 0x3333333333333333ull;
  t = (t | (t >> 2)) & 0x0f0f0f0f0f0f0f0full;
  t = (t | (t >> 4)) & 0x00ff00ff00ff00ffull;
  t = (t | (t >> 8)) & 0x0000ffff0000ffffull;
  t = (t | (t >> 16)) & 0x00000000ffffffffull;
  return (uint32_t)t;
}

// Word j of the piece [start, start + len) of a read (src: the read's first word, 32 codes per word, LSB first): a funnel shift of two
// neighbouring source words by 2 (start & 31) bits, masked to the codes the piece still has.  j < ceil(len / 32).  The second word is read
// only where the output word takes codes from it — never for a shift of 0 (which must not turn into a shift by 64), and never behind the
// read's last word, whose successor is the next read's.
STORE_HD inline uint64_t store_cut_word(const uint64_t* __restrict__ src, uint32_t start, uint32_t len, uint32_t j) {
  const uint64_t s = (uint64_t)start + 32ull * j;        // first code of the output word, in the read
  const uint32_t in = (uint32_t)(s & 31u);               // its place in its source word
  const uint32_t n = len - 32u * j < 32u ? len - 32u * j : 32u;
  const uint64_t* const w = src + (s >> 5);
  uint64_t out = w[0] >> (2u * in);
  if (in + n > 32u) out |= w[1] << (64u - 2u * in);      // (in > 0 here)
  if (n < 32u) out &= (1ull << (2u * n)) - 1ull;
  return out;
}

// 16 bytes of the new quality array, from byte d (a multiple of 16) on; x: the piece of byte d (store_piece_of over qual_off).  A chunk that
// lies in one piece is the source realigned in registers: aligned 8-byte loads, two where source and destination agree modulo 8 and three
// otherwise, funnel-shifted by the residue.  Every load holds a byte of the piece, so none reaches beyond the source array's 8 pad bytes.
// A chunk with a piece boundary in it (or the array's end: bytes from `total` on are 0) is put together byte by byte.
// src_qual must be 8-byte aligned.
struct StoreQ16 { uint64_t lo, hi; };
STORE_HD inline StoreQ16 store_cut_qual16(const uint8_t* __restrict__ src_qual, const uint64_t* __restrict__ src_qual_off, const herro_piece* __restrict__ pieces,
                                          const uint64_t* __restrict__ qual_off, uint32_t x, uint64_t d, uint64_t total) {
  if (d + 16 <= qual_off[x + 1]) {
    const uint64_t s = src_qual_off[pieces[x].rid] + pieces[x].start + (d - qual_off[x]);
    const uint32_t m = (uint32_t)(s & 7u);
    const uint64_t* const a = (const uint64_t*)(src_qual + (s - m));
    const uint64_t w0 = a[0], w1 = a[1];
    if (!m) return StoreQ16{w0, w1};
    const uint64_t w2 = a[2];
    return StoreQ16{(w0 >> (8u * m)) | (w1 << (64u - 8u * m)), (w1 >> (8u * m)) | (w2 << (64u - 8u * m))};
  }
  StoreQ16 out{0, 0};
  for (uint32_t i = 0; i < 16; i++) {
    const uint64_t b = d + i;
    if (b >= total) break;
    while (qual_off[x + 1] <= b) x++;                    // (b < total = qual_off[n_pieces]: ends)
    const uint64_t q = src_qual[src_qual_off[pieces[x].rid] + pieces[x].start + (b - qual_off[x])];
    if (i < 8) out.lo |= q << (8u * i); else out.hi |= q << (8u * (i - 8u));
  }
  return out;
}

// ---- the device's share (store_dev.hip) -------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
constexpr uint32_t STORE_CUT_TILE = 1024;   // elements (words; 16-byte quality chunks) of one workgroup: 256 lanes, four strides

struct StoreArrays {        // the six device arrays of a read store
  uint64_t* words = nullptr;      // [n_words + 1], the last one the zero pad
  uint64_t* word_off = nullptr;   // [n_reads + 1]
  uint8_t* qual = nullptr;        // [qual_bytes] and at least 8 pad bytes
  uint64_t* qual_off = nullptr;   // [n_reads + 1]
  uint32_t* p0 = nullptr;         // [n_words + 2], the last two the zero pad
  uint32_t* p1 = nullptr;
};

struct StoreCutStats { double words_ms = 0, qual_ms = 0, copy_words_ms = 0, copy_qual_ms = 0; };

// A new store beside `old`: read x = piece x of the old one, n pieces.  word_off / qual_off: store_cut_plan's.  Allocates the six arrays of `out` (the
// caller owns them on success; on an error they are freed and out is empty), uploads the piece table and the offsets, runs k_store_cut_words
// and k_store_cut_qual on st and returns when they are done.  stats (may be NULL): the kernels between events; level 2 also times a
// device-to-device hipMemcpyAsync of each kernel's output bytes, the yardstick of tools/adapterrate.py --cut.  hipSuccess or the failing call's
// error with its name in err.
hipError_t store_cut(const StoreArrays& old, const herro_piece* pieces, uint32_t n, const std::vector<uint64_t>& word_off,
                     const std::vector<uint64_t>& qual_off, hipStream_t st, StoreArrays& out, StoreCutStats* stats, int stats_level, std::string& err);
#endif

}  // namespace herro
