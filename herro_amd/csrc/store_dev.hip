// store_dev.hip — the cut of the read store on the device (store_dev.h; specification: include/herro_amd.h "herro_store_cut", DESIGN.md §13,
// tests/cut_ref.py).  Kernels:
//   k_store_cut_words  one lane per word of the new store, four strides per workgroup: store_cut_word, then the word and its two plane
//                      words (store_compact) in the one launch.
//   k_store_cut_qual   one lane per 16 bytes of the new quality array, aligned on the destination: store_cut_qual16, one 16-byte store.
// Lane -> piece: a search in the new offset table.  A workgroup owns STORE_CUT_TILE consecutive elements (four strides of its 256 lanes); the
// pieces of its first and last element are searched over the whole table once (the same for every lane: scalar loads), and a lane searches
// only between those two: no step where the tile lies in one piece, log2 of the tile's pieces otherwise.  A per-workgroup chunk table would
// be a second table to build and upload for what the offsets already say.  No LDS, no scratch.
#include "store_dev.h"

#include <algorithm>

namespace herro {
namespace {

__global__ __launch_bounds__(256) void k_store_cut_words(const uint64_t* __restrict__ src_words, const uint64_t* __restrict__ src_word_off,
                                                         const herro_piece* __restrict__ pieces, const uint64_t* __restrict__ word_off,
                                                         uint32_t n_pieces, uint64_t n_words, uint64_t* __restrict__ words,
                                                         uint32_t* __restrict__ p0, uint32_t* __restrict__ p1) {
  const uint64_t g0 = (uint64_t)blockIdx.x * STORE_CUT_TILE;
  if (g0 >= n_words) return;
  const uint64_t g1 = g0 + STORE_CUT_TILE < n_words ? g0 + STORE_CUT_TILE : n_words;
  const uint32_t x_lo = store_piece_of(word_off, 0, n_pieces - 1, g0), x_hi = store_piece_of(word_off, x_lo, n_pieces - 1, g1 - 1);
  for (uint64_t g = g0 + threadIdx.x; g < g1; g += 256) {
    const uint32_t x = store_piece_of(word_off, x_lo, x_hi, g);
    const herro_piece p = pieces[x];
    const uint64_t w = store_cut_word(src_words + src_word_off[p.rid], p.start, p.end - p.start, (uint32_t)(g - word_off[x]));
    words[g] = w;
    p0[g] = store_compact(w);
    p1[g] = store_compact(w >> 1);
  }
}

__global__ __launch_bounds__(256) void k_store_cut_qual(const uint8_t* __restrict__ src_qual, const uint64_t* __restrict__ src_qual_off,
                                                        const herro_piece* __restrict__ pieces, const uint64_t* __restrict__ qual_off,
                                                        uint32_t n_pieces, uint64_t total, uint8_t* __restrict__ qual) {
  const uint64_t n_chunks = (total + 15) / 16;
  const uint64_t c0 = (uint64_t)blockIdx.x * STORE_CUT_TILE;
  if (c0 >= n_chunks) return;
  const uint64_t c1 = c0 + STORE_CUT_TILE < n_chunks ? c0 + STORE_CUT_TILE : n_chunks;
  const uint32_t x_lo = store_piece_of(qual_off, 0, n_pieces - 1, 16 * c0), x_hi = store_piece_of(qual_off, x_lo, n_pieces - 1, 16 * (c1 - 1));
  for (uint64_t c = c0 + threadIdx.x; c < c1; c += 256) {
    const StoreQ16 q = store_cut_qual16(src_qual, src_qual_off, pieces, qual_off, store_piece_of(qual_off, x_lo, x_hi, 16 * c), 16 * c, total);
    *(ulonglong2*)(qual + 16 * c) = make_ulonglong2(q.lo, q.hi);
  }
}

void free_arrays(StoreArrays& a) {
  void* p[6] = {a.words, a.word_off, a.qual, a.qual_off, a.p0, a.p1};
  for (void* q : p) if (q) (void)hipFree(q);
  a = StoreArrays{};
}

}  // namespace

#define CUT_TRY(what, expr) do { const hipError_t _e = (expr); if (_e != hipSuccess) { err = std::string("herro_store_cut: ") + what + ": " + hipGetErrorString(_e); free_arrays(out); return _e; } } while (0)

hipError_t store_cut(const StoreArrays& old, const herro_piece* pieces, uint32_t n, const std::vector<uint64_t>& word_off,
                     const std::vector<uint64_t>& qual_off, hipStream_t st, StoreArrays& out, StoreCutStats* stats, int stats_level, std::string& err) {
  out = StoreArrays{};
  const uint64_t n_words = word_off[n], total = qual_off[n];
  const uint64_t qual_alloc = (total + 15) / 16 * 16 + 16;   // whole 16-byte stores, and the pad behind the last byte that herro_set_reads leaves
  struct Scratch { herro_piece* pieces = nullptr; hipEvent_t ev[3] = {nullptr, nullptr, nullptr}; void* copy = nullptr;
                   ~Scratch() { if (pieces) (void)hipFree(pieces); if (copy) (void)hipFree(copy); for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); } } S;
  CUT_TRY("words", hipMalloc((void**)&out.words, 8 * (n_words + 1)));
  CUT_TRY("p0", hipMalloc((void**)&out.p0, 4 * (n_words + 2)));
  CUT_TRY("p1", hipMalloc((void**)&out.p1, 4 * (n_words + 2)));
  CUT_TRY("word_off", hipMalloc((void**)&out.word_off, 8 * ((uint64_t)n + 1)));
  CUT_TRY("qual_off", hipMalloc((void**)&out.qual_off, 8 * ((uint64_t)n + 1)));
  CUT_TRY("qual", hipMalloc((void**)&out.qual, qual_alloc));
  CUT_TRY("piece table", hipMalloc((void**)&S.pieces, sizeof(herro_piece) * std::max<uint64_t>(n, 1)));
  CUT_TRY("word_off upload", hipMemcpyAsync(out.word_off, word_off.data(), 8 * ((uint64_t)n + 1), hipMemcpyHostToDevice, st));
  CUT_TRY("qual_off upload", hipMemcpyAsync(out.qual_off, qual_off.data(), 8 * ((uint64_t)n + 1), hipMemcpyHostToDevice, st));
  if (n) CUT_TRY("piece table upload", hipMemcpyAsync(S.pieces, pieces, sizeof(herro_piece) * n, hipMemcpyHostToDevice, st));
  // the pads: one zero word, two zero plane entries, the bytes behind the last whole 16-byte chunk
  CUT_TRY("pad", hipMemsetAsync(out.words + n_words, 0, 8, st));
  CUT_TRY("pad", hipMemsetAsync(out.p0 + n_words, 0, 8, st));
  CUT_TRY("pad", hipMemsetAsync(out.p1 + n_words, 0, 8, st));
  CUT_TRY("pad", hipMemsetAsync(out.qual + (qual_alloc - 16), 0, 16, st));
  if (stats) for (hipEvent_t& e : S.ev) CUT_TRY("event", hipEventCreate(&e));
  if (stats) CUT_TRY("event", hipEventRecord(S.ev[0], st));
  if (n_words) {
    k_store_cut_words<<<(uint32_t)((n_words + STORE_CUT_TILE - 1) / STORE_CUT_TILE), 256, 0, st>>>(old.words, old.word_off, S.pieces, out.word_off, n, n_words,
                                                                                                   out.words, out.p0, out.p1);
    CUT_TRY("k_store_cut_words launch", hipGetLastError());
  }
  if (stats) CUT_TRY("event", hipEventRecord(S.ev[1], st));
  if (total) {
    const uint64_t n_chunks = (total + 15) / 16;
    k_store_cut_qual<<<(uint32_t)((n_chunks + STORE_CUT_TILE - 1) / STORE_CUT_TILE), 256, 0, st>>>(old.qual, old.qual_off, S.pieces, out.qual_off, n, total, out.qual);
    CUT_TRY("k_store_cut_qual launch", hipGetLastError());
  }
  if (stats) CUT_TRY("event", hipEventRecord(S.ev[2], st));
  CUT_TRY("kernels", hipStreamSynchronize(st));
  if (stats) {
    float ms = 0;
    CUT_TRY("event", hipEventElapsedTime(&ms, S.ev[0], S.ev[1])); stats->words_ms = ms;
    CUT_TRY("event", hipEventElapsedTime(&ms, S.ev[1], S.ev[2])); stats->qual_ms = ms;
    if (stats_level >= 2 && n_words && total) {   // the yardstick: the new word array and the new quality array copied device to device (the second of two copies: the first warms up)
      CUT_TRY("yardstick buffer", hipMalloc(&S.copy, std::max(8 * n_words, total)));
      for (int which = 0; which < 2; which++) {
        const uint64_t nb = which ? total : 8 * n_words;
        const void* from = which ? (const void*)out.qual : (const void*)out.words;
        for (int pass = 0; pass < 2; pass++) {
          CUT_TRY("event", hipEventRecord(S.ev[0], st));
          CUT_TRY("yardstick copy", hipMemcpyAsync(S.copy, from, nb, hipMemcpyDeviceToDevice, st));
          CUT_TRY("event", hipEventRecord(S.ev[1], st));
          CUT_TRY("yardstick copy", hipStreamSynchronize(st));
        }
        CUT_TRY("event", hipEventElapsedTime(&ms, S.ev[0], S.ev[1]));
        (which ? stats->copy_qual_ms : stats->copy_words_ms) = ms;
      }
    }
  }
  return hipSuccess;
}

}  // namespace herro
