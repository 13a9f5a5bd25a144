// store_cut_check — seeded random read stores and piece tables through the host share of herro_store_cut (herro::store_cut_plan: the checks and
// the new offsets) and through the __host__ __device__ functions its kernels are made of (store_piece_of, store_cut_word, store_compact,
// store_cut_qual16; herro_amd/csrc/store_dev.h), on the CPU, meant for a sanitizer build.  Every word, plane entry and quality chunk is
// compared with a base-by-base answer; the arrays are allocated at exactly the sizes the device arrays have (the word array with its one pad
// word, the quality array with its 8 pad bytes), so a source load beyond them is the sanitizer's to report.  A damaged copy of every table
// is refused with a message that names the piece.  No HIP call.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o /tmp/store_cut_check tools/store_cut_check.cpp && /tmp/store_cut_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>

#include "../herro_amd/csrc/store_dev.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "table %d: %s (line %d)\n", table, #c, __LINE__); return 1; } } while (0)

int main(int argc, char** argv) {
  const int n_tables = argc > 1 ? std::atoi(argv[1]) : 4000;
  std::mt19937 rng(9876);
  auto pick = [&](uint32_t lo, uint32_t hi) { return lo + (uint32_t)(rng() % (hi - lo + 1)); };
  const uint32_t len_pool[] = {0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 200, 600};
  size_t n_pieces_all = 0, n_words_all = 0, n_chunks_all = 0, n_refused = 0;
  for (int table = 0; table < n_tables; table++) {
    // ---- a store: codes (with arbitrary bits above a read's end in its last word, as a smear leaves them) and qualities
    const uint32_t n_reads = pick(1, 6);
    std::vector<uint32_t> read_len(n_reads);
    std::vector<uint64_t> s_word_off(n_reads + 1, 0), s_qual_off(n_reads + 1, 0);
    for (uint32_t r = 0; r < n_reads; r++) {
      read_len[r] = len_pool[pick(0, 16)];
      s_word_off[r + 1] = s_word_off[r] + (read_len[r] + 31) / 32;
      s_qual_off[r + 1] = s_qual_off[r] + read_len[r];
    }
    const uint64_t sw = s_word_off[n_reads], sq = s_qual_off[n_reads];
    std::unique_ptr<uint64_t[]> words(new uint64_t[sw + 1]);              // exactly n_words + 1
    for (uint64_t i = 0; i < sw; i++) words[i] = (uint64_t)rng() << 32 | rng();
    words[sw] = 0;
    std::unique_ptr<uint64_t[]> qual_mem(new uint64_t[(sq + 8) / 8]);     // 8-byte aligned; the whole 8-byte words within qual_bytes + 8
    uint8_t* const qual = (uint8_t*)qual_mem.get();
    std::memset(qual, 0, (sq + 8) / 8 * 8);
    for (uint64_t i = 0; i < sq; i++) qual[i] = (uint8_t)pick(33, 126);
    auto code = [&](uint32_t r, uint32_t i) { return (uint32_t)(words[s_word_off[r] + i / 32] >> (2 * (i % 32))) & 3u; };
    // ---- a table
    const uint32_t n_pieces = pick(0, 12);
    std::vector<herro_piece> pieces(n_pieces);
    for (auto& p : pieces) {
      p.rid = pick(0, n_reads - 1);
      const uint32_t L = read_len[p.rid];
      p.start = pick(0, L);
      p.end = pick(0, 3) == 0 ? L : std::min(L, p.start + len_pool[pick(0, 14)]);
    }
    std::vector<uint64_t> word_off, qual_off;
    std::string why;
    CHECK(herro::store_cut_plan(n_reads, read_len.data(), n_pieces, n_pieces ? pieces.data() : nullptr, word_off, qual_off, why) == HERRO_OK);
    CHECK(word_off.size() == (size_t)n_pieces + 1 && qual_off.size() == (size_t)n_pieces + 1 && word_off[0] == 0 && qual_off[0] == 0);
    // ---- the answer base by base
    std::vector<uint8_t> want_qual;
    std::vector<uint64_t> want_words;
    for (uint32_t x = 0; x < n_pieces; x++) {
      const herro_piece& p = pieces[x];
      const uint32_t len = p.end - p.start;
      CHECK(word_off[x] == want_words.size() && qual_off[x] == want_qual.size());
      std::vector<uint64_t> w((len + 31) / 32, 0);
      for (uint32_t i = 0; i < len; i++) {
        w[i / 32] |= (uint64_t)code(p.rid, p.start + i) << (2 * (i % 32));
        want_qual.push_back(qual[s_qual_off[p.rid] + p.start + i]);
      }
      want_words.insert(want_words.end(), w.begin(), w.end());
    }
    CHECK(word_off[n_pieces] == want_words.size() && qual_off[n_pieces] == want_qual.size());
    // ---- every word and its planes, as k_store_cut_words maps them (the whole table searched, and a window as narrow as a tile's)
    const uint64_t nw = want_words.size();
    for (uint64_t g = 0; g < nw; g++) {
      const uint32_t x = herro::store_piece_of(word_off.data(), 0, n_pieces - 1, g);
      CHECK(word_off[x] <= g && g < word_off[x + 1]);
      const uint32_t lo = herro::store_piece_of(word_off.data(), 0, n_pieces - 1, g > 3 ? g - 3 : 0), hi = herro::store_piece_of(word_off.data(), lo, n_pieces - 1, std::min(nw - 1, g + 3));
      CHECK(herro::store_piece_of(word_off.data(), lo, hi, g) == x);
      const herro_piece& p = pieces[x];
      const uint64_t w = herro::store_cut_word(words.get() + s_word_off[p.rid], p.start, p.end - p.start, (uint32_t)(g - word_off[x]));
      CHECK(w == want_words[g]);
      uint32_t p0 = 0, p1 = 0;
      for (int i = 0; i < 32; i++) { p0 |= (uint32_t)((w >> (2 * i)) & 1u) << i; p1 |= (uint32_t)((w >> (2 * i + 1)) & 1u) << i; }
      CHECK(herro::store_compact(w) == p0 && herro::store_compact(w >> 1) == p1);
    }
    // ---- every 16-byte chunk of the qualities, as k_store_cut_qual maps them
    const uint64_t total = want_qual.size();
    for (uint64_t c = 0; 16 * c < total; c++) {
      const uint32_t x = herro::store_piece_of(qual_off.data(), 0, n_pieces - 1, 16 * c);
      CHECK(qual_off[x] <= 16 * c && 16 * c < qual_off[x + 1]);
      const herro::StoreQ16 q = herro::store_cut_qual16(qual, s_qual_off.data(), pieces.data(), qual_off.data(), x, 16 * c, total);
      uint8_t got[16];
      std::memcpy(got, &q.lo, 8);
      std::memcpy(got + 8, &q.hi, 8);
      for (uint32_t i = 0; i < 16; i++) CHECK(got[i] == (16 * c + i < total ? want_qual[16 * c + i] : 0));
      n_chunks_all++;
    }
    n_pieces_all += n_pieces;
    n_words_all += nw;
    // ---- one damaged copy of the table: refused, the message names the piece, nothing is filled in
    if (n_pieces) {
      std::vector<herro_piece> bad = pieces;
      const uint32_t x = pick(0, n_pieces - 1);
      switch (table % 3) {
        case 0: bad[x].rid = n_reads + pick(0, 3); break;
        case 1: bad[x].start = bad[x].end + 1; break;
        default: bad[x].end = read_len[bad[x].rid] + 1 + pick(0, 5); break;
      }
      for (uint32_t y = x + 1; y < n_pieces; y++) if (pick(0, 1)) bad[y].rid = n_reads;     // later ones too: the FIRST is named
      std::vector<uint64_t> wo{7}, qo{7};
      why.clear();
      CHECK(herro::store_cut_plan(n_reads, read_len.data(), n_pieces, bad.data(), wo, qo, why) == HERRO_E_INVALID);
      CHECK(why.rfind("herro_store_cut: piece " + std::to_string(x) + ": ", 0) == 0);
      CHECK(wo.size() == 1 && wo[0] == 7 && qo.size() == 1 && qo[0] == 7);
      CHECK(herro::store_cut_plan(n_reads, read_len.data(), n_pieces, nullptr, wo, qo, why) == HERRO_E_INVALID);
      n_refused += 2;
    }
    std::vector<uint64_t> wo, qo;
    const herro_piece one{0, 0, 0};
    CHECK(herro::store_cut_plan(n_reads, read_len.data(), herro::STORE_CUT_MAX_PIECES + 1, &one, wo, qo, why) == HERRO_E_UNSUPPORTED);
  }
  std::printf("store_cut_check: %d tables, %zu pieces, %zu words, %zu quality chunks, %zu damaged tables refused: ok\n", n_tables, n_pieces_all, n_words_all,
              n_chunks_all, n_refused);
  return 0;
}
