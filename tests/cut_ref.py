"""The specification of herro_store_cut (include/herro_amd.h; DESIGN.md §13, "The cut on the device") in numpy, with no shift arithmetic: a
store is unpacked to one code per base, sliced, and packed again.

A store is a dict of the six arrays as herro_debug_store_copy returns them (Context.store_arrays):
  words u64 [n_words + 1] (one zero pad word), word_off u64 [n + 1], qual u8 [qual_bytes], qual_off u64 [n + 1], p0 / p1 u32 [n_words + 2].

  store_of(reads, quals)   the store herro_set_reads builds: every read through herro_encode_2bit (api.encode_2bit), which is where a byte
                           that is not ACGT smears over its neighbours — and over the bits above the read's end.
  read_codes(store, r)     the codes of read r as the store holds them.
  cut(store, pieces)       the store herro_store_cut builds: code i of new read x = code start + i of old read rid; bits above a read's
                           end zero; planes = the even / odd bits of the new words; qualities the byte slice; offsets the running sums."""
import numpy as np

from herro_amd import api

NAMES = ("words", "word_off", "qual", "qual_off", "p0", "p1")


def _bits_of_words(words: np.ndarray) -> np.ndarray:
    """bit b of word w at [64 w + b]"""
    return np.unpackbits(np.ascontiguousarray(words, "<u8").view(np.uint8), bitorder="little")


def _pack(codes_per_read) -> dict:
    """words and word_off of reads given as code arrays: every read from a word boundary, zero above its end, the pad word behind"""
    n_words = sum((len(c) + 31) // 32 for c in codes_per_read)
    bits = np.zeros(64 * (n_words + 1), np.uint8)
    word_off = np.zeros(len(codes_per_read) + 1, np.uint64)
    w = 0
    for i, c in enumerate(codes_per_read):
        c = np.asarray(c, np.uint8)
        assert c.size == 0 or int(c.max()) <= 3
        bits[64 * w:64 * w + 2 * len(c):2] = c % 2
        bits[64 * w + 1:64 * w + 2 * len(c):2] = c // 2
        w += (len(c) + 31) // 32
        word_off[i + 1] = w
    return dict(words=np.packbits(bits, bitorder="little").view("<u8").astype(np.uint64), word_off=word_off)


def _planes_of(words: np.ndarray) -> tuple:
    """even / odd bits of every word but the pad, compacted, two zero entries behind"""
    n_words = len(words) - 1
    bits = _bits_of_words(words[:n_words])
    out = []
    for b in (bits[0::2], bits[1::2]):
        p = np.packbits(b, bitorder="little").view("<u4").astype(np.uint32) if n_words else np.zeros(0, np.uint32)
        out.append(np.concatenate([p, np.zeros(2, np.uint32)]))
    return out[0], out[1]


def store_of(reads, quals=None) -> dict:
    """herro_set_reads of ASCII reads (quals: one u8 array per read; None: 73 everywhere, as pair_cases.Reads)"""
    enc = [api.encode_2bit(bytes(r)) if len(r) else np.zeros(0, np.uint64) for r in reads]
    words = np.concatenate(enc + [np.zeros(1, np.uint64)]).astype(np.uint64)
    word_off = np.concatenate([[0], np.cumsum([len(e) for e in enc])]).astype(np.uint64)
    qual_off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    qual = np.full(int(qual_off[-1]), 73, np.uint8) if quals is None else np.concatenate([np.asarray(q, np.uint8) for q in quals] + [np.zeros(0, np.uint8)])
    assert len(qual) == int(qual_off[-1])
    p0, p1 = _planes_of(words)
    return dict(words=words, word_off=word_off, qual=qual, qual_off=qual_off, p0=p0, p1=p1)


def read_codes(store: dict, r: int) -> np.ndarray:
    """codes 0 .. 3 of read r as the store holds them"""
    w0, w1 = int(store["word_off"][r]), int(store["word_off"][r + 1])
    n = int(store["qual_off"][r + 1] - store["qual_off"][r])
    bits = _bits_of_words(store["words"][w0:w1])
    return (bits[0::2] + 2 * bits[1::2])[:n].astype(np.uint8)


def cut(store: dict, pieces) -> dict:
    n = len(store["word_off"]) - 1
    codes, quals = [], []
    cache = {}
    for p in pieces:
        rid, start, end = int(p["rid"]), int(p["start"]), int(p["end"])
        length = int(store["qual_off"][rid + 1] - store["qual_off"][rid])
        assert rid < n and start <= end <= length
        if rid not in cache:
            cache[rid] = read_codes(store, rid)
        codes.append(cache[rid][start:end])
        q0 = int(store["qual_off"][rid])
        quals.append(store["qual"][q0 + start:q0 + end])
    out = _pack(codes)
    out["p0"], out["p1"] = _planes_of(out["words"])
    out["qual"] = np.concatenate(quals + [np.zeros(0, np.uint8)]).astype(np.uint8)
    out["qual_off"] = np.concatenate([[0], np.cumsum([len(q) for q in quals])]).astype(np.uint64)
    return out


def assert_same(got: dict, want: dict, tag):
    for name in NAMES:
        g, w = np.asarray(got[name]), np.asarray(want[name])
        if g.dtype != w.dtype or g.shape != w.shape or not np.array_equal(g, w):
            bad = int(np.flatnonzero(g[:min(len(g), len(w))] != w[:min(len(g), len(w))])[0]) if g.dtype == w.dtype and (g[:min(len(g), len(w))] != w[:min(len(g), len(w))]).any() else -1
            raise AssertionError((tag, name, g.dtype, g.shape, w.shape, "first difference at", bad, g[max(bad, 0):bad + 3], w[max(bad, 0):bad + 3]))
