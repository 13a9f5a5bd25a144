"""The specification of the adapter step (include/herro_amd.h, "adapters") in plain numpy: the yardstick of
tests/test_adapters_host.py and tests/test_gpu_adapters.py.

* the scan: Sellers' dynamic programme for E(j) (row by row over the whole text), the runs of E <= k, `start` by an anchored programme over
  the reversed strings, and the order of the hits;
* the plan: the start / end / middle rule on a boolean mask of the read's bases;
* the cut.

No bit-vector code here: the kernels' recurrence and this file cannot share a mistake."""
import numpy as np

from align_ref import store_codes  # noqa: F401  (the store's codes, the non-ACGT quirk included)

HIT_DTYPE = np.dtype([("rid", "<u4"), ("start", "<u4"), ("end", "<u4"), ("adapter", "<u2"), ("strand", "u1"), ("errors", "u1")])
PIECE_DTYPE = np.dtype([("rid", "<u4"), ("start", "<u4"), ("end", "<u4")])
assert HIT_DTYPE.itemsize == 16 and PIECE_DTYPE.itemsize == 12
_CODE = {65: 0, 97: 0, 67: 1, 99: 1, 71: 2, 103: 2, 84: 3, 116: 3}


# ---- patterns -------------------------------------------------------------------------------------------------------------------------
def adapter_codes(seq: bytes) -> np.ndarray:
    if not 8 <= len(seq) <= 64:
        raise ValueError("8 <= length <= 64")
    if any(b not in _CODE for b in seq):
        raise ValueError("not A, C, G or T")
    return np.array([_CODE[b] for b in seq], np.int64)


def max_errors(m: int, max_err_pm: int = 0) -> int:
    pm = max_err_pm or 250
    if pm > 500:
        raise ValueError("max_err_pm <= 500")
    return m * pm // 1000


def patterns(adapters, forward_only=False):
    """[(adapter index, strand, codes)]: strand 1 is the reverse complement"""
    if not 1 <= len(adapters) <= 32:
        raise ValueError("1 <= n_adapters <= 32")
    out = []
    for a, seq in enumerate(adapters):
        c = adapter_codes(seq)
        out.append((a, 0, c))
        if not forward_only:
            out.append((a, 1, 3 - c[::-1]))
    return out


# ---- the scan -------------------------------------------------------------------------------------------------------------------------
def last_row(P: np.ndarray, T: np.ndarray, anchored: bool = False) -> np.ndarray:
    """D[m][0 .. n] of the edit-distance table of P (rows) against T (columns), unit costs.  Row 0 is all 0 (the alignment may begin at any
    text position: D[m][j] = E(j)) or, anchored, 0 .. n (it begins at T's first base: D[m][j] = distance of P and T[:j])."""
    n = len(T)
    idx = np.arange(n + 1, dtype=np.int64)
    row = idx.copy() if anchored else np.zeros(n + 1, np.int64)
    for i in range(1, len(P) + 1):
        c = np.empty(n + 1, np.int64)
        c[0] = i
        c[1:] = np.minimum(row[:-1] + (T != P[i - 1]), row[1:] + 1)        # diagonal, vertical
        row = np.minimum.accumulate(c - idx) + idx                          # horizontal: row[j] = min over j' <= j of c[j'] + (j - j')
    return row


def read_hits(T: np.ndarray, P: np.ndarray, k: int):
    """[(start, end, errors)] of one pattern in one read, ascending end"""
    m, n = len(P), len(T)
    if n == 0:
        return []
    E = last_row(P, np.asarray(T, np.int64))
    below = np.concatenate([[False], E[1:] <= k, [False]])                 # index = j; j = 0 is no end position
    edge = np.flatnonzero(below[1:] != below[:-1]) + 1
    out = []
    for a, b in zip(edge[0::2], edge[1::2]):                               # the run is j in [a, b)
        end = a + int(np.argmin(E[a:b]))                                    # the first of the least
        errors = int(E[end])
        width = min(end, 2 * m)                                             # a distance <= m / 2 needs a length <= 3 m / 2
        back = last_row(P[::-1], np.asarray(T[end - width:end], np.int64)[::-1], anchored=True)
        hit = np.flatnonzero(back == errors)
        assert len(hit), (end, errors)
        out.append((end - int(hit[0]), end, errors))                        # the shortest such substring: the largest start
    return out


def find_adapters(read_codes, adapters, max_err_pm: int = 0, forward_only: bool = False):
    """(hits HIT_DTYPE ascending (rid, end, start, adapter, strand), hits_off u64 [n_reads + 1])"""
    pats = patterns(adapters, forward_only)
    for _, _, c in pats:
        max_errors(len(c), max_err_pm)
    rows = []
    for rid, T in enumerate(read_codes):
        for a, s, P in pats:
            for start, end, errors in read_hits(np.asarray(T), P, max_errors(len(P), max_err_pm)):
                rows.append((rid, end, start, a, s, errors))
    rows.sort()
    hits = np.zeros(len(rows), HIT_DTYPE)
    for x, (rid, end, start, a, s, errors) in enumerate(rows):
        hits[x] = (rid, start, end, a, s, errors)
    off = np.zeros(len(read_codes) + 1, np.uint64)
    np.add.at(off, hits["rid"].astype(np.int64) + 1, 1)
    return hits, np.cumsum(off).astype(np.uint64)


# ---- the plan -------------------------------------------------------------------------------------------------------------------------
def trim_plan(read_len, adapter_len, hits, hits_off, end_window=0, end_max_err_pm=0, mid_max_err_pm=0, min_length=0, discard_chimeras=False):
    """(pieces PIECE_DTYPE, piece_off u64 [n_reads + 1], stats [trimmed, split, dropped, bases removed]); ValueError where the library
    answers HERRO_E_INVALID"""
    end_window, end_pm, mid_pm = end_window or 150, end_max_err_pm or 250, mid_max_err_pm or 100
    hits_off = [int(x) for x in hits_off]
    if len(hits_off) != len(read_len) + 1 or hits_off[0] != 0 or any(b < a for a, b in zip(hits_off, hits_off[1:])):
        raise ValueError("hits_off must ascend from 0")
    pieces, piece_off, stats = [], [0], [0, 0, 0, 0]
    for r, L in enumerate(int(x) for x in read_len):
        keep = np.zeros(L, bool)
        lo, hi, mids = 0, L, []
        for h in hits[hits_off[r]:hits_off[r + 1]]:
            rid, start, end, a, errors = int(h["rid"]), int(h["start"]), int(h["end"]), int(h["adapter"]), int(h["errors"])
            if rid != r or start > end or end > L or a >= len(adapter_len):
                raise ValueError("bad hit")
            m = int(adapter_len[a])
            if start < end_window and errors <= m * end_pm // 1000:
                lo = max(lo, end)
            elif end > L - end_window and errors <= m * end_pm // 1000:
                hi = min(hi, start)
            elif errors <= m * mid_pm // 1000:
                mids.append((start, end))
        keep[lo:hi] = lo < hi
        for s, e in mids:
            keep[s:e] = False
        if mids and discard_chimeras:
            keep[:] = False
        edge = np.flatnonzero(np.diff(np.concatenate([[0], keep.astype(np.int8), [0]])))
        mine = [(int(a), int(b)) for a, b in zip(edge[0::2], edge[1::2]) if b - a >= max(min_length, 1)]
        pieces += [(r, a, b) for a, b in mine]
        piece_off.append(len(pieces))
        stats[0] += lo > 0 or hi < L
        stats[1] += len(mine) > 1
        stats[2] += len(mine) == 0
        stats[3] += L - sum(b - a for a, b in mine)
    return np.array(pieces, PIECE_DTYPE) if pieces else np.zeros(0, PIECE_DTYPE), np.array(piece_off, np.uint64), stats


# ---- the cut --------------------------------------------------------------------------------------------------------------------------
def cut_reads(ids, descs, reads, quals, pieces):
    """ids / descs / reads / quals: one entry per read (bytes; descs entries may be None); -> the same four lists for the pieces, in their order"""
    per_read = {}
    for p in pieces:
        per_read[int(p["rid"])] = per_read.get(int(p["rid"]), 0) + 1
    seen, out = {}, ([], [], [], [])
    for p in pieces:
        r, a, b = int(p["rid"]), int(p["start"]), int(p["end"])
        if r >= len(reads) or a > b or b > len(reads[r]):
            raise ValueError("bad piece")
        seen[r] = seen.get(r, 0) + 1
        out[0].append(ids[r] + (b"_%d" % seen[r] if per_read[r] > 1 else b""))
        out[1].append(descs[r])
        out[2].append(reads[r][a:b])
        out[3].append(quals[r][a:b])
    return out
