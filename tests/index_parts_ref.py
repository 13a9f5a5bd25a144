"""numpy restatement of the overlap finder with its index built in parts (herro_set_index_params; csrc/overlap_dev.hip: k_sketch_part, k_occ16,
k_occ_pick, k_part_cls, k_part_runs, k_part_expand; DESIGN.md §10, "An index in parts"), on top of overlap_ref, occ_ref and rescue_ref.  All
integer.  What it must equal is the UNPARTITIONED specification — rescue_ref.find_overlaps_rescue, which is occ_ref's and overlap_ref's where the
options are off — for every part size and every number of hash ranges.

  blocks   nk[r] = len[r] - k + 1 if len[r] >= k + w - 1, else 0; cap = max(max_kmers // 2, 1); reads in ascending id, acc = 0: a new block opens
           in front of read r iff nk[r] > 0, acc > 0 and acc + nk[r] > cap (acc restarts at 0), then acc += nk[r].
  pass A   the 2k-bit hash space in R equal ranges; per range the store's minimizers whose hash lies in it, grouped by hash: occ of every member =
           the size of its group (a group lies in one range), and one entry of the census per group.  The cut is occ_ref.occ_cut of the census.
  pass B   per block pair (i, j), i <= j, ascending: the minimizers of the two blocks, each with its occ from pass A, grouped by hash.  A group
           is used iff 2 <= occ <= cut; with the rescue also iff cut < occ <= rescue_max_occ, and the rescued are chosen per read from occ
           (rescue_ref.streaks / streak_quota).  Two members x < y of a group in reads t != q give an anchor iff — i < j — t lies in block i and
           q in block j, or — i == j — always (t < q then); above the cut, iff one of the two is rescued.  The pair's anchors are chained and
           picked by overlap_ref.find_overlaps itself; the rows of all pairs, put in (tid, qid) order, are the result.

The underscored switches are not part of the specification: they make the mutants tests/test_index_parts_host.py holds it against."""
from __future__ import annotations

import numpy as np

import occ_ref as OR
import overlap_ref as R
import rescue_ref as RR


def read_kmers(lens, k: int, w: int) -> np.ndarray:
    lens = np.asarray(lens, np.int64)
    return np.where(lens >= k + w - 1, lens - k + 1, 0)


def block_cuts(lens, k: int, w: int, max_kmers: int) -> list:
    """the block rule: cuts [n_blocks + 1], ascending read ids; [0] for an empty store"""
    nk = read_kmers(lens, k, w)
    if not len(nk):
        return [0]
    cap = max(int(max_kmers) // 2, 1)
    cuts, acc = [0], 0
    for r, c in enumerate(nk):
        c = int(c)
        if c and acc and acc + c > cap:
            cuts.append(r)
            acc = 0
        acc += c
    return cuts + [len(nk)]


def occurrences_by_range(h, k: int, ranges: int):
    """pass A: (occ int64 [n] of every minimizer, counts int64 [D] of the distinct hashes in the order the ranges give them)"""
    h = np.asarray(h, np.uint64)
    occ = np.zeros(len(h), np.int64)
    counts = []
    space = 1 << (2 * k)
    step = -(-space // int(ranges))
    for lo in range(0, space, step):
        hi = min(lo + step, space) - 1
        m = np.flatnonzero((h >= np.uint64(lo)) & (h <= np.uint64(hi)))
        if not len(m):
            continue
        _, inv, cnt = np.unique(h[m], return_inverse=True, return_counts=True)
        occ[m] = cnt[inv]
        counts.append(cnt.astype(np.int64))
    return occ, (np.concatenate(counts) if counts else np.zeros(0, np.int64))


def rescue_from_occ(occ, rid, pos, lens, r0: int, r1: int, cut: int, occ_dist: int, rmax: int) -> np.ndarray:
    """the rescued flags (u8) of the minimizers of reads r0 .. r1 - 1, given in (rid, pos) order with their occ: rescue_ref's rule per read"""
    flag = np.zeros(len(occ), np.uint8)
    if not occ_dist:
        return flag
    bounds = np.searchsorted(rid, np.arange(r0, r1 + 1))
    for r in range(r0, r1):
        b, e = int(bounds[r - r0]), int(bounds[r - r0 + 1])
        for idx, ps, pe in RR.streaks(occ[b:e], pos[b:e], int(lens[r]), cut, rmax):
            m = RR.streak_quota(ps, pe, occ_dist)
            take = idx if m >= len(idx) else idx[np.lexsort((pos[b:e][idx], occ[b:e][idx]))[:m]]
            flag[b + take] = 1
    return flag


def pair_anchors(h, rid, pos, st, occ, flag, lens, k: int, cut: int, rmax: int, split: int, _local_length: bool = False, _same_block: bool = False):
    """the anchors of one block pair, (t, q, rel, tpos, qpos) int64 rows sorted by that tuple.  h .. flag: the pair's minimizers in (rid, pos)
    order; rmax 0: no rescue; split: the first read of block j for i < j, 0 for i == j."""
    o = np.lexsort((pos, rid, h))
    h, rid, pos, st, occ, flag = h[o], rid[o], pos[o], st[o].astype(np.int64), occ[o], flag[o].astype(bool)
    out = [np.zeros((0, 5), np.int64)]
    if len(h):
        b = np.flatnonzero(np.concatenate([[True], h[1:] != h[:-1], [True]]))
        for s0, s1 in zip(b[:-1], b[1:]):
            c = int(s1 - s0) if _local_length else int(occ[s0])      # (the mutant judges a run by its length inside the pair)
            used, high = 2 <= c <= cut, cut < c <= rmax
            if not (used or high) or s1 - s0 < 2:
                continue
            x, y = np.triu_indices(int(s1 - s0), 1)
            x, y = x + s0, y + s0
            keep = rid[x] != rid[y]
            if split and not _same_block:
                keep &= (rid[x] < split) & (rid[y] >= split)
            elif split:
                keep &= rid[y] >= split                               # (the mutant: block j's own pairs once more in (i, j))
            if high:
                keep &= flag[x] | flag[y]
            x, y = x[keep], y[keep]
            rel = st[x] ^ st[y]
            qpos = np.where(rel == 0, pos[y], lens[rid[y]] - pos[y] + k - 2)
            out.append(np.stack([rid[x], rid[y], rel, pos[x], qpos], axis=1).astype(np.int64).reshape(-1, 5))
    a = np.concatenate(out)
    return a[np.lexsort((a[:, 4], a[:, 3], a[:, 2], a[:, 1], a[:, 0]))]


def find_overlaps_parts(read_codes, max_kmers: int, ranges: int = 1, occ_dist: int = 0, rescue_max_occ: int | None = None, occ_frac_ppm: int = 0,
                        lookback: int | None = R.LOOKBACK, stats: dict | None = None, _local_length: bool = False, _local_classes: bool = False,
                        _same_block: bool = False, **kw):
    """The finder with its index in parts: (rids, rows, aln_off, scores) as overlap_ref.find_overlaps returns them.  stats gains cut, occ (clipped
    to 65535), rescued (flags in (rid, pos) order), blocks and pairs (the block pairs)."""
    P = R.params(**{n: v for n, v in kw.items() if not (occ_frac_ppm and n == "max_occ")})
    k, w = P["k"], P["w"]
    lens = np.array([len(c) for c in read_codes], np.int64)
    h, rid, pos, st = R.sketch_store(read_codes, k, w)
    occ, counts = occurrences_by_range(h, k, ranges)
    cut = P["max_occ"]
    if occ_frac_ppm:
        cut = OR.occ_cut(counts, occ_frac_ppm, int(kw.get("max_occ") or 0))
    d, rmax = RR.check(occ_dist, rescue_max_occ)
    if not d:
        rmax = 0
    cuts = block_cuts(lens, k, w, max_kmers)
    nb = len(cuts) - 1
    first = np.searchsorted(rid, cuts)               # a block's minimizers are a contiguous range of the (rid, pos) order
    all_flags = np.zeros(len(h), np.uint8)
    parts, n_pairs = [], 0
    for i in range(nb):
        for j in range(i, nb):
            sl = np.r_[first[i]:first[i + 1]] if i == j else np.r_[first[i]:first[i + 1], first[j]:first[j + 1]]
            if not len(sl):
                continue
            n_pairs += 1
            ph, prid, ppos, pst = h[sl], rid[sl], pos[sl], st[sl]
            pocc = RR.occurrences(ph) if _local_classes else occ[sl]        # (the mutant: U / H / transparent from the counts inside the pair)
            flag = np.zeros(len(sl), np.uint8)
            ni = int(first[i + 1] - first[i])
            if d:
                flag[:ni] = rescue_from_occ(pocc[:ni], prid[:ni], ppos[:ni], lens, cuts[i], cuts[i + 1], cut, d, rmax)
                if j > i:
                    flag[ni:] = rescue_from_occ(pocc[ni:], prid[ni:], ppos[ni:], lens, cuts[j], cuts[j + 1], cut, d, rmax)
                if i == j:
                    all_flags[sl] = flag
            a = pair_anchors(ph, prid, ppos, pst, occ[sl], flag, lens, k, cut, rmax, cuts[j] if j > i else 0, _local_length, _same_block)
            if not len(a):
                continue
            plain_sketch = R.sketch_store
            R.anchors = lambda *_args, _a=a: _a         # everything behind the anchors is overlap_ref.find_overlaps itself
            R.sketch_store = lambda *_args: (h, rid, pos, st)       # (it only hands the sketch on to anchors: not taken again per pair)
            try:
                parts.append(R.find_overlaps(read_codes, lookback=lookback, **dict(kw, max_occ=cut)))
            finally:
                R.anchors, R.sketch_store = RR._PLAIN_ANCHORS, plain_sketch
    if stats is not None:
        stats.update(cut=cut, occ=np.minimum(occ, RR.OCC_CAP), rescued=all_flags, blocks=nb, pairs=n_pairs)
    return merge_rows(parts)


def merge_rows(parts):
    """the (rids, rows, aln_off, scores) of several block pairs as one: rows by (tid, qid), grouped by target"""
    rows = np.concatenate([p[1] for p in parts]) if parts else np.zeros((0, 10), np.uint32)
    scores = np.concatenate([p[3] for p in parts]) if parts else np.zeros(0, np.int32)
    o = np.lexsort((rows[:, 0], rows[:, 5]))
    rows, scores = rows[o], scores[o]
    rids, counts = np.unique(rows[:, 5], return_counts=True)
    aln_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    return rids.astype(np.uint32), rows.astype(np.uint32).reshape(-1, 10), aln_off, scores.astype(np.int32)
