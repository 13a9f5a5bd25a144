"""Cases of the longer chain look-back (herro_set_chain_params, k_chain_far; DESIGN.md §10, "A longer look-back"), shared by
tests/test_lookback_host.py and tests/test_gpu_lookback.py: read pairs around tandem arrays, the rel-0 anchor group of each, its scores at
every look-back as tests/overlap_ref.py::chain gives them, slices of one group around every block and round boundary, and the mutant of the
reference that lets a farther round of 64 win a tie."""
from __future__ import annotations

import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overlap_ref as R  # noqa: E402

KW = dict(k=15, w=5, max_occ=4096, bandwidth=150, max_gap=5000)
LOOKBACKS = (64, 128, 192, 256, 512, 768, 1024)

# set -> (unit, copies, flank, seed), anchors of the rel-0 group of reads (0, 1), {look-back: score of tests/overlap_ref.py::chain}
SETS = {
    "T0": ((40, 12, 600, 7), 1527, {64: 903, 128: 1478, 192: 1478, 256: 1478, 512: 1478}),
    "T1": ((40, 30, 2400, 5), 10608, {64: 3084, 128: 3084, 192: 5346, 256: 5363, 512: 5399, 1024: 5399}),
    "T2": ((25, 60, 800, 9), 24958, {64: 2051, 128: 2063, 192: 2063, 256: 2801, 512: 2899, 1024: 2899}),
    "T3": ((60, 50, 300, 3), 33949, {64: 1513, 256: 2395, 512: 3095, 768: 3148, 1024: 3148, 2048: 3148}),
    "T4": ((60, 70, 400, 6), 77075, {64: 758, 256: 2758, 512: 4061, 768: 4508, 1024: 4548, 2048: 4548}),
}
T4_USED = (768, 1024)          # the look-backs the tests compute on T4 (about 3 s of reference each)
SLICE_FROM_TPOS = 2300         # T1's group from its first anchor at or behind this target position ...
SLICE_LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1089, 3000)   # ... in these lengths
EARLY_STOP_GAP = 120           # max_gap of the early-stop set: whole rounds of 64 lie beyond it (the farthest of a look-back of 1024, for a third of the anchors)
NEAR_STOP_GAP = 30             # ... and one where the stop falls behind each of the rounds 0 .. 5 for a share of the anchors, and never later
GAPS = (KW["max_gap"], EARLY_STOP_GAP, NEAR_STOP_GAP)


def tandem(unit: int, copies: int, flank: int, seed: int) -> list[bytes]:
    """flank random bp + a unit-bp unit x copies + flank random bp, two copies with 1 % substitutions each"""
    rng = np.random.default_rng(seed)
    u = rng.integers(0, 4, unit)
    g = np.concatenate([rng.integers(0, 4, flank), np.tile(u, copies), rng.integers(0, 4, flank)])
    reads = []
    for _ in range(2):
        r = g.copy()
        m = rng.random(len(r)) < 0.01
        r[m] = (r[m] + rng.integers(1, 4, m.sum())) & 3
        reads.append(bytes(b"ACGT"[x] for x in r))
    return reads


@functools.lru_cache(maxsize=None)
def reads(name: str) -> tuple:
    return tuple(tandem(*SETS[name][0]))


def store(names) -> tuple:
    """(seq u8, qual u8, off u64, codes) of the reads of the named sets, one after the other: Context.set_reads' arguments and the reference's"""
    rs = [r for n in names for r in reads(n)]
    seq = np.frombuffer(b"".join(rs), np.uint8)
    off = np.concatenate([[0], np.cumsum([len(r) for r in rs])]).astype(np.uint64)
    return seq, np.full(len(seq), 40 + 33, np.uint8), off, [R.store_codes(r) for r in rs]


@functools.lru_cache(maxsize=None)
def group(name: str) -> tuple:
    """(tpos, qpos) int64 of the rel-0 group of reads (0, 1) of a set, ascending (tpos, qpos)"""
    codes = [R.store_codes(r) for r in reads(name)]
    lens = np.array([len(c) for c in codes], np.int64)
    a = R.anchors(*R.sketch_store(codes, KW["k"], KW["w"]), lens, KW["k"], KW["max_occ"])
    a = a[(a[:, 0] == 0) & (a[:, 1] == 1) & (a[:, 2] == 0)]
    return a[:, 3].copy(), a[:, 4].copy()


@functools.lru_cache(maxsize=None)
def slices() -> tuple:
    tp, qp = group("T1")
    s = int(np.searchsorted(tp, SLICE_FROM_TPOS, side="left"))
    assert s + max(SLICE_LENGTHS) <= len(tp)
    return tuple((tp[s:s + n], qp[s:s + n]) for n in SLICE_LENGTHS)


@functools.lru_cache(maxsize=None)
def ref_group(name: str, lookback: int) -> tuple:
    """tests/overlap_ref.py::chain of a set's group: (score, first, last, anchors in the chain).  Computed once per process."""
    return R.chain(*group(name), KW["k"], KW["bandwidth"], KW["max_gap"], lookback)


@functools.lru_cache(maxsize=None)
def ref_slices(lookback: int, max_gap: int) -> tuple:
    return tuple(R.chain(tp, qp, KW["k"], KW["bandwidth"], max_gap, lookback) for tp, qp in slices())


def chain_far_round_wins_ties(tp, qp, k: int, bandwidth: int, max_gap: int, lookback: int):
    """THE MUTANT of tests/overlap_ref.py::chain: the look-back walked in rounds of 64 from near to far, and a later round replaces the best
    where it is greater OR EQUAL — the natural bug of a kernel that works in rounds.  The reference lets it replace only where strictly greater."""
    tp, qp = np.asarray(tp, np.int64), np.asarray(qp, np.int64)
    n = len(tp)
    f, p = np.zeros(n, np.int64), np.full(n, -1, np.int64)
    for i in range(n):
        best, bp = k, -1
        for hi in range(i, max(0, i - lookback), -64):           # predecessors hi - 1 ... lo of one round, nearest first
            lo = max(0, i - lookback, hi - 64)
            dt, dq = tp[i] - tp[lo:hi][::-1], qp[i] - qp[lo:hi][::-1]
            dd = np.abs(dt - dq)
            ok = (dt > 0) & (dq > 0) & (dt <= max_gap) & (dq <= max_gap) & (dd <= bandwidth)
            sc = np.where(ok, f[lo:hi][::-1] + np.minimum(np.minimum(dt, dq), k) - ((dd * k) >> 6) - (R._ilog2(dd + 1) >> 1), np.iinfo(np.int64).min)
            j = int(np.argmax(sc))
            if sc[j] > k and sc[j] >= best:                      # (the reference: sc[j] > best)
                best, bp = int(sc[j]), hi - 1 - j
        f[i], p[i] = best, bp
    e = int(np.argmax(f))
    s, cnt = e, 1
    while p[s] >= 0:
        s, cnt = int(p[s]), cnt + 1
    return int(f[e]), s, e, cnt
