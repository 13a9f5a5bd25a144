"""not-gpu: the overlap finder's specification (tests/overlap_ref.py) on hand cases and on seeded synthetic sets,
the hash, and the error codes herro_find_overlaps returns without a device.

The whole file takes about 8 s on one core (the reference finds the 312 pairs of the first synthetic set in 0.3 s at k = 25, the
234 of the third in under 2 s at k = 15)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import overlap_ref as R  # noqa: E402
from herro_amd import api, synth  # noqa: E402

COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _codes(seq: bytes):
    return R.store_codes(seq)


def _rand(rng, n) -> bytes:
    return bytes(b"ACGT"[x] for x in rng.integers(0, 4, n))


def _rc(seq: bytes) -> bytes:
    return seq.translate(COMP)[::-1]


def _sketch_slow(codes, k, w):
    """the sketch straight from its definition, in python integers"""
    n = len(codes)
    nk = n - k + 1
    if nk < w:
        return []
    mask = (1 << (2 * k)) - 1
    hs, ss = [], []
    for i in range(nk):
        f = r = 0
        for j in range(k):
            f = (f << 2) | int(codes[i + j])
            r |= (3 - int(codes[i + j])) << (2 * j)
        hs.append(None if f == r else int(R.hash64(np.array([min(f, r)], np.uint64), k)[0]) & mask)
        ss.append(int(r < f))
    sel = set()
    for s in range(nk - w + 1):
        real = [h for h in hs[s:s + w] if h is not None]
        if real:
            m = min(real)
            sel |= {s + o for o in range(w) if hs[s + o] == m}
    return [(hs[i], i + k - 1, ss[i]) for i in sorted(sel)]


def test_sketch_equals_its_definition():
    rng = np.random.default_rng(1)
    for trial, (k, w) in enumerate([(5, 3), (6, 1), (6, 4), (9, 17), (15, 5), (25, 17), (31, 64)]):
        seq = _rand(rng, 150 + 40 * trial) + b"ACGTACGTACGTACGTACGT" * 3 + b"NNNN" + _rand(rng, 60)
        c = _codes(seq)
        h, p, s = R.sketch(c, k, w)
        assert list(zip(h.tolist(), p.tolist(), s.tolist())) == _sketch_slow(c, k, w), (k, w)


def test_a_kmer_equal_to_its_reverse_complement_is_never_selected():
    seq = b"TTTTTTTTACGCGTGGGGGGGG"          # ACGCGT is its own reverse complement
    c = _codes(seq)
    f, r = R.kmers(c, 6)
    pal = np.flatnonzero(f == r)
    assert pal.tolist() == [8]
    h, p, s = R.sketch(c, 6, 1)               # w = 1: every k-mer is the minimum of its own window
    assert sorted(set(range(5, len(seq))) - set(p.tolist())) == [8 + 5]
    for w in (2, 3, 7):
        assert 13 not in R.sketch(c, 6, w)[1].tolist()


def test_tied_window_minima_select_all():
    seq = b"ACGGTCA" * 12                      # period 7 < w: every window holds its minimum more than once
    c = _codes(seq)
    h, p, s = R.sketch(c, 5, 16)
    assert len(np.unique(h)) == 1
    assert np.array_equal(np.diff(p), np.full(len(p) - 1, 7)) and len(p) >= 10
    allh = R.hash64(np.minimum(*R.kmers(c, 5)), 5)
    assert h[0] == allh.min()                  # both copies inside one window of 16 are there: no left / right rule


def test_short_reads_have_no_minimizer():
    rng = np.random.default_rng(2)
    for k, w in ((25, 17), (15, 5), (31, 64)):
        assert len(R.sketch(_codes(_rand(rng, k + w - 2)), k, w)[0]) == 0
        assert len(R.sketch(_codes(_rand(rng, k + w - 1)), k, w)[0]) >= 1


def test_reverse_strand_anchors_lie_on_one_diagonal():
    rng = np.random.default_rng(3)
    a = _rand(rng, 600)
    b = _rand(rng, 150) + _rc(a[100:500]) + _rand(rng, 90)
    codes = [_codes(a), _codes(b)]
    lens = np.array([len(a), len(b)])
    h, rid, pos, st = R.sketch_store(codes, 15, 5)
    an = R.anchors(h, rid, pos, st, lens, 15, 128)
    rev = an[an[:, 2] == 1]
    assert len(rev) >= 30 and len(rev) >= 0.9 * len(an)
    # a[100 + x] pairs with base x of rc(b)[90:490], i.e. tpos - qpos = 100 - 90 on the query's reverse complement
    assert set((rev[:, 3] - rev[:, 4]).tolist()) == {10}
    rids, rows, off, sc = R.find_overlaps(codes, k=15, w=5, min_score=100)
    assert rids.tolist() == [0, 1] and off.tolist() == [0, 1, 2]
    qid, qlen, qs, qe, strand, tid, tlen, ts, te, cl = (int(x) for x in rows[0])
    assert (qid, tid, strand, qlen, tlen, cl) == (1, 0, 1, len(b), len(a), 0)
    assert 95 <= ts < 130 and 470 < te <= 505 and 145 <= qs < 180 and 520 < qe <= 555   # (a flanking base may match by chance)
    assert _rc(b[qs:qe]) == a[ts:te]           # the anchor span begins and ends on an exact k-mer match; here nothing differs in between


def test_chain_tie_rules():
    k = 15
    # two predecessors give 30: (100, 100) and (100, 104) both reach (200, 202) at |dt - dq| = 2, cost 0 — the nearest wins
    assert R.chain([100, 100, 200], [100, 104, 202], k, 150, 5000) == (30, 1, 2, 2)
    # two chains of equal score: the one ending first
    assert R.chain([100, 120, 10000, 10020], [100, 120, 10000, 10020], k, 150, 5000) == (30, 0, 1, 2)
    assert R.chain_many([[100, 100, 200], [100, 120, 10000, 10020]], [[100, 104, 202], [100, 120, 10000, 10020]], k, 150, 5000) == \
        [(30, 1, 2, 2), (30, 0, 1, 2)]
    # the gap cost: |dt - dq| = 70 costs (70 * 15 >> 6) + (floor(log2 71) >> 1) = 16 + 3 > 15: not worth chaining
    assert R.chain([100, 300], [100, 230], k, 150, 5000) == (15, 0, 0, 1)
    assert R.chain([100, 300], [100, 260], k, 150, 5000) == (15 + 15 - 9 - 2, 0, 1, 2)
    # max_gap, bandwidth and "0 < dt, dq" are conditions, not costs
    assert R.chain([100, 5101], [100, 5101], k, 150, 5000)[0] == 15 and R.chain([100, 5100], [100, 5100], k, 150, 5000)[0] == 30
    assert R.chain([100, 300], [100, 320], k, 20, 5000) == (15 + 15 - 4 - 2, 0, 1, 2) and R.chain([100, 300], [100, 320], k, 19, 5000)[3] == 1
    assert R.chain([100, 100], [100, 140], k, 150, 5000)[3] == 1 and R.chain([100, 140], [100, 100], k, 150, 5000)[3] == 1
    # the better strand, strand 0 on a tie
    assert R.pick_strands([(0, 1, 0, 50, 1, 2, 3, 4, 5), (0, 1, 1, 50, 6, 7, 8, 9, 5)])[(0, 1)][:2] == (50, 0)
    assert R.pick_strands([(0, 1, 0, 50, 1, 2, 3, 4, 5), (0, 1, 1, 51, 6, 7, 8, 9, 5)])[(0, 1)][:2] == (51, 1)


def test_chain_many_equals_chain():
    rng = np.random.default_rng(4)
    tps, qps = [], []
    for g in range(40):
        n = int(rng.integers(1, 300))
        d = int(rng.integers(-50, 50))
        t = np.sort(rng.integers(0, 3000, n))
        q = t + d + rng.integers(-4, 5, n) * (rng.random(n) < 0.3)
        extra = rng.integers(0, 3000, (n // 3, 2))          # off-diagonal noise
        a = np.unique(np.concatenate([np.stack([t, q], 1), extra]), axis=0)
        a = a[np.lexsort((a[:, 1], a[:, 0]))]
        tps.append(a[:, 0]); qps.append(a[:, 1])
    for k, bw, gap, H in ((15, 150, 5000, 64), (25, 20, 300, 64), (15, 150, 5000, 5)):
        assert R.chain_many(tps, qps, k, bw, gap, H) == [R.chain(t, q, k, bw, gap, H) for t, q in zip(tps, qps)]


def test_lookback_limit_counts_anchors():
    """70 off-diagonal anchors between two anchors of the diagonal: a look-back of 64 cannot join them, an unlimited one can."""
    t = [100] + [110] * 70 + [120]
    q = [100] + list(range(1000, 1070)) + [120]
    assert R.chain(t, q, 15, 150, 5000)[0] == 15
    assert R.chain(t, q, 15, 150, 5000, None) == (30, 0, 71, 2)


def test_max_occ_drops_a_repeated_hash():
    rng = np.random.default_rng(5)
    reads = [_rand(rng, 200)] * 5                              # every minimizer occurs once per read: 5 times in the store
    codes = [_codes(r) for r in reads]
    lens = np.array([len(r) for r in reads])
    h, rid, pos, st = R.sketch_store(codes, 15, 5)
    full = R.anchors(h, rid, pos, st, lens, 15, 5)
    assert len(h) % 5 == 0 and len(h) >= 100 and len(full) == 10 * (len(h) // 5)   # 10 pairs of reads per minimizer
    assert len(R.anchors(h, rid, pos, st, lens, 15, 4)) == 0
    assert (full[:, 0] < full[:, 1]).all()


def _pair(seed=6):
    rng = np.random.default_rng(seed)
    core = _rand(rng, 700)
    return [_codes(_rand(rng, 100) + core + _rand(rng, 50)), _codes(_rand(rng, 30) + core + _rand(rng, 200))]


def test_min_score_and_min_anchors_at_their_boundaries():
    codes = _pair()
    st = {}
    rids, rows, off, sc = R.find_overlaps(codes, k=15, w=5, min_score=1, min_anchors=1, stats=st)
    score, rel, ts, te, qs, qe, cnt = st["pairs"][(0, 1)]
    assert len(rows) == 2 and score > 200 and cnt > 20 and rel == 0
    assert len(R.find_overlaps(codes, k=15, w=5, min_score=score, min_anchors=cnt)[1]) == 2
    assert len(R.find_overlaps(codes, k=15, w=5, min_score=score + 1, min_anchors=1)[1]) == 0
    assert len(R.find_overlaps(codes, k=15, w=5, min_score=1, min_anchors=cnt + 1)[1]) == 0
    assert len(R.find_overlaps(codes)[1]) == 0              # the default -m 2500 needs reads of ~10 kb


def test_dual_records_mirror_each_other():
    rng = np.random.default_rng(7)
    g = _rand(rng, 3000)
    reads = [g[0:1500], g[700:2400], _rc(g[1200:3000]), _rand(rng, 900)]
    rids, rows, off, sc = R.find_overlaps([_codes(r) for r in reads], k=15, w=5, min_score=100)
    assert rids.tolist() == [0, 1, 2] and off.tolist() == [0, 2, 4, 6]
    by = {(int(r[5]), int(r[0])): (r, s) for r, s in zip(rows, sc)}
    assert sorted(by) == [(0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1)]
    for (t, q), (r, s) in by.items():
        m, ms = by[(q, t)]
        assert r[:4].tolist() == m[5:9].tolist() and r[5:9].tolist() == m[:4].tolist() and r[4] == m[4] and s == ms and r[9] == 0
    assert by[(0, 1)][0][4] == 0 and by[(0, 2)][0][4] == 1 and by[(1, 2)][0][4] == 1
    for t in range(3):                                         # ascending qid inside a target
        q = rows[int(off[t]):int(off[t + 1]), 0]
        assert (np.diff(q.astype(np.int64)) > 0).all() and (rows[int(off[t]):int(off[t + 1]), 5] == rids[t]).all()


def test_the_hash_is_a_bijection():
    assert sorted(R.hash64(np.arange(1 << 10, dtype=np.uint64), 5).tolist()) == list(range(1 << 10))
    rng = np.random.default_rng(8)
    x = rng.integers(0, 1 << 50, 2000).astype(np.uint64)
    y = R.hash64(x, 25)
    assert (y < (1 << 50)).all()
    assert [R.hash64_inverse(int(v), 25) for v in y] == x.tolist()
    for k in (5, 15, 31):
        v = rng.integers(0, 1 << (2 * k), 200).astype(np.uint64)
        assert [R.hash64_inverse(int(u), k) for u in R.hash64(v, k)] == v.tolist()


def test_error_codes_without_a_device():
    c = api.HostContext([100, 200, 300])
    with pytest.raises(api.HerroError) as e:
        c.find_overlaps()
    assert e.value.code == -2                                  # HERRO_E_NO_DEVICE
    with pytest.raises(api.HerroError) as e:
        c.sketch()
    assert e.value.code == -2
    for bad in (dict(k=32), dict(k=4), dict(w=65), dict(w=0), dict(k=0)):
        with pytest.raises(api.HerroError) as e:
            c.find_overlaps(**bad)
        assert e.value.code == -1, bad                         # HERRO_E_INVALID, before anything else
    # the C entry itself (the binding checks k and w too): k = 32 and w = 65 through the struct
    import ctypes as C
    L = api.lib()
    for k, w in ((32, 0), (0, 65), (4, 17)):
        p = api.OverlapParams(k=k, w=w)
        h = C.c_void_p()
        assert L.herro_find_overlaps(c.h, C.byref(p), C.byref(h)) == -1 and not h.value
        assert L.herro_debug_sketch(c.h, C.byref(p), None, None, None, None, 0) == -1
    h = C.c_void_p()
    assert L.herro_find_overlaps(c.h, None, C.byref(h)) == -2  # NULL parameters: the defaults
    assert L.herro_find_overlaps(None, None, C.byref(h)) == -1
    assert L.herro_overlaps_n(None) == 0 and L.herro_overlaps_n_targets(None) == 0
    L.herro_overlaps_free(None)


def evaluate(sb, pairs):
    """(missed, wrong strand, cross-group pairs, min coverage of the true target span) of {(t, q): (score, rel, ts, te, qs, qe, ..)}"""
    grp = np.full(sb.n_reads, -1, np.int64)
    for ti in range(sb.n_targets):
        grp[int(sb.tgt_rid[ti])] = ti
        grp[sb.aln[int(sb.tgt_aln_off[ti]):int(sb.tgt_aln_off[ti + 1]), 0].astype(np.int64)] = ti
    cross = sum(1 for (t, q) in pairs if grp[t] != grp[q])
    miss = wrong = 0
    cov = []
    for a in sb.aln:
        qid, qlen, qs, qe, strand, tid, tlen, ts, te = (int(x) for x in a[:9])
        r = pairs.get((min(tid, qid), max(tid, qid)))
        if r is None:
            miss += 1
            continue
        fts, fte = (r[2], r[3]) if tid < qid else (r[4], r[5])
        wrong += int(r[1] != strand)
        cov.append(max(0, min(te, fte) - max(ts, fts)) / max(1, te - ts))
    return miss, wrong, cross, min(cov) if cov else 0.0


SETS = [   # generator arguments, (k, w), the least coverage of the true target span
    (dict(n_targets=4, target_len=4096, n_overlaps=12, seed=21), (25, 17), 0.90),
    (dict(n_targets=3, target_len=4096, n_overlaps=12, seed=23, p_partial=0.3, min_partial_len=1024), (25, 17), 0.90),
    (dict(n_targets=3, target_len=4096, n_overlaps=12, seed=22, p_sub=0.01, p_ins=0.01, p_del=0.01), (25, 17), 0.85),   # 3 % per read
    (dict(n_targets=3, target_len=4096, n_overlaps=12, seed=22, p_sub=0.01, p_ins=0.01, p_del=0.01), (15, 5), 0.90),
]


@pytest.mark.parametrize("case", range(len(SETS)))
def test_every_true_pair_of_a_synthetic_set_is_found(case):
    kw, (k, w), least = SETS[case]
    sb = synth.generate(**kw)
    codes = [R.store_codes(sb.read_seq(i)) for i in range(sb.n_reads)]
    st = {}
    R.find_overlaps(codes, k=k, w=w, max_occ=64, min_score=100, stats=st)
    miss, wrong, cross, cov = evaluate(sb, st["pairs"])
    print(kw, k, w, "pairs", len(st["pairs"]), "missed", miss, "wrong strand", wrong, "cross-group", cross, "min coverage %.3f" % cov)
    assert (miss, wrong, cross) == (0, 0, 0)
    assert cov >= least
    if case == 0:
        assert len(st["pairs"]) == 312                       # target-query and query-query pairs of 4 groups of 13 reads
