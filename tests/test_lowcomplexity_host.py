"""not-gpu: the front end's specifications (tests/overlap_ref.py, tests/extend_ref.py, tests/align_ref.py) on low-complexity reads
(tests/lowcomplexity.py): the census of the events the tie and edge rules govern, on the new sets and — the contrast — on random ones;
each specification against independent code on this material; what the finder's specification finds, pinned; three mutants of the
rules; what the material shows about fix_cigar's left shift.

The reference work of the whole file is shared through _CACHE and takes about a minute on one core."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import align_ref as A  # noqa: E402
import extend_ref as E  # noqa: E402
import lowcomplexity as LC  # noqa: E402
import overlap_ref as R  # noqa: E402
from herro_amd import synth  # noqa: E402

# the parameter sets tests/test_gpu_lowcomplexity.py runs the finder with
PARAM_SETS = [
    dict(max_occ=64, min_score=100),
    dict(k=15, w=5, max_occ=64, min_score=60),
    dict(k=16, w=8, max_occ=32, min_score=60),
    dict(k=15, w=5, max_occ=8, min_score=60),
]
GRID_SEED, SHRINK_SEED, PAL_SEED, HAND_SEED, GAP_SEED = 11, 12, 13, 14, 15

_CACHE = {}


def _cached(name, make):
    if name not in _CACHE:
        _CACHE[name] = make()
    return _CACHE[name]


def low():
    """the working set and its codes"""
    def make():
        ws = LC.working_set()
        return ws, ws.codes()
    return _cached("low", make)


def random_set():
    """the parts of test_gpu_overlap._batch at small size: five groups of eight reads around 3 kb, uniform random genomes"""
    def make():
        sb = synth.merge([
            synth.generate(1, 3000, 7, seed=51, p_partial=0.3, min_partial_len=1024),
            synth.generate(1, 3000, 7, seed=52, p_sub=0.01, p_ins=0.01, p_del=0.01, p_partial=0.3),
            synth.generate(1, 3000, 7, seed=53, p_sub=0.03, p_ins=0.025, p_del=0.025, p_partial=0.2),
            synth.generate(1, 3000, 7, seed=54, p_sub=0.002, p_ins=0.0015, p_del=0.0015),
            synth.generate(1, 3000, 7, seed=55, p_long_indel=0.003, p_partial=0.2),
        ])
        return sb, [R.store_codes(sb.read_seq(i)) for i in range(sb.n_reads)]
    return _cached("random", make)


def grid():
    def make():
        rd, rows, kinds = LC.lopsided_grid(np.random.default_rng(GRID_SEED))
        return rd, rows, kinds, [R.store_codes(r) for r in rd]
    return _cached("grid", make)


def palindrome():
    def make():
        rd = LC.palindromic_pair(np.random.default_rng(PAL_SEED))
        return rd, [R.store_codes(r) for r in rd]
    return _cached("pal", make)


def gapped():
    """90 records whose flanks hold a gap of 65-195 bases, their codes, and the reference's alignment of the whole reads"""
    def make():
        rd, rows = LC.gapped_flank_batch(np.random.default_rng(GAP_SEED), 90)
        codes = [R.store_codes(r) for r in rd]
        return rd, rows, codes, A.align_records(codes, LC.whole_rows(rows))
    return _cached("gapped", make)


def _aligned(name, codes, rows):
    """align_ref.align_records with the bases its fix_cigar left-shifts counted: (result, shifted bases, indels seen)"""
    def make():
        seen = [0, 0]
        per = _CACHE[name + " per record"] = []                  # the bases moved in every record that reaches fix_cigar, in order
        orig = A.fix_cigar

        def counting(cig, T, Q):
            per.append(LC.fix_cigar_shifted(cig, T, Q))
            seen[0] += per[-1]
            seen[1] += sum(1 for _, ty in cig if ty != A.M_)
            return orig(cig, T, Q)
        A.fix_cigar = counting
        try:
            res = A.align_records(codes, rows)
        finally:
            A.fix_cigar = orig
        return res, seen[0], seen[1]
    return _cached(name, make)


def grid_aligned():
    rd, rows, kinds, codes = grid()
    return _aligned("grid_aligned", codes, rows)


def low_aligned():
    ws, codes = low()
    return _aligned("low_aligned", codes, LC.true_rows(ws))


def low_sides():
    ws, codes = low()
    return _cached("sides", lambda: LC.short_sides(codes, LC.shrunk_rows(np.random.default_rng(SHRINK_SEED), ws), 63))


def random_sides():
    def make():
        sb, codes = random_set()
        rng = np.random.default_rng(SHRINK_SEED)
        rows = sb.aln[:, :9].astype(np.int64)
        sh = rng.integers(1, 64, (len(rows), 4))
        rows[:, 2] += sh[:, 0]; rows[:, 3] -= sh[:, 1]; rows[:, 7] += sh[:, 2]; rows[:, 8] -= sh[:, 3]
        return LC.short_sides(codes, rows.astype(np.uint32), 63)
    return _cached("random_sides", make)


# ---- 1. the sets keep their teeth ---------------------------------------------------------------------------------------------------------
def test_census_of_the_low_complexity_sets():
    ws, codes = low()
    assert len(ws.reads) == 24 and all(2300 <= len(r) <= 3800 for r in ws.reads) and sum(t[3] for t in ws.truth) == 6
    c25, c16, c15 = LC.census_sketch(codes, 25, 17), LC.census_sketch(codes, 16, 8), LC.census_sketch(codes, 15, 5)
    print(dict(c25=c25, c16=c16, c15=c15))
    # floors at about half of what the generator gives (101; 545; 5 421 and 897; 210; 208; 26 of 496)
    assert c25["runs3_repeated"] >= 50                          # hash runs of three or more reads, one of them more than once
    assert c16["palindromic"] >= 250 and c25["palindromic"] == 0 == c15["palindromic"]   # only an even k has them
    assert c15["repeated"] >= 2500 and c25["repeated"] >= 400
    assert LC.cut_hashes_in_true_overlaps(ws, 15, 5, 8) >= 100  # max_occ = 8 bites inside true overlaps ...
    assert LC.cut_hashes_in_true_overlaps(ws, 25, 17, 64) == 0  # ... the first parameter set's cut does not
    rd, rows, kinds, gcodes = grid()
    (out, cig, sc, ok, hend), _, _ = grid_aligned()
    assert len(rows) == 400 and LC.grid_net_indel_above(rows) >= 150 and ok.all()
    pal, pcodes = palindrome()
    assert LC.pairs_chained_on_both_strands(pcodes, k=15, w=5, min_score=60) >= 1
    assert LC.pairs_chained_on_both_strands(pcodes, min_score=100) >= 1
    sides = low_sides()
    tied = LC.tied_extension_sides(sides)
    assert len(sides) == 496 and tied >= 10
    # ... and the figures themselves, as DESIGN.md quotes them
    assert (c25["minimizers"], c25["repeated"], c25["runs3_repeated"]) == (8093, 897, 101)
    assert (c15["minimizers"], c15["repeated"], c15["runs3_repeated"], c16["palindromic"]) == (24265, 5421, 596, 545)
    assert (LC.cut_hashes_in_true_overlaps(ws, 15, 5, 8), LC.grid_net_indel_above(rows), tied) == (210, 208, 26)
    n_ops = [len(A.parse_cigar(x)) for x in cig]
    assert max(n_ops) == 205 and sum(1 for x in cig if len(A.parse_cigar(x)) == 1 and A.parse_cigar(x)[0][0] <= 2) == 129


def test_the_same_census_on_random_reads_is_empty():
    """the contrast: on the uniform random genomes of the suite's other sets the events above do not happen"""
    sb, codes = random_set()
    assert sb.n_reads == 40
    c25, c16, c15 = LC.census_sketch(codes, 25, 17), LC.census_sketch(codes, 16, 8), LC.census_sketch(codes, 15, 5)
    print(dict(c25=c25, c16=c16, c15=c15))
    assert (c25["runs3_repeated"], c25["repeated"], c15["runs3_repeated"], c15["repeated"]) == (0, 0, 0, 2)   # one 15-mer twice in one read, among 53 930 minimizers
    assert c16["palindromic"] == 2 and c16["repeated"] == 0
    assert (c25["minimizers"], c15["minimizers"]) == (17732, 53930)   # (not for lack of minimizers)
    for kw in PARAM_SETS:
        assert LC.pairs_chained_on_both_strands(codes, **kw) == 0
    assert LC.grid_net_indel_above(sb.aln) == 1 and len(sb.aln) == 35     # one record of the long-indel part
    sides = random_sides()
    # no contrast here: a mismatch and two matches behind the best cell repeat its H on random reads as well
    assert (len(sides), LC.tied_extension_sides(sides)) == (70, 7)


# ---- 2. the specification against independent code on this material -------------------------------------------------------------------
def _hash_slow(x: int, k: int) -> int:
    m = (1 << (2 * k)) - 1
    x = (~x + (x << 21)) & m
    x ^= x >> 24
    x = (x + (x << 3) + (x << 8)) & m
    x ^= x >> 14
    x = (x + (x << 2) + (x << 4)) & m
    x ^= x >> 28
    return (x + (x << 31)) & m


def _sketch_slow(codes, k, w):
    """the sketch window by window, python integers: [(hash, pos, strand)]"""
    c = [int(x) for x in codes]
    nk = len(c) - k + 1
    if nk < w:
        return []
    hs, ss = [], []
    for i in range(nk):
        f = r = 0
        for j in range(k):
            f = (f << 2) | c[i + j]
            r |= (3 - c[i + j]) << (2 * j)
        hs.append(None if f == r else _hash_slow(min(f, r), k))
        ss.append(int(r < f))
    sel = set()
    for s in range(nk - w + 1):
        real = [h for h in hs[s:s + w] if h is not None]
        if real:
            lo = min(real)
            sel.update(s + o for o in range(w) if hs[s + o] == lo)
    return [(hs[i], i + k - 1, ss[i]) for i in sorted(sel)]


def test_sketch_equals_a_loop_over_windows():
    ws, codes = low()
    extra, _, _ = LC.short_and_n_reads()
    assert any(b"N" in r for r in extra) and min(len(r) for r in extra) < 9
    some = [codes[0][:1200], codes[11][:1200], codes[20][-1200:]] + [R.store_codes(r) for r in extra]
    pal = 0
    for k, w in ((25, 17), (16, 8), (6, 4), (30, 64), (15, 5)):
        for c in some:
            h, p, s = R.sketch(c, k, w)
            assert list(zip(h.tolist(), p.tolist(), s.tolist())) == _sketch_slow(c, k, w), (k, w, len(c))
            if k % 2 == 0:
                f, r = R.kmers(c, k)
                pal += int((f == r).sum())
    assert pal >= 100                                            # windows that hold a k-mer equal to its reverse complement were met


def test_chain_equals_chain_many_group_for_group():
    ws, codes = low()
    lens = np.array([len(c) for c in codes], np.int64)
    a = R.anchors(*R.sketch_store(codes, 15, 5), lens, 15, 64)
    b = np.flatnonzero(np.concatenate([[True], (a[1:, :3] != a[:-1, :3]).any(axis=1), [True]]))
    size = np.diff(b)
    pick = np.argsort(-size, kind="stable")[:40].tolist() + np.flatnonzero(size <= 3)[:40].tolist()
    tps, qps = [a[b[g]:b[g + 1], 3] for g in pick], [a[b[g]:b[g + 1], 4] for g in pick]
    assert max(len(t) for t in tps) > 300 and any((np.diff(t) == 0).any() for t in tps)     # several anchors on one target position
    assert R.chain_many(tps, qps, 15, 150, 5000) == [R.chain(t, q, 15, 150, 5000) for t, q in zip(tps, qps)]


def _valid(cig, out, sc, codes):
    ops = A.parse_cigar(cig)
    assert all(ln > 0 for ln, _ in ops) and all(x[1] != y[1] for x, y in zip(ops, ops[1:]))
    assert ops[0][1] == A.M_ and ops[-1][1] == A.M_ and out[9] == len(cig)
    T, Q = A.record_seqs(codes, out)
    assert A.score_cigar(ops, T, Q) == sc


N_PIECES = 23


def test_banded_gotoh_on_the_grid_and_on_low_complexity_pairs():
    rd, rows, kinds, gcodes = grid()
    (out, cig, sc, ok, hend), _, _ = grid_aligned()
    assert ok.all()
    for r in range(len(rows)):
        _valid(cig[r], out[r], sc[r], gcodes)
    small = [r for r in range(len(rows)) if rows[r, 1] <= 129 and rows[r, 6] <= 129]
    assert len(small) == 256
    for r in small:                                              # the band pushed along the matrix edge loses nothing
        T, Q = A.record_seqs(gcodes, rows[r])
        assert hend[r] == A.gotoh_unbanded(T, Q), (rows[r].tolist(), kinds[r])
    # 500-bp pieces of the working set's true pairs, cut where the two reads show the same genome position
    ws, codes = low()
    pieces = []
    for (t, q), (strand, (t0, t1), (q0, q1)) in list(LC.true_pairs(ws).items())[:24]:
        gt, gq = ws.gpos[t], ws.gpos[q]
        a = t0 + 200
        want = gt[a], gt[a + 500]
        qa, qb = (int(np.flatnonzero(gq == x)[0]) if len(np.flatnonzero(gq == x)) else -1 for x in want)
        if qa < 0 or qb < 0:
            continue
        qa, qb = (qa, qb) if qa < qb else (qb + 1, qa + 1)
        pieces.append([q, len(ws.reads[q]), qa, qb, strand, t, len(ws.reads[t]), a, a + 500])
    print(len(pieces))
    assert len(pieces) == N_PIECES
    pieces = np.array(pieces, np.uint32)
    assert int(np.abs((pieces[:, 3] - pieces[:, 2]).astype(np.int64) - 500).max()) <= 60
    p_out, p_cig, p_sc, p_ok, p_hend = A.align_records(codes, pieces)
    assert p_ok.all()
    for r in range(len(pieces)):
        T, Q = A.record_seqs(codes, pieces[r])
        assert p_hend[r] == A.gotoh_unbanded(T, Q), pieces[r].tolist()
        _valid(p_cig[r], p_out[r], p_sc[r], codes)


def test_the_band_follows_a_gap_wider_than_its_half_along_its_edge_cells():
    """A gap of 65-195 bases right behind the span: the path runs in the band's bottom cell (the target has the bases) or its top cell
    (the query has them) while the band moves.  The bottom cell of a band that has just moved has its upper and diagonal neighbours in
    the band of their own diagonals — k_align and k_extend once read -inf there; tests/test_gpu_lowcomplexity.py holds them to this."""
    rd, rows, codes, (out, cig, sc, ok, hend) = gapped()
    assert len(rows) == 90 and ok.all() and set(rows[:, 4].tolist()) == {0, 1}
    for r in range(len(rows)):
        _valid(cig[r], out[r], sc[r], codes)
    gaps = [max(ln for ln, ty in A.parse_cigar(x) if ty != A.M_) for x in cig]
    assert sum(1 for g in gaps if g >= 65) >= 30                 # ... found as one gap, in both directions
    assert sum(1 for x in cig if any(ln >= 65 and ty == A.I_ for ln, ty in A.parse_cigar(x))) >= 10
    assert sum(1 for x in cig if any(ln >= 65 and ty == A.D_ for ln, ty in A.parse_cigar(x))) >= 10
    ext = E.extend_records(codes, rows)[1].astype(np.int64)
    assert (np.abs(ext[:, 2] - ext[:, 3]) >= 65).sum() >= 15 and not ext[:, :2].any()


def test_extension_equals_the_whole_matrix_on_short_flanks():
    sides = low_sides()
    res = E.extend_sides(sides, E.ZDROP)
    assert (res[:, 0] > 0).sum() >= 100
    for (T, Q), r in zip(sides, res):
        got = tuple(int(x) for x in r[:3])
        assert got == E.extend_unbanded(T, Q) == LC.best_cell(LC.whole_matrix(T, Q))[0], (T.tolist(), Q.tolist())


# ---- 3. what the specification finds ----------------------------------------------------------------------------------------------------------
# minimizers, anchors, pairs found, (missed, wrong strand, cross-group) of the 62 true pairs of >= 1 000 bp, least coverage of the true span
FOUND = [
    (8093, 6838, 75, (0, 0, 0), 0.634),
    (24265, 35654, 78, (0, 0, 0), 0.888),
    (16198, 18794, 78, (0, 0, 0), 0.871),
    (24265, 14068, 78, (0, 0, 0), 0.871),
]


@pytest.mark.parametrize("case", range(len(PARAM_SETS)))
def test_what_the_finder_finds_on_the_working_set(case):
    ws, codes = low()
    assert len(LC.true_pairs(ws)) == 62
    st = {}
    R.find_overlaps(codes, stats=st, **PARAM_SETS[case])
    miss, wrong, cross, cov = LC.evaluate(ws, st["pairs"])
    got = (st["minimizers"], st["anchors"], len(st["pairs"]), (miss, wrong, cross), round(cov, 3))
    print(PARAM_SETS[case], got)
    assert got == FOUND[case]


# ---- 4. mutants -----------------------------------------------------------------------------------------------------------------------------
def _sketch_leftmost_only(codes, k, w):
    """overlap_ref.sketch with one rule changed: of equal minima in a window only the leftmost is selected"""
    nk = len(codes) - k + 1
    if nk < w:
        return np.zeros(0, np.uint64), np.zeros(0, np.int64), np.zeros(0, np.uint8)
    f, r = R.kmers(codes, k)
    h = np.where(f == r, R.INF, R.hash64(np.minimum(f, r), k))
    st = (r < f).astype(np.uint8)
    win = np.lib.stride_tricks.sliding_window_view(h, w)
    first = np.arange(nk - w + 1) + win.argmin(axis=1)
    idx = np.unique(first[win.min(axis=1) != R.INF])
    return h[idx], idx + (k - 1), st[idx]


def _pick_strand_1_on_a_tie(chains):
    best = {}
    for t, q, rel, sc, ts, te, qs, qe, cnt in chains:
        cur = best.get((t, q))
        if cur is None or sc >= cur[0]:
            best[(t, q)] = (sc, rel, ts, te, qs, qe, cnt)
    return best


def _found(codes, **kw):
    rids, rows, off, sc = R.find_overlaps(codes, **kw)
    return rids.tolist(), rows.tolist(), off.tolist(), sc.tolist()


def test_two_mutants_are_caught_by_the_new_sets_only(monkeypatch):
    ws, codes = low()
    sb, rcodes = random_set()
    pal, pcodes = palindrome()
    kw = PARAM_SETS[1]
    want_low, want_rand, want_pal = _found(codes, **kw), _found(rcodes, **kw), _found(pcodes, **kw)
    assert len(want_low[1]) > 100 and len(want_rand[1]) > 100 and len(want_pal[1]) == 2
    with monkeypatch.context() as m:
        m.setattr(R, "sketch", _sketch_leftmost_only)
        assert _found(codes, **kw) != want_low
        assert _found(rcodes, **kw) == want_rand
        h = R.sketch_store(codes, 15, 5)[0]
    assert len(h) < len(R.sketch_store(codes, 15, 5)[0])
    with monkeypatch.context() as m:
        m.setattr(R, "pick_strands", _pick_strand_1_on_a_tie)
        got = _found(pcodes, **kw)
        assert got != want_pal and [r[4] for r in got[1]] == [1, 1] and [r[4] for r in want_pal[1]] == [0, 0]
        assert _found(rcodes, **kw) == want_rand
        assert _found(codes, **kw) == want_low               # no read pair of the working set chains on both strands (section 1)


def _differs(a, b):
    """records on which two results of align_records differ (CIGAR, coordinates, score or ok)"""
    return [r for r in range(len(a[1])) if a[1][r] != b[1][r] or not np.array_equal(a[0][r], b[0][r]) or a[2][r] != b[2][r] or a[3][r] != b[3][r]]


def _ext_differs(a, b):
    return np.flatnonzero(np.any([(x != y).any(axis=1) for x, y in zip(a, b)], axis=0)).tolist()


def test_a_bottom_cell_that_forgets_is_caught_where_a_gap_is_wider_than_half_the_band(monkeypatch):
    """The third mutant is what k_align and k_extend did before these sets existed: after the band has moved, its new bottom cell read -inf
    above and diagonally below itself although those cells lay in the band of their own diagonals.  The grid catches it on one record,
    the gapped records on twelve alignments and three extensions; the reads of the working set and the repeat flanks do not."""
    rd, rows, kinds, gcodes = grid()
    ws, codes = low()
    g_rd, g_rows, g_codes, g_ref = gapped()
    shrunk = LC.shrunk_rows(np.random.default_rng(SHRINK_SEED), ws)
    h_rd, h_rows = LC.hand_flank_batch(np.random.default_rng(HAND_SEED), LC.GRID_LENGTHS)
    h_codes = [R.store_codes(r) for r in h_rd]
    ext_params = [dict(), dict(max_ext=50), dict(zdrop=30)]      # test_gpu_extend.PARAMS
    want_ext = [E.extend_records(g_codes, g_rows, **kw) for kw in ext_params]
    want_shrunk, want_hand = E.extend_records(codes, shrunk), E.extend_records(h_codes, h_rows)
    grid_ref, low_ref = grid_aligned()[0], low_aligned()[0]
    monkeypatch.setattr(A, "BOTTOM_CELL_FORGETS", True)
    got_grid = A.align_records(gcodes, rows)
    assert _differs(got_grid, grid_ref) == [89] and kinds[89] == "one_gap" and rows[89, [1, 6]].tolist() == [300, 600]
    assert (int(grid_ref[2][89]), int(got_grid[2][89])) == (-328, -352)
    assert len(_differs(A.align_records(g_codes, LC.whole_rows(g_rows)), g_ref)) == 12
    assert [len(_ext_differs(E.extend_records(g_codes, g_rows, **kw), w)) for kw, w in zip(ext_params, want_ext)] == [3, 0, 0]
    some = A.align_records(codes, LC.true_rows(ws)[:20])         # (twenty of the 62 true pairs keep this within seconds)
    assert _differs(some, tuple(x[:20] for x in low_ref)) == []
    assert _ext_differs(E.extend_records(codes, shrunk), want_shrunk) == [] and _ext_differs(E.extend_records(h_codes, h_rows), want_hand) == []


def test_the_palindromic_pairs_two_chains_tie():
    pal, pcodes = palindrome()
    for kw in (PARAM_SETS[0], PARAM_SETS[1]):
        ch = LC.chains(pcodes, **kw)
        assert [c[:3] for c in ch] == [(0, 1, 0), (0, 1, 1)]
        assert ch[0][3] == ch[1][3] and ch[0][8] == ch[1][8] and ch[0][3] > 1000
        st = {}
        R.find_overlaps(pcodes, stats=st, **kw)
        assert st["pairs"][(0, 1)][:2] == (ch[0][3], 0)


# ---- 5. fix_cigar's left shift -------------------------------------------------------------------------------------------------------------
SHIFTED = ((732, 1869), (0, 6090))          # (bases moved, indels seen): the grid, the working set's 62 true pairs


def test_what_the_left_shift_of_fix_cigar_moves():
    """On the reads of the working set the DP's own tie order already leaves every gap leftmost: the loop moves nothing.  On the grid's
    homopolymer and 3-bp-repeat records it does: there the band is pushed along the matrix edge, the gap lies where the band let it,
    and the shift carries it to the front.  (The golden vectors of tests/test_align_host.py stay fix_cigar's own test.)"""
    _, g_moved, g_indels = grid_aligned()
    (out, cig, sc, ok, hend), l_moved, l_indels = low_aligned()
    assert ok.all() and len(ok) == 62
    print(dict(grid=(g_moved, g_indels), low=(l_moved, l_indels)))
    assert ((g_moved, g_indels), (l_moved, l_indels)) == SHIFTED
    per, kinds = _CACHE["grid_aligned per record"], grid()[2]
    assert len(per) == 400                                       # every grid record aligns: one call each, in order
    assert {k: sum(m for m, kind in zip(per, kinds) if kind == k) for k in LC.GRID_KINDS} == \
        dict(one_gap=0, unrelated=0, homopolymer=372, repeat3=360)
