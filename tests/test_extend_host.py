"""not-gpu: the end extension's specification (tests/extend_ref.py) on hand cases, its strand symmetry, the "entered by
a match" property, what it recovers on the seeded synthetic sets of test_overlap_host.py, and the error codes herro_extend_overlaps
returns without a device.

The sets take ~2 s each on one core: only the target-query records (the ones the generator knows the truth of) are extended, and all
their sides run through the reference together."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import extend_ref as E  # noqa: E402
import overlap_ref as R  # noqa: E402
from test_overlap_host import SETS  # noqa: E402
from herro_amd import api, synth  # noqa: E402

COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _rand(rng, n, alphabet=b"ACGT") -> bytes:
    return bytes(alphabet[x] for x in rng.integers(0, len(alphabet), n))


def _rc(seq: bytes) -> bytes:
    return seq.translate(COMP)[::-1]


CORE = _rand(np.random.default_rng(100), 120)


def _record(t_left=b"", t_right=b"", q_left=b"", q_right=b"", **kw):
    """A strand-0 record whose span is CORE on both reads; the flanks are written in read order (t_left + CORE + t_right).
    Returns (ext [t_left, q_left, t_right, q_right], scores [left, right], rows_out) of the reference."""
    t = t_left + CORE + t_right
    q = q_left + CORE + q_right
    row = np.array([[1, len(q), len(q_left), len(q_left) + len(CORE), 0, 0, len(t), len(t_left), len(t_left) + len(CORE)]], np.uint32)
    out, ext, sc = E.extend_records([E.store_codes(t), E.store_codes(q)], row, **kw)
    # the coordinates follow from the lengths
    assert out[0, 7] == len(t_left) - ext[0, 0] and out[0, 8] == len(t_left) + len(CORE) + ext[0, 2]
    assert out[0, 2] == len(q_left) - ext[0, 1] and out[0, 3] == len(q_left) + len(CORE) + ext[0, 3] and out[0, 9] == 0
    return ext[0].tolist(), sc[0].tolist(), out[0]


def test_identical_flanks_extend_to_the_shorter_reads_end():
    rng = np.random.default_rng(101)
    F, X, Y = _rand(rng, 80), _rand(rng, 30), _rand(rng, 40)
    # right: the query read ends 50 bases behind the span, the target goes on; left: the target read starts 30 bases in front of it
    ext, sc, _ = _record(t_left=X, q_left=Y + X, t_right=F, q_right=F[:50])
    assert ext == [30, 30, 50, 50] and sc == [60, 100]


def test_a_mismatch_right_at_the_boundary_is_crossed():
    F = _rand(np.random.default_rng(102), 39)
    ext, sc, _ = _record(t_right=b"A" + F, q_right=b"C" + F)
    assert ext == [0, 0, 40, 40] and sc == [0, -4 + 2 * 39]
    # ... on the left too (the flank is read away from the span: its last base is the boundary)
    ext, sc, _ = _record(t_left=F + b"A", q_left=F + b"C")
    assert ext == [40, 40, 0, 0] and sc == [-4 + 2 * 39, 0]


def test_first_flank_base_differs_extension_0():
    assert _record(t_right=b"A", q_right=b"C")[:2] == ([0, 0, 0, 0], [0, 0])
    assert _record(t_right=b"AG", q_right=b"CG")[:2] == ([0, 0, 0, 0], [0, 0])           # -4 + 2 < 0
    assert _record(t_right=b"A" * 200, q_right=b"C" * 200, t_left=b"G" * 70, q_left=b"T" * 90)[:2] == ([0, 0, 0, 0], [0, 0])
    assert _record(t_right=b"AGG", q_right=b"CGG")[:2] == ([0, 0, 0, 0], [0, 0])         # -4 + 4 = 0 is not greater than 0
    assert _record(t_right=b"AGGT", q_right=b"CGGT")[:2] == ([0, 0, 4, 4], [0, 2])


def test_a_three_base_indel_in_the_flank():
    F = _rand(np.random.default_rng(103), 80)
    cut = F[:30] + F[33:]
    ext, sc, _ = _record(t_right=cut, q_right=F)                # the query has three bases more: an insertion
    assert ext == [0, 0, 77, 80] and sc == [0, 2 * 77 - 10]
    ext, sc, _ = _record(t_right=F, q_right=cut)                # ... a deletion
    assert ext == [0, 0, 80, 77] and sc == [0, 2 * 77 - 10]
    ext, sc, _ = _record(t_left=F, q_left=cut)
    assert ext == [80, 77, 0, 0] and sc == [2 * 77 - 10, 0]


def test_a_flank_that_turns_random_stops_at_the_last_match():
    F = _rand(np.random.default_rng(104), 60)
    # the tails never match: the best cell is the last base of F, and the sweep gives up once it is 400 below it.  On even
    # diagonals the best cell is the main diagonal's: 120 - 2 (d - 120) < 120 - 400 first holds at d = 322, odd diagonals lie
    # lower, so the check of d = 336 is the first to stop (that of 320 sees -280, which is not below -280)
    ext, sc, _ = _record(t_right=F + b"A" * 300, q_right=F + b"C" * 300)
    assert ext == [0, 0, 60, 60] and sc == [0, 120]
    t, q = E.store_codes(F + b"A" * 300), E.store_codes(F + b"C" * 300)
    assert E.extend_sides([(t, q)], 400).tolist() == [[120, 60, 60, 336]]
    assert E.extend_sides([(t, q)], 100000).tolist() == [[120, 60, 60, 720]]
    # random tails: whatever chance adds, the end is a matching pair at or behind the last base of F
    for seed in range(20):
        rng = np.random.default_rng(200 + seed)
        t, q = E.store_codes(F + _rand(rng, 300)), E.store_codes(F + _rand(rng, 300))
        (s, i, j, last), = E.extend_sides([(t, q)], 400).tolist()
        assert i >= 60 and j >= 60 and s >= 120 and t[j - 1] == q[i - 1]
        assert i <= 60 + (s - 120) and j <= 60 + (s - 120)       # every base past F was paid for: two bases per point at the most


def test_zdrop_smaller_than_one_long_gap_stops_before_the_gap():
    F = _rand(np.random.default_rng(105), 140, b"ACG")          # no T: the 60 extra target bases match nothing
    t_right = F[:40] + b"T" * 60 + F[40:]
    ext, sc, _ = _record(t_right=t_right, q_right=F)            # the default zdrop of 400 takes the gap (4 + 2 * 60 = 124)
    assert ext == [0, 0, 200, 140] and sc == [0, 2 * 140 - 124]
    ext, sc, _ = _record(t_right=t_right, q_right=F, zdrop=30)
    assert ext == [0, 0, 40, 40] and sc == [0, 80]
    # the rule looks every 16 diagonals: the path through the gap is lowest, 80 - 124, on d = 140, and is back at -40 on d = 144,
    # where the mismatching main diagonal holds 80 - 2 * 64; the check of d = 128 saw that diagonal at -16
    ext, sc, _ = _record(t_right=t_right, q_right=F, zdrop=119)
    assert ext == [0, 0, 40, 40] and sc == [0, 80]
    ext, sc, _ = _record(t_right=t_right, q_right=F, zdrop=120)
    assert ext == [0, 0, 200, 140] and sc == [0, 2 * 140 - 124]


def test_max_ext_cuts_the_flank():
    F = _rand(np.random.default_rng(106), 80)
    assert _record(t_right=F, q_right=F, t_left=F, q_left=F)[:2] == ([80, 80, 80, 80], [160, 160])
    assert _record(t_right=F, q_right=F, t_left=F, q_left=F, max_ext=50)[:2] == ([50, 50, 50, 50], [100, 100])
    with pytest.raises(ValueError):
        E.params(max_ext=(1 << 20) + 1)
    assert E.params() == (400, 2048) and E.params(7, 1 << 20) == (7, 1 << 20)


def test_an_empty_flank_on_either_sequence():
    F = _rand(np.random.default_rng(107), 50)
    assert _record(t_right=F)[:2] == ([0, 0, 0, 0], [0, 0])
    assert _record(q_right=F)[:2] == ([0, 0, 0, 0], [0, 0])
    assert _record(t_left=F)[:2] == ([0, 0, 0, 0], [0, 0])
    assert _record(q_left=F, t_right=F, q_right=F)[:2] == ([0, 0, 50, 50], [0, 100])
    assert _record()[:2] == ([0, 0, 0, 0], [0, 0])


def _mutate(rng, seq: bytes, p: float) -> bytes:
    out = bytearray()
    for b in seq:
        x = rng.random()
        if x < p / 3:
            continue
        if x < 2 * p / 3:
            out.append(b"ACGT"[rng.integers(0, 4)])
        elif x < p:
            out.append(b"ACGT"[(b"ACGT".index(b) + 1 + rng.integers(0, 3)) % 4])
            continue
        out.append(b)
    return bytes(out)


def _seeded_batch(seed=110, n=24):
    """reads and strand-0 records with a common 100-base span and flanks of 0-400 bases at 0-8 % error that turn random"""
    rng = np.random.default_rng(seed)
    reads, rows = [], []
    for r in range(n):
        core = _rand(rng, 100)
        fl = [_rand(rng, int(rng.integers(0, 400))) for _ in range(2)]
        p = float(rng.uniform(0, 0.08))
        tl, tr = _rand(rng, int(rng.integers(0, 80))) + fl[0], fl[1] + _rand(rng, int(rng.integers(0, 80)))
        ql, qr = _rand(rng, int(rng.integers(0, 80))) + _mutate(rng, fl[0], p), _mutate(rng, fl[1], p) + _rand(rng, int(rng.integers(0, 80)))
        t, q = tl + core + tr, ql + core + qr
        rows.append([2 * r + 1, len(q), len(ql), len(ql) + 100, 0, 2 * r, len(t), len(tl), len(tl) + 100])
        reads += [t, q]
    return reads, np.array(rows, np.uint32)


def test_a_reverse_strand_record_equals_its_forward_twin():
    reads, rows = _seeded_batch()
    twin_reads = [r if i % 2 == 0 else _rc(r) for i, r in enumerate(reads)]
    twin = rows.copy()
    twin[:, 4] = 1
    twin[:, 2], twin[:, 3] = rows[:, 1] - rows[:, 3], rows[:, 1] - rows[:, 2]
    out0, ext0, sc0 = E.extend_records([E.store_codes(r) for r in reads], rows)
    out1, ext1, sc1 = E.extend_records([E.store_codes(r) for r in twin_reads], twin)
    assert np.array_equal(ext0, ext1) and np.array_equal(sc0, sc1) and (ext0 > 0).sum() > 60
    assert np.array_equal(out0[:, 7:9], out1[:, 7:9])
    assert np.array_equal(out1[:, 2], rows[:, 1] - out0[:, 3]) and np.array_equal(out1[:, 3], rows[:, 1] - out0[:, 2])


def test_the_result_cell_is_entered_by_a_match():
    reads, rows = _seeded_batch(seed=111, n=40)
    codes = [E.store_codes(r) for r in reads]
    out, ext, sc = E.extend_records(codes, rows)
    seen = 0
    for r in range(len(rows)):
        (tl, ql), (tr, qr) = E.side_seqs(codes, rows[r], 2048)
        for T, Q, j, i, s in ((tl, ql, ext[r, 0], ext[r, 1], sc[r, 0]), (tr, qr, ext[r, 2], ext[r, 3], sc[r, 1])):
            assert (s > 0) == (i > 0) == (j > 0)
            if s > 0:
                assert T[j - 1] == Q[i - 1], r
                seen += 1
    assert seen > 60


def test_the_band_changes_nothing_on_short_flanks():
    """flanks of at most 63 bases lie inside the first band whatever happens: the banded sweep equals the whole matrix"""
    rng = np.random.default_rng(112)
    sides = []
    for trial in range(40):
        f = _rand(rng, int(rng.integers(1, 64)))
        g = _mutate(rng, f, 0.15)[:63] or b"A"
        sides.append((E.store_codes(f), E.store_codes(g)))
    got = E.extend_sides(sides, 1 << 20)
    for (t, q), g in zip(sides, got.tolist()):
        assert tuple(g[:3]) == E.extend_unbanded(t, q)


# ---- the seeded sets of test_overlap_host.py -----------------------------------------------------------------------------------------
def window_count(ts, te, tlen, W):
    """windows the reference's windowing takes from a target span (windowing.rs:53-108): none from a span shorter than W, whole
    windows only, except within 0.1 W of the read's ends"""
    if te - ts < W:
        return 0
    thr = int(np.float32(0.1) * np.float32(W))
    first = 0 if ts < thr else (ts + W - 1) // W
    last = (te - 1) // W + 1 if te > tlen - thr else te // W
    return max(0, last - first)


WINDOWS = (256, 1024, 4096)
TRUE_COUNTS = [(768, 192, 48), (531, 130, 28), (576, 144, 36)]     # SETS[0], [1], [2]: seed 21, seed 23 (partial), seed 22 (3 % error)
# The unbanded prototype these figures were first taken with never passed the true span.  The reference does, on the query, by one base
# in one record each of seed 23 and seed 22: the generator's own CIGAR ends "...1D1M" there, and the flank base behind the query's true
# end happens to equal the target's last base, so taking both target bases as a (mis)match and a match scores more than the generator's
# deletion.  The target span, from which the windows are cut, is never passed.
QUERY_OVERSHOOT = [0, 1, 1]
EXTENDED_4096 = [43, 20, 21]                                       # (overlap, window) pairs at W = 4096 after the extension; anchor spans: 0
_SET = {}


def extended_set(case):
    """(truth rows, anchor rows, extended rows, ext) of the set's target-query records, in the truth's order"""
    if case not in _SET:
        kw, (k, w), _ = SETS[case]
        sb = synth.generate(**kw)
        codes = [R.store_codes(sb.read_seq(i)) for i in range(sb.n_reads)]
        rids, rows, off, sc = R.find_overlaps(codes, k=k, w=w, max_occ=64, min_score=100)
        by = {(int(r[5]), int(r[0])): x for x, r in enumerate(rows)}
        pick = [by[(int(a[5]), int(a[0]))] for a in sb.aln]          # every true pair is found (test_overlap_host.py)
        anchor = rows[pick]
        assert np.array_equal(anchor[:, 4], sb.aln[:, 4])
        out, ext, esc = E.extend_records(codes, anchor)
        _SET[case] = (sb.aln.astype(np.int64), anchor.astype(np.int64), out.astype(np.int64), ext)
    return _SET[case]


def counts(rows):
    return tuple(sum(window_count(int(r[7]), int(r[8]), int(r[6]), W) for r in rows) for W in WINDOWS)


@pytest.mark.parametrize("case", range(3))
def test_what_the_extension_recovers_on_a_synthetic_set(case):
    truth, anchor, out, ext = extended_set(case)
    # every extended span contains its anchor span
    assert (out[:, 7] <= anchor[:, 7]).all() and (out[:, 8] >= anchor[:, 8]).all()
    assert (out[:, 2] <= anchor[:, 2]).all() and (out[:, 3] >= anchor[:, 3]).all()
    # ... and none exceeds the generator's true span by more than 0 bases
    over = np.stack([truth[:, 7] - out[:, 7], out[:, 8] - truth[:, 8], truth[:, 2] - out[:, 2], out[:, 3] - truth[:, 3]], 1)
    short = np.stack([anchor[:, 7] - truth[:, 7], truth[:, 8] - anchor[:, 8]], 1)
    left = np.stack([out[:, 7] - truth[:, 7], truth[:, 8] - out[:, 8]], 1)
    c_true, c_anchor, c_ext = counts(truth), counts(anchor), counts(out)
    print(dict(case=case, records=len(truth), overshoot=int(over.max()), anchor_shortfall_median=float(np.median(short)),
               anchor_shortfall_max=int(short.max()), left_after_median=float(np.median(left)), left_after_max=int(left.max()),
               bases_added_mean=float(ext.sum(1).mean()), true=c_true, anchor=c_anchor, extended=c_ext))
    assert over[:, :2].max() <= 0             # the span the windows are cut from: the target's
    assert int(over[:, 2:].max()) == QUERY_OVERSHOOT[case] and int((over[:, 2:] > 0).sum()) == QUERY_OVERSHOOT[case]
    assert c_true == TRUE_COUNTS[case]
    assert c_ext[:2] == c_true[:2]             # all coverage at W = 256 / 1024 is back
    assert c_anchor[0] < c_true[0] and c_anchor[2] == 0
    assert c_ext[2] > 0                        # and the bench's own shape is no longer empty
    assert c_ext[2] == EXTENDED_4096[case]     # (the rest end a few bases short of a read end on an error and stay under W)


# ---- error codes -------------------------------------------------------------------------------------------------------------------------
def test_error_codes_without_a_device():
    c = api.HostContext([100, 200, 300])
    rows = np.array([[1, 200, 10, 60, 0, 0, 100, 20, 70]], np.uint32)
    with pytest.raises(api.HerroError) as e:
        c.extend_overlaps(rows)
    assert e.value.code == -2 and "herro_extend_overlaps" in str(e.value)      # HERRO_E_NO_DEVICE
    with pytest.raises(api.HerroError) as e:
        c.extend_overlaps(rows[:0])
    assert e.value.code == -2                                                  # n = 0 as herro_align_overlaps: the context is looked at first
    for bad in ((1 << 20) + 1, 0xFFFFFFFF):
        with pytest.raises(api.HerroError) as e:
            c.extend_overlaps(rows, max_ext=bad)
        assert e.value.code == -1 and "max_ext" in str(e.value), bad           # HERRO_E_INVALID, before anything else
    with pytest.raises(api.HerroError) as e:
        c.extend_overlaps(rows, max_ext=1 << 20)
    assert e.value.code == -2
    with pytest.raises(api.HerroError) as e:
        c.extend_overlaps(rows, zdrop=-1)
    assert e.value.code == -1
    # the C entry itself
    L = api.lib()
    arr = (api.Alignment * 1)()
    h = C.c_void_p()
    p = api.ExtendParams(zdrop=0, max_ext=(1 << 20) + 1)
    assert L.herro_extend_overlaps(c.h, 1, C.byref(arr), C.byref(p), C.byref(h)) == -1 and not h.value
    assert L.herro_extend_overlaps(c.h, 1, C.byref(arr), None, C.byref(h)) == -2            # NULL parameters: the defaults
    assert L.herro_extend_overlaps(None, 1, C.byref(arr), None, C.byref(h)) == -1
    assert L.herro_extend_overlaps(c.h, 1, None, None, C.byref(h)) == -1
    assert L.herro_extend_overlaps(c.h, 1, C.byref(arr), None, None) == -1
    assert L.herro_extended_n(None) == 0 and not L.herro_extended_alignments(None) and not L.herro_extended_ext(None)
    assert not L.herro_extended_scores(None)
    L.herro_extended_free(None)
