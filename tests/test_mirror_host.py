"""not-gpu: mirrored records (herro_aligned_dev_mirror) — the specification tests/mirror_ref.py on hand cases whose
CIGARs are written out, on a seeded set of pairs where the mirror is held against the swapped record aligned directly, the pairing
helpers of herro_amd.api, and the entry's error codes without a device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_ref as A  # noqa: E402
import mirror_cases as MC  # noqa: E402
import mirror_ref as MR  # noqa: E402
import overlap_ref as R  # noqa: E402
from herro_amd import api  # noqa: E402

INT32_MIN = -(1 << 31)


# ---- hand cases ---------------------------------------------------------------------------------------------------------------------------
def test_hand_cases_give_the_cigars_written_out():
    names, reads, rows, off, ops, want = MC.hand()
    codes = [A.store_codes(r) for r in reads]
    assert {"swap_strand0", "reverse_strand1", "homopolymer_strand1", "repeat3_strand1", "shift_eats_the_m", "ends_i_next_to_d",
            "failed_source", "single_m", "type_3"} <= set(names)
    n_ops = dict(zip(names, np.diff(off).astype(int).tolist()))
    assert n_ops["failed_source"] == 0 and n_ops["single_m"] == 1 and n_ops["two_ops_trailing"] == 2 and n_ops["three_ops_middle_moves"] == 3
    for i, name in enumerate(names):
        src = [(int(x) >> 2, int(x) & 3) for x in ops[int(off[i]):int(off[i + 1])]]
        row, cig, sc, ok = MR.mirror_record(codes, rows[i], src, 0)
        w_row, w_cig = want[i]
        assert row.tolist() == w_row.tolist(), name
        if w_cig is None:
            assert not ok and cig == [] and sc == INT32_MIN, name
            continue
        assert ok and A.cigar_text(cig) == w_cig, (name, A.cigar_text(cig))
        T, Q = A.record_seqs(codes, row)
        # a source score of 0: the field is g(source) - g(mirror), and the identity holds against the bases
        Ts, Qs = A.record_seqs(codes, rows[i])
        assert _consumes(src, Ts, Qs) and _consumes(cig, T, Q), name
        assert A.score_cigar(cig, T, Q) == A.score_cigar(src, Ts, Qs) + sc, name
    # the cases that must move something do, and only on the material that says so
    moved = {n for n, (s, tp, qp, o, text, _) in MC.HAND.items() if isinstance(o, str) and text is not None and o != text}
    assert {"homopolymer_strand1", "repeat3_strand1", "shift_eats_the_m", "three_ops_middle_moves"} <= moved
    assert "swap_strand0" not in moved and "reverse_strand1" not in moved


def _consumes(ops, T, Q):
    return sum(ln for ln, t in ops if t != A.I_) == len(T) and sum(ln for ln, t in ops if t != A.D_) == len(Q)


# ---- the seeded set: the mirror against the swapped record aligned directly -----------------------------------------------------------
def _mutate(rng, s, err):
    out, i = [], 0
    while i < len(s):
        r = rng.random()
        if r < err / 3:
            out.append(int(rng.integers(0, 4))); i += 1
        elif r < 2 * err / 3:
            out.append(int(rng.integers(0, 4)))
        elif r < err:
            i += 1
        else:
            out.append(int(s[i])); i += 1
    return np.array(out, np.uint8)


def _low_complexity(rng, n):
    parts = []
    while sum(len(p) for p in parts) < n:
        k = rng.integers(0, 3)
        if k == 0:
            parts.append(rng.integers(0, 4, rng.integers(5, 40)))
        elif k == 1:
            parts.append(np.full(rng.integers(3, 15), rng.integers(0, 4)))
        else:
            parts.append(np.tile(rng.integers(0, 4, rng.integers(2, 4)), rng.integers(2, 8)))
    return np.concatenate(parts)[:n].astype(np.uint8)


N_PAIRS = 240
# measured by this test (DESIGN.md §9 quotes them): strand-1 records whose mirrored ops fix_cigar changes; mirrors whose CIGAR text is
# byte-identical to the directly aligned swapped record's
SHIFT_CHANGED_STRAND1, SAME_TEXT = 76, 218


def seeded_pairs(seed=5):
    """240 pairs of 60-300 bases, every second one of homopolymers and 2-3-bp repeats, 1 / 3 / 8 % error, five clean bases at each end
    (nothing is trimmed), every second pair of pairs on strand 1: (codes, rows u32 [240, 9])"""
    rng = np.random.default_rng(seed)
    codes, rows = [], []
    for p in range(N_PAIRS):
        n = int(rng.integers(60, 300))
        t = _low_complexity(rng, n) if p % 2 else rng.integers(0, 4, n).astype(np.uint8)
        q = np.concatenate([t[:5], _mutate(rng, t[5:-5], (0.01, 0.03, 0.08)[p % 3]), t[-5:]]).astype(np.uint8)
        strand = (p // 2) % 2
        if strand:
            q = (3 - q[::-1]).astype(np.uint8)
        codes += [t, q]
        rows.append([2 * p + 1, len(q), 0, len(q), strand, 2 * p, len(t), 0, len(t)])
    return codes, np.array(rows, np.uint32)


def test_the_mirror_of_every_seeded_pair_is_an_optimal_alignment_of_the_swapped_record():
    codes, rows = seeded_pairs()
    assert (rows[:, 4] == 0).sum() == (rows[:, 4] == 1).sum() == N_PAIRS // 2
    out, cigs, scores, ok, _ = A.align_records(codes, rows, threads=4)
    d_out, d_cigs, d_scores, d_ok, _ = A.align_records(codes, rows[:, MR.SWAP], threads=4)
    assert ok.all() and d_ok.all()
    assert np.array_equal(out[:, :9], rows) and np.array_equal(d_out[:, :9], rows[:, MR.SWAP])       # clean ends: nothing trimmed
    changed = [0, 0]
    same_text = unbanded = 0
    for r in range(N_PAIRS):
        src = A.parse_cigar(cigs[r])
        strand = int(rows[r, 4])
        row, cig, sc, good = MR.mirror_record(codes, out[r], src, int(scores[r]))
        assert good and row.tolist() == rows[r, MR.SWAP].tolist(), r                                  # no mirror fails, none is trimmed
        T, Q = A.record_seqs(codes, row)
        before = MR.mirror_ops(src, strand)
        changed[strand] += cig != before
        if strand == 0:
            assert cig == before, r                                                                   # the shift moves nothing on strand 0
        again, tsh, qsh = A.fix_cigar(cig, T, Q)
        assert again == cig and tsh == 0 and qsh == 0, r                                              # a second pass changes nothing
        assert _consumes(cig, T, Q), r
        assert A.score_cigar(cig, T, Q) == sc, r                                                      # the score identity, on the bases
        assert sc == int(scores[r]) == int(d_scores[r]), (r, sc, int(scores[r]), int(d_scores[r]))
        same_text += A.cigar_text(cig) == d_cigs[r]
        if r < 60:
            unbanded += A.gotoh_unbanded(T, Q) == sc
    print(dict(strand1_changed=changed[1], same_text=same_text, unbanded_of_60=unbanded))
    assert changed[0] == 0 and unbanded == 60
    assert (changed[1], same_text) == (SHIFT_CHANGED_STRAND1, SAME_TEXT)


# ---- pairing ------------------------------------------------------------------------------------------------------------------------------
def _reads_for_the_finder():
    import lowcomplexity as LC
    ws = LC.working_set(seed=7, n_genomes=1, L=4000, n_reads=5, min_len=2000, max_len=3000)
    return ws, ws.codes()


def test_pair_rows_on_the_finders_output_pairs_every_row():
    ws, codes = _reads_for_the_finder()
    rids, rows, aln_off, _ = R.find_overlaps(codes, max_occ=64, min_score=100)
    assert len(rows) >= 8 and len(rows) % 2 == 0
    prim, rec = api.pair_rows(rows)
    n = len(rows)
    assert len(prim) == n // 2 and prim.dtype == np.int64 and rec.dtype == np.uint32 and len(rec) == n
    assert (np.diff(prim) > 0).all() and sorted(rec.tolist()) == list(range(n))
    assert (rows[prim, 5] < rows[prim, 0]).all()                       # targets ascend: the first row of a pair is the one with t < q
    for i in range(n):
        p = int(rec[i])
        if p < len(prim):
            assert prim[p] == i
        else:
            assert rows[i, :9].tolist() == rows[prim[p - len(prim)], :9][MR.SWAP].tolist()
    # every row kept: the job's grouping is the finder's, rec in row order
    ok = np.ones(2 * len(prim), bool)
    j_rids, off2, jrec = api.paired_job_args(rids, aln_off, rec, ok)
    assert j_rids.tolist() == rids.tolist() and off2.tolist() == aln_off.tolist() and jrec.tolist() == rec.tolist()
    assert off2.dtype == np.uint64 and jrec.dtype == np.uint32


def test_pair_rows_leaves_rows_without_an_exact_mate_alone():
    a = [3, 900, 10, 800, 1, 1, 950, 20, 830]
    b = [7, 500, 0, 400, 0, 2, 600, 100, 500]
    sw = lambda r: [r[k] for k in MR.SWAP]                             # noqa: E731
    near = sw(b)
    near[3] += 1                                                        # one coordinate off: no mate
    lone = [9, 100, 0, 90, 0, 4, 100, 5, 95]
    other_strand = sw(lone)
    other_strand[4] = 1
    rows = np.array([a, b, lone, sw(a), near, other_strand, a, sw(a)], np.uint32)
    prim, rec = api.pair_rows(rows)
    #                 a  b  lone  a' near other  a(again)  a'(again)
    assert prim.tolist() == [0, 1, 2, 4, 5, 6]
    assert rec.tolist() == [0, 1, 2, 6 + 0, 3, 4, 5, 6 + 5]
    prim, rec = api.pair_rows(np.zeros((0, 9), np.uint32))
    assert len(prim) == 0 and len(rec) == 0
    # a row that is its own swap is not its own mate
    self_row = np.array([[2, 50, 0, 40, 0, 2, 50, 0, 40]], np.uint32)
    prim, rec = api.pair_rows(self_row)
    assert prim.tolist() == [0] and rec.tolist() == [0]
    prim, rec = api.pair_rows(np.concatenate([self_row, self_row]))
    assert prim.tolist() == [0] and rec.tolist() == [0, 1]


def _pair_rows_in_order(rows):
    """the rule as a loop: every row takes the oldest unpaired earlier row that is its exact swap, or waits as a primary"""
    waiting, prim, rec, mated = {}, [], [0] * len(rows), []
    for i, row in enumerate(rows.tolist()):
        w = waiting.get(tuple(row))
        if w:
            mated.append((i, w.pop(0)))
            continue
        rec[i] = len(prim)
        waiting.setdefault(tuple(row[k] for k in MR.SWAP), []).append(len(prim))
        prim.append(i)
    for i, p in mated:
        rec[i] = len(prim) + p
    return prim, rec


def test_pair_rows_equals_the_rule_taken_row_by_row():
    rng = np.random.default_rng(3)
    for trial in range(300):
        n = int(rng.integers(1, 40))
        rows = rng.integers(0, 2, (n, 9)).astype(np.uint32)              # few distinct rows: duplicates, rows equal to their own swap
        if trial % 2:
            rows[:, :4] = rows[:, 5:9] * rng.integers(0, 2, (n, 1))
        want = _pair_rows_in_order(rows)
        for exact in (False, True):
            prim, rec = api.pair_rows(rows, exact_ids=exact)
            assert (prim.tolist(), rec.tolist()) == want, (trial, exact, rows.tolist())


def test_paired_job_args_drops_failed_records_and_keeps_the_targets():
    rids = np.array([7, 3, 9, 4], np.uint32)
    aln_off = np.array([0, 3, 5, 5, 8], np.uint64)
    # eight rows over five primaries: rows 0 .. 4 are primaries 0 .. 4, rows 5, 6, 7 the mates of primaries 0, 1, 3
    rec_of_row = np.array([0, 1, 2, 3, 4, 5 + 0, 5 + 1, 5 + 3], np.uint32)
    ok = np.ones(10, bool)
    ok[1] = False            # a failed primary: row 1 goes, its mirror (row 6) is judged on its own
    ok[5 + 0] = False        # a failed mirror: row 5 goes, its primary (row 0) stays
    ok[3] = ok[4] = False    # target 3 (rows 3, 4) loses all its rows
    r, off, rec = api.paired_job_args(rids, aln_off, rec_of_row, ok)
    assert r.tolist() == [7, 3, 9, 4] and off.tolist() == [0, 2, 2, 2, 4] and rec.tolist() == [0, 2, 5 + 1, 5 + 3]
    assert off.dtype == np.uint64 and rec.dtype == np.uint32
    r, off, rec = api.paired_job_args(np.zeros(0, np.uint32), np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, bool))
    assert len(r) == 0 and off.tolist() == [0] and len(rec) == 0


# ---- error codes without a device ---------------------------------------------------------------------------------------------------------
def test_mirror_needs_a_device_and_its_arguments():
    names, reads, rows, off, ops, _ = MC.hand()
    c = api.HostContext(np.array([len(r) for r in reads], np.uint32))
    h = c.aligned_dev_from_ops(rows, off, ops)
    with pytest.raises(api.HerroError) as e:
        h.mirror()
    assert e.value.code == -2 and "no device" in str(e.value)           # HERRO_E_NO_DEVICE
    L = c._l
    out = C.c_void_p()
    assert L.herro_aligned_dev_mirror(None, h.h, C.byref(out)) == -1     # HERRO_E_INVALID
    assert L.herro_aligned_dev_mirror(c.h, None, C.byref(out)) == -1
    assert L.herro_aligned_dev_mirror(c.h, h.h, None) == -1
    other = api.HostContext(np.array([len(r) for r in reads], np.uint32))
    assert L.herro_aligned_dev_mirror(other.h, h.h, C.byref(out)) == -1 and "another context" in other.last_error()
    assert not out.value
    h.close()
