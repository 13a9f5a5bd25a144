"""not-gpu: pair overlaps without a device — the premises of read set D (tests/pair_cases.py), herro_pairs_from_table and
herro_job_create_paired on a device-free context against paired_job_args + create_job_aligned, every validation message of
herro_pairs_from_table, and the codes of the entries that need a device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_ref as A  # noqa: E402
import aligned_dev_cases as AC  # noqa: E402
import lowcomplexity as LC  # noqa: E402
import mirror_ref as MR  # noqa: E402
import overlap_ref as R  # noqa: E402
import pair_cases as PC  # noqa: E402
from herro_amd import api  # noqa: E402

_CACHE = {}


def _d():
    """set D, its codes and the stepwise chain on the CPU at the defaults: the finder's rows, their pairing, the primaries aligned and
    mirrored (2 P records: rows, CIGARs)"""
    if "d" not in _CACHE:
        d = PC.set_d()
        codes = d.codes()
        rids, rows, aln_off, scores = R.find_overlaps(codes, **PC.DEFAULTS)
        prim, rec_of_row = api.pair_rows(rows, exact_ids=True)
        out, cigs, sc, ok, _ = A.align_records(codes, rows[prim], threads=4)
        assert ok.all()
        m_rows, m_cigs, _, m_ok = MR.mirror_records(codes, out, cigs, sc)
        assert m_ok.all()
        _CACHE["d"] = dict(reads=d, codes=codes, rids=rids, rows=rows, aln_off=aln_off, scores=scores, prim=prim, rec_of_row=rec_of_row,
                           rows2=np.concatenate([out, m_rows]), cigs2=list(cigs) + list(m_cigs))
    return _CACHE["d"]


# ---- the premises of set D ----------------------------------------------------------------------------------------------------------------
def test_set_d_chains_on_both_strands_with_unequal_scores():
    s = _d()
    codes = s["codes"]
    assert [len(r) for r in s["reads"].reads] == [3000, 2460, 3000, 2460, 2500, 1900, 2500, 1900, 30, 2000]
    ch = LC.chains(codes, **PC.DEFAULTS)
    assert {c[:3]: c[3] for c in ch} == PC.D_CHAINS_DEFAULTS and [c[:3] for c in ch] == sorted(PC.D_CHAINS_DEFAULTS)
    picked = R.pick_strands(ch)
    assert len(picked) == 4
    rids, rows = s["rids"], s["rows"]
    assert rids.tolist() == list(range(8))                                    # reads 8 and 9 get no record
    assert rows[s["prim"]][:, [5, 0, 4]].tolist() == [[0, 1, 0], [2, 3, 1], [4, 5, 0], [6, 7, 1]]
    assert s["scores"][s["prim"]].tolist() == [1477, 1487, 1890, 1889]
    ch = LC.chains(codes, **PC.SMALL_K)
    both = {c[:3]: c[3] for c in ch if c[0] in (0, 2)}
    assert both == PC.D_BOTH_SMALL_K
    assert LC.pairs_chained_on_both_strands(codes, **PC.SMALL_K) == 2
    ch = LC.chains(codes, **PC.HIGH_SCORE)                                     # the weaker strand is not kept
    assert [c[:3] for c in ch] == [(0, 1, 0), (2, 3, 1), (4, 5, 0), (6, 7, 1)]
    assert LC.chains(PC.set_e().codes(), **PC.DEFAULTS) == []
    c = PC.set_c().codes()
    ch = LC.chains(c, **PC.DEFAULTS)
    assert [x[:3] for x in ch] == [(0, 1, 0), (0, 1, 1)] and ch[0][3] == ch[1][3]          # set C: an exact tie


def test_the_primaries_are_the_first_row_of_every_pair_in_ascending_order():
    """what the device relies on: the finder's rows sort by (tid, qid), so the row (t, q) with t < q is its pair's primary and the
    primaries ascend in (t, q); rec_of_row follows from the row order alone"""
    s = _d()
    rows, prim, rec = s["rows"], s["prim"], s["rec_of_row"]
    pr = rows[prim]
    assert (pr[:, 5] < pr[:, 0]).all()
    key = pr[:, 5].astype(np.uint64) << np.uint64(32) | pr[:, 0]
    assert (np.diff(key.astype(np.int64)) > 0).all()
    n = len(prim)
    keys = np.concatenate([key, pr[:, 0].astype(np.uint64) << np.uint64(32) | pr[:, 5]])
    assert np.array_equal(np.argsort(keys).astype(np.uint32), rec)


# ---- herro_pairs_from_table and herro_job_create_paired on a device-free context ---------------------------------------------------
def _host_handle(c, s, empty=()):
    off, ops = AC.cigars_to_ops([b"" if r in empty else x for r, x in enumerate(s["cigs2"])])
    return c.aligned_dev_from_ops(s["rows2"], off, ops)


@pytest.mark.parametrize("empty", [(), (1, 6), (0, 4, 2, 6)])
def test_create_job_paired_equals_paired_job_args_on_a_host_context(empty):
    """(1, 6): primary 1 and the mirror of primary 2 failed; (0, 4, 2, 6): both records of pairs 0 and 2 — targets 0, 1, 4 and 5 lose
    their only row and keep their place"""
    s = _d()
    n = len(s["prim"])
    assert n == 4
    c = api.HostContext(s["reads"].lens)
    m = _host_handle(c, s, empty)
    assert m.n == 2 * n and m.failed == len(empty)
    p = c.pairs_from_table(s["rows"][s["prim"]], s["scores"][s["prim"]], s["rids"], s["aln_off"], s["rec_of_row"])
    assert p.n_pairs == n
    want = dict(primaries=s["rows"][s["prim"]], chain_scores=s["scores"][s["prim"]], ext=np.zeros((n, 4), np.uint32),
                ext_scores=np.zeros((n, 2), np.int32), rids=s["rids"], aln_off=s["aln_off"], rec_of_row=s["rec_of_row"])
    PC.assert_same_fields(PC.pairs_fields(p), want, empty)
    j_rids, off2, rec = api.paired_job_args(s["rids"], s["aln_off"], s["rec_of_row"], m.ok)
    assert len(rec) == 2 * n - len(empty) and len(j_rids) == 8
    if len(empty) == 4:
        assert np.diff(off2.astype(np.int64)).tolist() == [0, 0, 1, 1, 0, 0, 1, 1]
    for W in (256, 1024):
        jp = c.create_job_paired(p, m, W)
        ja = c.create_job_aligned(j_rids, off2, rec, m, W)
        a, b = c.job_arrays(jp), c.job_arrays(ja)
        assert jp.n_windows == ja.n_windows > 0 and jp.skipped() == ja.skipped()
        for k in a:
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (empty, W, k)
        jp.close()
        ja.close()
    p.close()
    m.close()


def test_an_empty_table_gives_an_empty_handle():
    c = api.HostContext([30, 2000, 2000])
    p = c.pairs_from_table(np.zeros((0, 10), np.uint32), None, np.zeros(0, np.uint32), np.zeros(1, np.uint64), np.zeros(0, np.uint32))
    assert p.n_pairs == 0 and p.aln_off.tolist() == [0] and len(p.rids) == 0 and len(p.rec_of_row) == 0
    assert p.primaries.shape == (0, 10) and p.ext.shape == (0, 4) and p.ext_scores.shape == (0, 2)
    p.close()


# ---- validation ---------------------------------------------------------------------------------------------------------------------------
def _raises(code, text, fn, *args):
    with pytest.raises(api.HerroError) as e:
        fn(*args)
    assert e.value.code == code and text in str(e.value), str(e.value)


def test_every_validation_message_of_pairs_from_table():
    s = _d()
    c = api.HostContext(s["reads"].lens)
    pr, sc, rids, off, rec = s["rows"][s["prim"]], s["scores"][s["prim"]], s["rids"], s["aln_off"], s["rec_of_row"]
    who = "herro_pairs_from_table: "

    def bad_row(r, col, v):
        x = pr.copy()
        x[r, col] = v
        return x
    # the primaries: the record checks of herro_align_overlaps, naming the record
    _raises(-1, who + "record 2: read id outside the read store", c.pairs_from_table, bad_row(2, 0, 10), sc, rids, off, rec)
    _raises(-1, who + "record 1: read id outside the read store", c.pairs_from_table, bad_row(1, 5, 77), sc, rids, off, rec)
    _raises(-1, who + "record 3: query coordinates outside the read", c.pairs_from_table, bad_row(3, 3, 1901), sc, rids, off, rec)
    _raises(-1, who + "record 0: query coordinates outside the read", c.pairs_from_table, bad_row(0, 2, 2461), sc, rids, off, rec)
    _raises(-1, who + "record 0: target coordinates outside the read", c.pairs_from_table, bad_row(0, 8, 3001), sc, rids, off, rec)
    _raises(-1, who + "record 1: strand must be 0 or 1", c.pairs_from_table, bad_row(1, 4, 2), sc, rids, off, rec)
    # aln_off ascends from 0 to 2 P
    for t, v in ((0, 1), (3, 1), (3, 9), (8, 7)):
        x = off.copy()
        x[t] = v
        _raises(-1, who + f"aln_off[{t}] = {v}: aln_off must ascend from 0 to 8", c.pairs_from_table, pr, sc, rids, x, rec)
    # rec_of_row holds every value of 0 .. 2 P - 1 once
    x = rec.copy()
    x[5] = 8
    _raises(-1, who + "rec_of_row[5] = 8 is outside the 8 records", c.pairs_from_table, pr, sc, rids, off, x)
    x = rec.copy()
    x[6] = x[2]
    _raises(-1, who + f"rec_of_row[6] = {x[2]} occurs twice", c.pairs_from_table, pr, sc, rids, off, x)
    big = api.HostContext([1 << 25, 1 << 25])
    _raises(-1, who + "record 0: overlap longer than 2^25 bases in all", big.pairs_from_table,
            np.array([[1, 1 << 25, 0, 1 << 25, 0, 0, 1 << 25, 0, 1 << 25]], np.uint32), None, [0, 1], [0, 1, 2], [0, 1])
    with pytest.raises(ValueError):
        c.pairs_from_table(pr, sc, rids, off[:-1], rec)


def test_create_job_paired_refuses_foreign_handles_and_wrong_counts():
    s = _d()
    c, other = api.HostContext(s["reads"].lens), api.HostContext(s["reads"].lens)
    pr, sc = s["rows"][s["prim"]], s["scores"][s["prim"]]
    p = c.pairs_from_table(pr, sc, s["rids"], s["aln_off"], s["rec_of_row"])
    m = _host_handle(c, s)
    m_other = _host_handle(other, s)
    p_other = other.pairs_from_table(pr, sc, s["rids"], s["aln_off"], s["rec_of_row"])
    off, ops = AC.cigars_to_ops(s["cigs2"][:4])
    m_short = c.aligned_dev_from_ops(s["rows2"][:4], off, ops)                # the primaries without their mirrors
    _raises(-1, "herro_job_create_paired: the handle belongs to another context", c.create_job_paired, p, m_other, 256)
    assert c._l.herro_job_create_status(c.h) == -1
    _raises(-1, "herro_job_create_paired: the handle belongs to another context", c.create_job_paired, p_other, m, 256)
    _raises(-1, "herro_job_create_paired: the aligned handle has 4 records, the pairs need 8", c.create_job_paired, p, m_short, 256)
    c.create_job_paired(p, m, 256).close()
    assert c._l.herro_job_create_status(c.h) == 0


def test_the_find_and_align_entries_need_a_device():
    s = _d()
    c = api.HostContext(s["reads"].lens)
    _raises(-2, "herro_find_overlap_pairs: the context has no device", c.find_overlap_pairs)
    _raises(-2, "herro_find_overlap_pairs: the context has no device", c.find_overlap_pairs, False)
    # parameters are checked first, in C as well (the binding refuses k = 32 itself)
    h = C.c_void_p()
    k32 = api.OverlapParams(k=32)
    assert c._l.herro_find_overlap_pairs(c.h, C.byref(k32), None, 0, C.byref(h)) == -1 and "5 <= k <= 31" in c.last_error()
    far = api.ExtendParams(max_ext=(1 << 20) + 1)
    assert c._l.herro_find_overlap_pairs(c.h, None, C.byref(far), 0, C.byref(h)) == -1 and "max_ext must be at most 2^20" in c.last_error()
    assert c._l.herro_find_overlap_pairs(c.h, None, None, 2, C.byref(h)) == -1 and "unknown flag" in c.last_error()
    assert not h.value
    p = c.pairs_from_table(s["rows"][s["prim"]], None, s["rids"], s["aln_off"], s["rec_of_row"])
    assert p.chain_scores.tolist() == [0, 0, 0, 0]
    _raises(-2, "the context has no device", p.align)
    other = api.HostContext(s["reads"].lens)
    assert other._l.herro_pairs_align(other.h, p.h, C.byref(h)) == -1 and "belongs to another context" in other.last_error()
