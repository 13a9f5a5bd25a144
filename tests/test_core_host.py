"""not-gpu: a core set of targets without a device — the counts the read sets of tests/pair_cases.py have under the masks of
tests/core_cases.py (numpy reference), the filter's fixed points, the `_core` entries and herro_pairs_from_table_core /
herro_pairs_n_rows / herro_job_create_paired on a device-free context, and shard.core_masks."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aligned_dev_cases as AC  # noqa: E402
import align_ref as A  # noqa: E402
import core_cases as CC  # noqa: E402
import mirror_ref as MR  # noqa: E402
import pair_cases as PC  # noqa: E402
from herro_amd import api, shard  # noqa: E402

_CACHE = {}


# ---- the counts, from overlap_ref -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,pn", sorted(CC.EXPECTED))
def test_counts_under_the_masks(name, pn):
    (anchors, pairs), table = CC.EXPECTED[(name, pn)]
    kw = CC.PARAMS[pn]
    codes, a, f = CC.reference(name, kw)
    M = CC.masks(len(codes))
    assert (len(a), len(f["primaries"])) == (anchors, pairs)
    assert CC.counts(name, kw, M["all"]) == (anchors, pairs, 2 * pairs) and CC.counts(name, kw, M["none"]) == (0, 0, 0)
    for mask, want in table.items():
        assert CC.counts(name, kw, M[mask]) == want, (name, pn, mask)
        assert CC.counts(name, kw, CC.odd_bytes(M[mask])) == want


def test_counts_of_sets_c_and_e():
    codes, a, f = CC.reference("C", PC.DEFAULTS)
    assert len(codes) == 2 and len(a) == CC.C_ANCHORS and len(f["primaries"]) == 1
    for m in ([1, 0], [0, 1]):                                              # any one-read mask: every anchor, the pair, one row
        assert CC.counts("C", PC.DEFAULTS, np.array(m, np.uint8)) == (CC.C_ANCHORS, 1, 1)
    codes, a, f = CC.reference("E", PC.DEFAULTS)
    for m in CC.masks(len(codes)).values():
        assert CC.counts("E", PC.DEFAULTS, m)[1:] == (0, 0)


@pytest.mark.parametrize("name,pn", sorted(CC.EXPECTED))
def test_the_filter_keeps_all_and_drops_none(name, pn):
    codes, _, f = CC.reference(name, CC.PARAMS[pn])
    M = CC.masks(len(codes))
    PC.assert_same_fields(CC.filter_pairs(f, M["all"]), f, "all")
    empty = CC.filter_pairs(f, M["none"])
    for k in PC.FIELDS:
        assert empty[k].dtype == f[k].dtype and empty[k].shape[1:] == f[k].shape[1:], k
        assert (empty[k].tolist() == [0]) if k == "aln_off" else (len(empty[k]) == 0), k
    rids, rows, aln_off, scores = _rows_of(f)
    got = CC.filter_rows(rids, rows, aln_off, scores, M["all"])
    for g, w in zip(got, (rids, rows, aln_off, scores)):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    assert [len(x) for x in CC.filter_rows(rids, rows, aln_off, scores, M["none"])] == [0, 0, 1, 0]


def _rows_of(f):
    """the finder's 2 P rows of a fields dict: row i is primary rec_of_row[i] or the swap of primary rec_of_row[i] - P"""
    pr, rec, P = f["primaries"], f["rec_of_row"].astype(np.int64), len(f["primaries"])
    both = np.concatenate([pr, pr[:, [5, 6, 7, 8, 4, 0, 1, 2, 3, 9]]])
    return f["rids"], both[rec], f["aln_off"], np.concatenate([f["chain_scores"]] * 2)[rec]


def test_filter_rows_is_the_row_half_of_filter_pairs():
    codes, _, f = CC.reference("B", PC.DEFAULTS)
    rids, rows, aln_off, scores = _rows_of(f)
    for name, m in CC.masks(len(codes)).items():
        g = CC.filter_pairs(f, m)
        r2 = CC.filter_rows(rids, rows, aln_off, scores, m)
        w = _rows_of(g)
        for x, y in zip(r2, w):
            assert x.dtype == y.dtype and np.array_equal(x, y), name


# ---- the entries on a device-free context ---------------------------------------------------------------------------------------------------
def _d():
    """set D at the defaults on the CPU: the full table, its primaries aligned and mirrored (2 P records: rows, CIGARs)"""
    if "d" not in _CACHE:
        codes, _, f = CC.reference("D", PC.DEFAULTS)
        out, cigs, sc, ok, _ = A.align_records(codes, f["primaries"], threads=4)
        assert ok.all()
        m_rows, m_cigs, _, m_ok = MR.mirror_records(codes, out, cigs, sc)
        assert m_ok.all()
        _CACHE["d"] = dict(lens=np.array([len(x) for x in codes], np.uint32), f=f, rows2=np.concatenate([out, m_rows]), cigs2=list(cigs) + list(m_cigs))
    return _CACHE["d"]


def _raises(code, text, fn, *args, **kw):
    with pytest.raises(api.HerroError) as e:
        fn(*args, **kw)
    assert e.value.code == code and text in str(e.value), str(e.value)


def test_the_core_finders_check_parameters_first_and_need_a_device():
    s = _d()
    c = api.HostContext(s["lens"])
    mask = CC.masks(len(s["lens"]))["first_half"]
    h = C.c_void_p()
    k32 = api.OverlapParams(k=32)
    far = api.ExtendParams(max_ext=(1 << 20) + 1)
    for core in (None, mask.ctypes.data):
        assert c._l.herro_find_overlaps_core(c.h, C.byref(k32), core, C.byref(h)) == -1 and "5 <= k <= 31" in c.last_error()
        assert c._l.herro_find_overlaps_core(c.h, None, core, C.byref(h)) == -2 and "herro_find_overlaps: the context has no device" in c.last_error()
        assert c._l.herro_find_overlap_pairs_core(c.h, C.byref(k32), None, 0, core, C.byref(h)) == -1 and "5 <= k <= 31" in c.last_error()
        assert c._l.herro_find_overlap_pairs_core(c.h, None, C.byref(far), 0, core, C.byref(h)) == -1 and "max_ext must be at most 2^20" in c.last_error()
        assert c._l.herro_find_overlap_pairs_core(c.h, None, None, 2, core, C.byref(h)) == -1 and "unknown flag" in c.last_error()
        assert c._l.herro_find_overlap_pairs_core(c.h, None, None, 0, core, C.byref(h)) == -2
        assert "herro_find_overlap_pairs: the context has no device" in c.last_error() and not h.value
    _raises(-2, "herro_find_overlap_pairs: the context has no device", c.find_overlap_pairs, core=mask)
    _raises(-2, "herro_find_overlaps: the context has no device", c.find_overlaps, core=mask)
    with pytest.raises(ValueError):                                           # a mask of another length never reaches the library
        c.find_overlap_pairs(core=mask[:-1])
    with pytest.raises(ValueError):
        c.find_overlaps(core=np.ones(len(mask) + 1, np.uint8))


def test_pairs_from_table_core_takes_a_filtered_table_and_names_each_fault():
    s = _d()
    f = s["f"]
    c = api.HostContext(s["lens"])
    M = CC.masks(len(s["lens"]))
    full = c.pairs_from_table(f["primaries"], f["chain_scores"], f["rids"], f["aln_off"], f["rec_of_row"])
    assert full.n_rows == 2 * full.n_pairs == 8
    for name in ("first_half", "every3rd", "all", "none"):
        g = CC.filter_pairs(f, M[name])
        p = c.pairs_from_table(g["primaries"], g["chain_scores"], g["rids"], g["aln_off"], g["rec_of_row"], n_rows=len(g["rec_of_row"]))
        assert p.n_rows == len(g["rec_of_row"]) and p.n_pairs == len(g["primaries"]) and c._l.herro_pairs_n_rows(p.h) == p.n_rows
        PC.assert_same_fields(PC.pairs_fields(p), g, name)
        p.close()
    g = CC.filter_pairs(f, M["first_half"])
    assert (len(g["primaries"]), len(g["rec_of_row"])) == (3, 5)
    pr, sc, rids, off, rec = g["primaries"], g["chain_scores"], g["rids"], g["aln_off"], g["rec_of_row"]
    who = "herro_pairs_from_table_core: "
    for t, v in ((0, 1), (2, 0), (2, 6), (len(off) - 1, 4)):                  # aln_off ascends from 0 to n_rows
        x = off.copy()
        x[t] = v
        _raises(-1, who + f"aln_off[{t}] = {v}: aln_off must ascend from 0 to 5", c.pairs_from_table, pr, sc, rids, x, rec, n_rows=5)
    x = rec.copy()
    x[3] = 6
    _raises(-1, who + "rec_of_row[3] = 6 is outside the 6 records", c.pairs_from_table, pr, sc, rids, off, x, n_rows=5)
    x = rec.copy()
    x[4] = x[1]
    _raises(-1, who + f"rec_of_row[4] = {x[1]} occurs twice", c.pairs_from_table, pr, sc, rids, off, x, n_rows=5)
    # the strict entry refuses the same table: it wants two rows per pair
    _raises(-1, "herro_pairs_from_table: aln_off[", c.pairs_from_table, pr, sc, rids, off, np.concatenate([rec, [5]]).astype(np.uint32))
    assert c._l.herro_pairs_n_rows(None) == 0
    full.close()


@pytest.mark.parametrize("mask", ["first_half", "every3rd"])
def test_create_job_paired_on_a_masked_table_equals_job_create_over_the_same_rows(mask):
    """the aligned handle holds 2 P' records (primaries, then mirrors), the table R' <= 2 P' rows: the job is herro_job_create's over those rows
    as CIGAR text"""
    s = _d()
    f = s["f"]
    P = len(f["primaries"])
    m = CC.masks(len(s["lens"]))[mask]
    g = CC.filter_pairs(f, m)
    c_keep = np.asarray(m)[f["primaries"][:, 5]] | np.asarray(m)[f["primaries"][:, 0]]
    kept = np.flatnonzero(c_keep)
    Pn, Rn = len(kept), len(g["rec_of_row"])
    assert 0 < Rn < 2 * Pn
    sel = np.concatenate([kept, P + kept])                                     # the records of the masked handle in the full one
    rows2, cigs2 = s["rows2"][sel], [s["cigs2"][i] for i in sel]
    c = api.HostContext(s["lens"])
    h = c.aligned_dev_from_ops(rows2, *AC.cigars_to_ops(cigs2))
    assert h.n == 2 * Pn
    p = c.pairs_from_table(g["primaries"], g["chain_scores"], g["rids"], g["aln_off"], g["rec_of_row"], n_rows=Rn)
    rec = g["rec_of_row"].astype(np.int64)
    for W in (256, 1024):
        jp = c.create_job_paired(p, h, W)
        jc = c.create_job(g["rids"], rows2[rec], g["aln_off"], [cigs2[i] for i in rec], W)
        a, b = c.job_arrays(jp), c.job_arrays(jc)
        assert jp.n_targets == jc.n_targets == len(g["rids"]) and jp.n_windows == jc.n_windows > 0 and jp.skipped() == jc.skipped()
        assert set(a) == set(b)
        for k in a:
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (mask, W, k)
        jp.close()
        jc.close()
    # a handle of R' records (one per row) is not what the pairs need
    short = c.aligned_dev_from_ops(rows2[rec], *AC.cigars_to_ops([cigs2[i] for i in rec]))
    _raises(-1, f"herro_job_create_paired: the aligned handle has {Rn} records, the pairs need {2 * Pn}", c.create_job_paired, p, short, 256)
    assert c._l.herro_job_create_status(c.h) == -1
    for x in (p, h, short):
        x.close()


# ---- shard.core_masks -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", [[3000] * 12, [3000, 2460, 3000, 2460, 2500, 1900, 2500, 1900, 30, 2000], [5000, 100, 100, 100, 4000, 7]])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_core_masks_partition_the_reads_as_partition_targets_does(lens, world):
    W = 256
    lens = np.array(lens, np.uint32)
    masks = shard.core_masks(lens, W, world)
    again = shard.core_masks(lens, W, world)
    assert len(masks) == world and all(m.dtype == np.uint8 and m.shape == (len(lens),) for m in masks)
    assert all(np.array_equal(a, b) for a, b in zip(masks, again))             # deterministic
    assert np.array_equal(np.sum(masks, axis=0), np.ones(len(lens)))           # every read in exactly one mask
    nw = shard.windows_of(lens, W)
    parts = shard.partition_targets(nw, world)
    assert [np.flatnonzero(m).tolist() for m in masks] == [p.tolist() for p in parts]
    assert [int(nw[m != 0].sum()) for m in masks] == [int(nw[p].sum()) for p in parts]   # the partition's balance
    if world == 1:
        assert masks[0].all()
