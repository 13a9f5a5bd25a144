"""gpu: the store cut on the device (herro_store_cut; DESIGN.md §13, "The cut on the device") through the C ABI.  All six arrays of the new
store (herro_debug_store_copy) against tests/cut_ref.py on every set of tests/cut_cases.py, and against a second context's store built by
the host path (io.cut_reads + set_reads) where all bytes are ACGT; the context's state afterwards, a second cut, contexts that share the old
store, jobs of the old store, a refused table, name classes given to the cut; and end to end: api.trim_reads(on_device=True) against the host path — ids, offsets, stats,
the finder's pairs field for field, one paired job's windows byte for byte."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import adapter_cases as AC  # noqa: E402
import cut_cases as CC  # noqa: E402
import cut_ref as CR  # noqa: E402
import gpu_common as G  # noqa: E402
import pair_cases as PC  # noqa: E402
from herro_amd import api, io  # noqa: E402

pytestmark = pytest.mark.gpu
_OTHER = {}


def _other():
    """a second context (no model): the host path's store, and the holder of a shared store"""
    if "c" not in _OTHER:
        _OTHER["c"] = api.Context(0)
    return _OTHER["c"]


def _reads_of(name):
    seq, qual, off = CC.arrays(name)
    n = len(off) - 1
    return io.Reads([b"r%d" % i for i in range(n)], [None] * n, seq, qual, off)


def _lengths(c):
    return np.diff(c.store_arrays()["qual_off"].astype(np.int64)).tolist()


# ---- 1. every set: the six arrays ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,table", CC.ALL_TABLES, ids=CC.IDS)
def test_the_cut_store_equals_the_reference_and_the_host_path(name, table):
    c = G.ctx()
    s = CC.get(name)
    tab = s["tables"][table][1]
    old, want = CC.reference(name, table)
    c.set_reads(*CC.arrays(name))
    CR.assert_same(c.store_arrays(), old, (name, "the store before the cut"))
    c.cut_store(tab)
    got = c.store_arrays()
    CR.assert_same(got, want, (name, table))
    assert c.n_reads == len(tab)
    if s["acgt"]:
        o = _other()
        cut = io.cut_reads(_reads_of(name), tab)
        o.set_reads(cut.seq, cut.qual, cut.off)
        CR.assert_same(got, o.store_arrays(), (name, table, "host path"))
        assert c.n_reads == o.n_reads and _lengths(c) == _lengths(o)


def test_packed_codes_are_the_exact_equivalent_on_reads_that_are_not_acgt():
    """herro_set_reads_packed of the reference's words: the store the cut builds, whatever the bytes were"""
    c, o = G.ctx(), _other()
    _, want = CC.reference("nonacgt", 0)
    c.set_reads(*CC.arrays("nonacgt"))
    c.cut_store(CC.get("nonacgt")["tables"][0][1])
    o._chk(o._l.herro_set_reads_packed(o.h, len(want["word_off"]) - 1, want["words"].ctypes.data, want["word_off"].ctypes.data,
                                       want["qual"].ctypes.data, want["qual_off"].ctypes.data, None))
    CR.assert_same(c.store_arrays(), o.store_arrays(), "packed")


# ---- 2. state ---------------------------------------------------------------------------------------------------------------------------------
def test_a_second_cut_on_the_cut_store():
    c = G.ctx()
    old, first = CC.reference("grid", 0)
    c.set_reads(*CC.arrays("grid"))
    c.cut_store(CC.get("grid")["tables"][0][1])
    lens = np.diff(first["qual_off"].astype(np.int64))
    rows = [(x, int(l) // 3, int(l) - int(l) // 4) for x, l in enumerate(lens) if x % 3 != 1][::-1]   # a third dropped, the rest trimmed, backwards
    tab = CC.pieces(rows)
    c.cut_store(tab)
    CR.assert_same(c.store_arrays(), CR.cut(first, tab), "second cut")
    assert c.n_reads == len(rows)


def test_a_sharing_context_keeps_the_old_store_until_it_shares_again():
    c, o = G.ctx(), _other()
    tab = CC.get("shapes")["tables"][0][1]
    old, want = CC.reference("shapes", 0)
    c.set_reads(*CC.arrays("shapes"))
    o.share_reads(c)
    c.cut_store(tab)
    CR.assert_same(o.store_arrays(), old, "the sharer still holds the old store")
    assert o.n_reads == len(old["word_off"]) - 1
    CR.assert_same(c.store_arrays(), want, "the cutter holds the new one")
    o.share_reads(c)
    CR.assert_same(o.store_arrays(), want, "after share_reads")
    assert o.n_reads == len(tab)
    o.cut_store(CC.pieces([(0, 1, 20)]))                                      # the sharer cuts: the first holder keeps its store
    CR.assert_same(c.store_arrays(), want, "the first holder after the sharer's cut")
    CR.assert_same(o.store_arrays(), CR.cut(want, CC.pieces([(0, 1, 20)])), "the sharer's cut")


def test_a_job_of_the_old_store_refuses_and_a_refused_table_leaves_the_store():
    c = G.ctx()
    rs = PC.set_d()
    PC.load(c, rs)
    p = c.find_overlap_pairs(**PC.DEFAULTS)
    m = p.align()
    job = c.create_job_paired(p, m, 256)
    try:
        before = c.store_arrays()
        for rows, text in (([(0, 0, 10), (10, 0, 0)], "piece 1: rid outside the reads"), ([(0, 0, 3001)], "piece 0: end beyond the read"), ([(1, 5, 4)], "piece 0: start > end")):
            with pytest.raises(api.HerroError) as e:
                c.cut_store(CC.pieces(rows))
            assert e.value.code == -1 and text in str(e.value)
        CR.assert_same(c.store_arrays(), before, "after refused tables")
        assert c.n_reads == len(rs.reads)
        job.featurize()                                                       # the store is as it was: the job still runs
        c.cut_store(CC.pieces([(i, 0, len(r)) for i, r in enumerate(rs.reads)]))   # even the identity table makes a new store
        CR.assert_same(c.store_arrays(), before, "identity")
        with pytest.raises(api.HerroError) as e:
            job.featurize()
        assert e.value.code == -6 and "the read store was replaced" in str(e.value)
    finally:
        for x in (job, m, p):
            x.close()
    fresh = api.Context(0)
    try:
        with pytest.raises(api.HerroError) as e:
            fresh.cut_store(CC.pieces([]))
        assert e.value.code == -6
    finally:
        fresh.close()


# ---- 3. end to end ----------------------------------------------------------------------------------------------------------------------------
def _raw_sets():
    clean, raw, _ = AC.chimera_parts()                                        # = adapter_cases.set_chimera()'s reads: trimmed at both ends, two split
    both_ends = [AC.A28 + r + AC.LC.rc(AC.A22) for r in PC.set_d().reads]     # pair_cases.set_d with an adapter at either end of every read
    return dict(chimera=raw, both_ends=both_ends)


def _windows(c):
    p = c.find_overlap_pairs(**PC.DEFAULTS)
    m = p.align()
    job = c.create_job_paired(p, m, 256)
    job.featurize()
    wins = [job.window(w) for w in range(job.n_windows)]
    out = (PC.pairs_fields(p), [(w.bases.copy(), w.quals.copy(), w.qids.copy()) for w in wins])
    for x in (job, m, p):
        x.close()
    return out


def test_name_classes_given_to_the_cut_reach_the_jobs_as_those_of_set_reads_do():
    """twelve reads that all overlap each other (pair_cases.set_a) with an adapter at either end, trimmed on both paths with name classes that put
    reads 2 i and 2 i + 1 into one class (a job keeps one error-ratio slot per target and class, which ranks a window's overlaps): the windows of
    a paired job agree — and differ from those of the classes NULL stands for, so the classes did arrive.  The job's descriptors come from the
    context's host-side read_len, h_word_off and h_qual_off, which this holds to the host path's as well."""
    sb = PC.set_a()
    o = np.asarray(sb.off, np.int64)
    tail = AC.LC.rc(AC.A22)
    seq = b"".join(AC.A28 + np.asarray(sb.seq[o[i]:o[i + 1]], np.uint8).tobytes() + tail for i in range(sb.n_reads))
    qual = np.concatenate([np.concatenate([np.full(28, 73, np.uint8), np.asarray(sb.qual[o[i]:o[i + 1]], np.uint8), np.full(22, 73, np.uint8)]) for i in range(sb.n_reads)])
    off = np.concatenate([[0], np.cumsum(np.diff(o) + 50)]).astype(np.uint64)
    reads = io.Reads([b"r%d" % i for i in range(sb.n_reads)], [None] * sb.n_reads, np.frombuffer(seq, np.uint8), qual, off)
    c = G.ctx()
    c.set_reads(reads.seq, reads.qual, reads.off)
    hits, hits_off = c.find_adapters([AC.A28, AC.A22], max_err_pm=AC.CHIMERA_PM)
    pieces, _, stats = api.trim_plan(np.diff(off.astype(np.int64)).astype(np.uint32), [28, 22], hits, hits_off)
    assert len(pieces) == sb.n_reads and stats.reads_trimmed == sb.n_reads and pieces["rid"].tolist() == list(range(sb.n_reads))
    classes = (np.arange(len(pieces)) // 2).astype(np.uint32)
    c.cut_store(pieces, name_class=classes)
    dev_store = c.store_arrays()
    dev_pairs, dev_windows = _windows(c)
    cut = io.cut_reads(reads, pieces)
    c.set_reads(cut.seq, cut.qual, cut.off, name_class=classes)
    CR.assert_same(dev_store, c.store_arrays(), "classes")
    host_pairs, host_windows = _windows(c)
    PC.assert_same_fields(dev_pairs, host_pairs, "classes")
    assert len(dev_windows) == len(host_windows) > 100
    for w, (a, b) in enumerate(zip(dev_windows, host_windows)):
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), w
    c.set_reads(reads.seq, reads.qual, reads.off)
    c.cut_store(pieces)                                                       # NULL: every read its own class
    _, plain_windows = _windows(c)
    differ = sum(not all(np.array_equal(x, y) for x, y in zip(a, b)) for a, b in zip(dev_windows, plain_windows))
    print("windows that differ between the paired classes and one class per read:", differ, "of", len(plain_windows))
    assert len(plain_windows) == len(dev_windows) and differ > 0


@pytest.mark.parametrize("which", ["chimera", "both_ends"])
def test_trim_reads_on_the_device_equals_the_host_path(which):
    raw = _raw_sets()[which]
    rng = np.random.default_rng(310)
    rs = AC.as_reads(raw)
    reads = io.Reads([b"read%d" % i for i in range(len(raw))], [b"d %d" % i if i % 2 else None for i in range(len(raw))], rs.seq,
                     rng.integers(33, 90, len(rs.seq)).astype(np.uint8), rs.off)
    c = G.ctx()
    dev, dev_stats = api.trim_reads(c, reads, [AC.A28, AC.A22], max_err_pm=AC.CHIMERA_PM, on_device=True)
    assert dev.seq is None and dev.qual is None and c.n_reads == len(dev.ids)
    dev_store = c.store_arrays()
    dev_pairs, dev_windows = _windows(c)
    host, host_stats = api.trim_reads(c, reads, [AC.A28, AC.A22], max_err_pm=AC.CHIMERA_PM)
    assert dev.ids == host.ids and dev.descriptions == host.descriptions and dev.off.tolist() == host.off.tolist() and dev_stats == host_stats
    assert dev_stats.reads_trimmed == len(raw) and dev_stats.reads_split == (2 if which == "chimera" else 0)
    CR.assert_same(dev_store, c.store_arrays(), which)
    host_pairs, host_windows = _windows(c)
    assert len(host_pairs["primaries"]) >= 4 and len(host_windows) > 10
    PC.assert_same_fields(dev_pairs, host_pairs, which)
    assert len(dev_windows) == len(host_windows)
    for w, (a, b) in enumerate(zip(dev_windows, host_windows)):
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), (which, w)
