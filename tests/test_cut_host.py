"""The store cut without a GPU (herro_store_cut; DESIGN.md §13, "The cut on the device"): tests/cut_ref.py against the existing host path
(io.cut_reads + api.encode_2bit) on the all-ACGT sets, its documented difference on the others, every refusal of herro_store_cut on a
context without a device, and the naming rule through both of its callers."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cut_cases as CC  # noqa: E402
import cut_ref as CR  # noqa: E402
from herro_amd import api, io  # noqa: E402


def _reads_of(name):
    s = CC.get(name)
    seq, qual, off = CC.arrays(name)
    return io.Reads([b"r%d" % i for i in range(len(s["reads"]))], [None] * len(s["reads"]), seq, qual, off)


# ---- 1. the reference against the host path ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,table", [t for t in CC.ALL_TABLES if CC.get(t[0])["acgt"]], ids=[i for t, i in zip(CC.ALL_TABLES, CC.IDS) if CC.get(t[0])["acgt"]])
def test_reference_equals_cut_reads_then_encode(name, table):
    """all bytes ACGT: the six arrays are those of the cut reads encoded from their ASCII"""
    _, want = CC.reference(name, table)
    cut = io.cut_reads(_reads_of(name), CC.get(name)["tables"][table][1])
    o = cut.off.astype(np.int64)
    reads = [cut.seq[o[i]:o[i + 1]].tobytes() for i in range(len(o) - 1)]
    host = CR.store_of(reads, [cut.qual[o[i]:o[i + 1]] for i in range(len(o) - 1)])
    CR.assert_same(want, host, (name, table))
    assert len(want["words"]) == int(want["word_off"][-1]) + 1 and int(want["words"][-1]) == 0
    assert len(want["p0"]) == len(want["words"]) + 1 and not want["p0"][-2:].any() and not want["p1"][-2:].any()


def test_identity_table_gives_the_store_back():
    old, new = CC.reference("shapes", [t for t, _ in CC.get("shapes")["tables"]].index("identity"))
    CR.assert_same(new, old, "identity")


def test_reference_on_reads_that_are_not_acgt_moves_the_parents_codes():
    """the documented difference: a piece holds the codes its parent holds — what a non-ACGT byte smeared over the bases behind it stays, and the
    bits above the piece's end are zero even where the parent's smear reached above the read's end; the host path re-encodes and differs"""
    s = CC.get("nonacgt")
    tab = s["tables"][0][1]
    old, new = CC.reference("nonacgt", 0)
    differs = 0
    for x, p in enumerate(tab):
        rid, start, end = int(p["rid"]), int(p["start"]), int(p["end"])
        assert np.array_equal(CR.read_codes(new, x), CR.read_codes(old, rid)[start:end]), x
        w1 = int(new["word_off"][x + 1])
        if (end - start) % 32:
            assert int(new["words"][w1 - 1]) >> (2 * ((end - start) % 32)) == 0, x
        host = api.encode_2bit(s["reads"][rid][start:end]) if end > start else np.zeros(0, np.uint64)
        differs += not np.array_equal(host, new["words"][int(new["word_off"][x]):w1])
    assert differs > 10
    n_last = next(i for i, r in enumerate(s["reads"]) if r.endswith(b"N") and len(r) == 71)
    assert int(old["words"][int(old["word_off"][n_last + 1]) - 1]) >> (2 * 7) != 0        # the smear above the read's end in the old store


# ---- 2. herro_store_cut's refusals on a context without a device ------------------------------------------------------------------------------
def _refused(c, rows, code, text):
    with pytest.raises(api.HerroError) as e:
        c.cut_store(CC.pieces(rows))
    assert e.value.code == code and text in str(e.value), str(e.value)


def test_store_cut_refuses_a_bad_table_before_it_asks_for_a_device():
    c = api.HostContext(np.array([10, 0, 33], np.uint32))
    try:
        _refused(c, [(0, 0, 10), (3, 0, 0)], -1, "herro_store_cut: piece 1: rid outside the reads")
        _refused(c, [(0, 5, 4), (3, 0, 0)], -1, "herro_store_cut: piece 0: start > end")
        _refused(c, [(2, 0, 33), (1, 0, 0), (0, 0, 11)], -1, "herro_store_cut: piece 2: end beyond the read")
        _refused(c, [(1, 0, 1)], -1, "herro_store_cut: piece 0: end beyond the read")
        L = api.lib()
        assert L.herro_store_cut(c.h, 3, None, None) == -1 and "null piece table" in c.last_error()
        one = CC.pieces([(0, 0, 1)])
        assert L.herro_store_cut(c.h, 2 ** 31, one.ctypes.data, None) == -4 and "more than 2^31 - 1 pieces" in c.last_error()
        # a good table (and an empty one): the context has no device
        _refused(c, [(0, 0, 10), (2, 1, 33), (1, 0, 0)], -2, "herro_store_cut: the context has no device")
        _refused(c, [], -2, "herro_store_cut: the context has no device")
        assert c.n_reads == 3
        with pytest.raises(api.HerroError) as e:
            c.cut_store(CC.pieces([(0, 0, 1)]), name_class=[1, 2])
        assert e.value.code == -1
        with pytest.raises(api.HerroError) as e:
            c.store_arrays()
        assert e.value.code == -2
    finally:
        c.close()


# ---- 3. the naming rule through both of its callers -------------------------------------------------------------------------------------------
def test_the_naming_rule_is_the_same_through_cut_reads_and_cut_names():
    reads = io.Reads([b"a", b"b", b"c"], [b"first read", None, b""], np.frombuffer(b"ACGTACGTAC" + b"GGGG" + b"TTTTTTTTTTTT", np.uint8),
                     np.arange(26, dtype=np.uint8) + 40, np.array([0, 10, 14, 26], np.uint64))
    tab = CC.pieces([(2, 6, 12), (0, 0, 4), (2, 0, 3), (0, 6, 10), (2, 3, 6), (1, 1, 1)])
    cut = io.cut_reads(reads, tab)
    ids, descs, off = io.cut_names(reads.ids, reads.descriptions, reads.off, tab)
    assert ids == cut.ids == [b"c_1", b"a_1", b"c_2", b"a_2", b"c_3", b"b"]
    assert descs == cut.descriptions == [b"", b"first read", b"", b"first read", b"", None]
    assert off.dtype == np.uint64 and off.tolist() == cut.off.tolist() == [0, 6, 10, 13, 17, 20, 20]
    ids, descs, off = io.cut_names(reads.ids, reads.descriptions, reads.off + np.uint64(100), CC.pieces([]))    # off need not start at 0
    assert ids == [] and descs == [] and off.tolist() == [0]
    for rows, text in (([(3, 0, 0)], "piece 0: rid outside the reads"), ([(0, 0, 1), (1, 3, 2)], "piece 1: start > end"), ([(1, 0, 5)], "piece 0: end beyond the read")):
        for fn, who in ((lambda t: io.cut_reads(reads, t), "herro_reads_cut: "), (lambda t: io.cut_names(reads.ids, reads.descriptions, reads.off, t), "herro_reads_cut_names: ")):
            with pytest.raises(ValueError, match=who + text):
                fn(CC.pieces(rows))
