"""not-gpu: the device-free half of the device-resident hand-off (herro_align_overlaps_dev / herro_aligned_dev_from_ops /
herro_job_create_aligned): error codes without a device, the argument checks, the fallback through the
text of the ops on a herro_debug_host_ctx context, and the Python regrouping helper."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aligned_dev_cases as AC  # noqa: E402
from herro_amd import api, synth  # noqa: E402


def _host_ctx(sb):
    return api.HostContext((sb.off[1:] - sb.off[:-1]).astype(np.uint32))


def test_align_dev_needs_a_device():
    sb = synth.generate(1, 600, 4, seed=2, flank_min=20, flank_max=40)
    c = _host_ctx(sb)
    with pytest.raises(api.HerroError) as e:
        c.align_dev(sb.aln[:, :9])
    assert e.value.code == -2 and "no device" in str(e.value)          # HERRO_E_NO_DEVICE, the text path's message
    with pytest.raises(api.HerroError) as t:
        c.align(sb.aln[:, :9])
    assert str(t.value) == str(e.value)


def test_argument_errors_of_create_job_aligned():
    sb = synth.generate(1, 600, 4, seed=2, flank_min=20, flank_max=40)
    c = _host_ctx(sb)
    L = c._l
    rids = np.array([sb.tgt_rid[0]], np.uint32)
    off = np.array([0, 2], np.uint64)
    rec = np.array([0, 1], np.uint32)
    assert not L.herro_job_create_aligned(c.h, 1, rids.ctypes.data, off.ctypes.data, rec.ctypes.data, None, 256)
    assert L.herro_job_create_status(c.h) == -1 and "null handle" in c.last_error()
    op_off, ops = AC.cigars_to_ops([sb.cigar(a) for a in range(len(sb.aln))])
    h = c.aligned_dev_from_ops(sb.aln[:, :9], op_off, ops)
    assert not L.herro_job_create_aligned(c.h, 1, rids.ctypes.data, off.ctypes.data, None, h.h, 256)
    assert L.herro_job_create_status(c.h) == -1 and "null rec" in c.last_error()
    with pytest.raises(api.HerroError) as e:                             # an index outside the handle, named
        c.create_job_aligned(rids, off, np.array([0, len(sb.aln)], np.uint32), h, 256)
    assert e.value.code == -1 and f"rec[1] = {len(sb.aln)}" in str(e.value)
    other = _host_ctx(sb)
    with pytest.raises(api.HerroError) as e:                             # a handle of another context
        other.create_job_aligned(rids, off, rec, h, 256)
    assert e.value.code == -1 and "another context" in str(e.value)
    # a record without ops counts as failed: refused by name
    op_off2 = op_off.copy()
    op_off2[2:] -= op_off[2] - op_off[1]
    h2 = c.aligned_dev_from_ops(sb.aln[:, :9], op_off2, ops)
    assert h2.ok.tolist() == [True, False] + [True] * (len(sb.aln) - 2) and h2.failed == 1 and h2.scores[1] == np.iinfo(np.int32).min
    assert h2.cigar(1) == b"" and h2.cigar(0) == sb.cigar(0)
    with pytest.raises(api.HerroError) as e:
        c.create_job_aligned(rids, off, rec, h2, 256)
    assert e.value.code == -1 and "rec[1] = 1" in str(e.value) and "failed" in str(e.value)
    assert L.herro_aligned_dev_cigar(h.h, len(sb.aln), None, 0) == -1
    h.close(); h2.close()


def test_a_device_free_context_goes_through_the_text_of_the_ops():
    """the fallback of herro_job_create_aligned, all of it on the host: the job of herro_job_create on the texts of the same ops"""
    sb = synth.generate(3, 1500, 8, seed=7, flank_min=30, flank_max=60, p_partial=0.3)
    c = _host_ctx(sb)
    op_off, ops = AC.cigars_to_ops([sb.cigar(a) for a in range(len(sb.aln))])
    h = c.aligned_dev_from_ops(sb.aln[:, :9], op_off, ops)
    assert all(h.cigar(r) == sb.cigar(r) for r in range(len(sb.aln)))
    order = [2, 0]                                                       # a subset of the targets, regrouped
    rec = np.concatenate([np.arange(int(sb.tgt_aln_off[t]), int(sb.tgt_aln_off[t + 1])) for t in order]).astype(np.uint32)
    off = np.concatenate([[0], np.cumsum([int(sb.tgt_aln_off[t + 1] - sb.tgt_aln_off[t]) for t in order])]).astype(np.uint64)
    ja = c.create_job_aligned(sb.tgt_rid[order], off, rec, h, 256)
    h.close()                                                            # the job owns its ops
    jt = api.job_from_synth(c, sb, 256, order)
    assert c._l.herro_debug_job_dev_built(ja.h) == 0
    a, t = AC.same_jobs(c, ja, jt, "host")
    assert len(a["ow"]) > 0 and np.array_equal(a["ow"]["op_begin"], t["ow"]["op_begin"]) and np.array_equal(a["ops"], t["ops"])
    ja.close(); jt.close()
    # what herro_job_create refuses as text is refused with its words
    tstart, pairs = AC.ZERO_LEN_CASE
    seq, qual, roff, rows = AC.hand_reads([(tstart, pairs)])
    c2 = api.HostContext((roff[1:] - roff[:-1]).astype(np.uint32))
    h = c2.aligned_dev_from_ops(rows, [0, len(pairs)], AC.pairs_ops(pairs))
    one = (np.array([0], np.uint32), np.array([0, 1], np.uint64))
    with pytest.raises(api.HerroError) as ea:
        c2.create_job_aligned(*one, np.array([0], np.uint32), h, AC.HAND_W)
    with pytest.raises(api.HerroError) as et:
        c2.create_job(one[0], rows, one[1], [AC.pairs_text(pairs)], AC.HAND_W)
    assert ea.value.code == et.value.code and str(ea.value) == str(et.value)
    h.close()


def test_regrouping_helper():
    rids = np.array([7, 3, 9, 4], np.uint32)
    aln_off = np.array([0, 3, 5, 5, 8], np.uint64)
    ok = np.array([1, 0, 1, 0, 0, 1, 1, 0], bool)                        # target 3 (records 3, 4): all failed; target 9: none at all
    r, off, rec = api.aligned_dev_job_args(rids, aln_off, ok)
    assert r.tolist() == [7, 3, 9, 4] and off.tolist() == [0, 2, 2, 2, 4] and rec.tolist() == [0, 2, 5, 6]
    assert off.dtype == np.uint64 and rec.dtype == np.uint32
    # the same grouping as the text path's helper
    rows = np.arange(8 * 10, dtype=np.uint32).reshape(8, 10)
    _, rows2, off2, cig2 = api.aligned_job_args(rids, aln_off, rows, [b"%dM" % i for i in range(8)], ok)
    assert off2.tolist() == off.tolist() and np.array_equal(rows2, rows[rec]) and cig2 == [b"%dM" % i for i in rec]
    r, off, rec = api.aligned_dev_job_args(np.zeros(0, np.uint32), np.zeros(1, np.uint64), np.zeros(0, bool))
    assert len(r) == 0 and off.tolist() == [0] and len(rec) == 0
    r, off, rec = api.aligned_dev_job_args(rids[:2], [0, 2, 3], np.zeros(3, bool))
    assert off.tolist() == [0, 0, 0] and len(rec) == 0
