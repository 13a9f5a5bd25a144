"""-m gpu: the device job build (k_cigar_scan / k_ops_scan -> k_window_cuts -> k_scan_alns -> k_win_pass<false> -> k_scan_wins ->
k_win_pass<true>: csrc/cigar_dev.hip, csrc/build_dev.hip) past the sizes at which its loops run once and at the edges of the windowing,
on the cases of tests/build_cases.py: more than one pass of k_scan_alns (8192 alignments each, a carry between them), two to four
windows per thread of k_scan_wins with empty and short ranges, two to four rounds of k_win_pass over a target's alignments, targets
that give no overlap between others, and the hand-made alignments of tests/aligned_dev_cases.py at W = 16 and W = 40.

Two references, both needed: the job the same context builds on the host (herro_debug_set_host_build) from the device scan's records
— field for field, it shares the scan kernel and nothing behind it — and the job of a device-free api.HostContext, which shares
nothing with the device and which tests/test_build_cases.py holds to the oracle's extract_windows on these very cases.  Every
comparison is exact."""
import numpy as np
import pytest

import aligned_dev_cases as AC
import build_cases as BC
import gpu_common as G
from herro_amd import api
from test_gpu_build_dev import _same
from test_gpu_cigar_scan import _same_jobs

pytestmark = pytest.mark.gpu


def _built(c, job):
    return c._l.herro_debug_job_dev_built(job.h)


def _lens(sb):
    return (sb.off[1:] - sb.off[:-1]).astype(np.uint32)


def _text_jobs(c, hc, case):
    """(device-built job, job of the same context built by the host, job of the device-free context) from the CIGAR texts"""
    _, W, rids, rows, aln_off, cigars = case
    jd = c.create_job(rids, rows, aln_off, cigars, W)
    c.host_build(True)
    try:
        jh = c.create_job(rids, rows, aln_off, cigars, W)
    finally:
        c.host_build(False)
    jx = hc.create_job(rids, rows, aln_off, cigars, W)
    return jd, jh, jx


def _ops_job(c, case):
    """the job of the same alignments from binary ops (k_ops_scan: exactly n_ops slots per alignment in the op array)"""
    _, W, rids, rows, aln_off, cigars = case
    op_off, ops = AC.cigars_to_ops(cigars)
    h = c.aligned_dev_from_ops(rows, op_off, ops)
    try:
        return c.create_job_aligned(rids, aln_off, np.arange(len(rows), dtype=np.uint32), h, W)
    finally:
        h.close()


def _compare(c, hc, case, tag, with_ops):
    """The jobs of `case`, compared; returns (device-built job, host-built job of the same context) still open, the others closed."""
    jd, jh, jx = _text_jobs(c, hc, case)
    ja = None
    try:
        assert _built(c, jd) == 1 and _built(c, jh) == 0, tag
        ad = c.job_arrays(jd)
        _same(ad, c.job_arrays(jh), tag)
        n_ow = _same_jobs(hc, jd, jx)
        assert jd.skipped() == jh.skipped() == jx.skipped(), tag
        assert len(ad["win"]) == BC.n_windows(case) and n_ow == len(ad["ow"])
        if with_ops:
            ja = _ops_job(c, case)
            assert _built(c, ja) == 1, tag
            AC.same_jobs(c, ja, jd, tag + " (ops, text)")
            AC.same_jobs(c, ja, jx, tag + " (ops, host context)")
    except BaseException:
        jd.close(); jh.close()
        raise
    finally:
        jx.close()
        if ja is not None:
            ja.close()
    return jd, jh, ad


def _same_pileup(jd, jh, windows):
    """behind featurize(), the windows' counts and encoded features of the two jobs (every byte of them is addressed through the
    offsets the build computed: scr_off, ev_off, col_off, row_off, the tile list)"""
    for w in windows:
        a, b = jd.window(w, encoded=True), jh.window(w, encoded=True)
        x, y = a.info, b.info
        assert (x.rid, x.wid, x.n_total_wins, x.length, x.n_supported, x.n_overlaps, x.n_alns) == \
               (y.rid, y.wid, y.n_total_wins, y.length, y.n_supported, y.n_overlaps, y.n_alns), w
        assert np.array_equal(a.bases, b.bases) and np.array_equal(a.quals, b.quals), w
        assert np.array_equal(a.sup_pos, b.sup_pos) and np.array_equal(a.sup_ins, b.sup_ins), w


def _pileup_windows(name, case, arr):
    """the windows whose offsets come out of a carry or of a thread's second and later window"""
    n_win = len(arr["win"])
    if name.startswith("aln_"):
        n, aln_off, two = len(case[3]), case[4].astype(np.int64), arr["tgt_win_off"].astype(np.int64)
        assert n in (8193, 16385)
        alns = [a for k in range(1, n // BC.SCAN_ALNS_PASS + 1) for a in (k * BC.SCAN_ALNS_PASS - 1, k * BC.SCAN_ALNS_PASS)] + [n - 1]
        tg = sorted({int(np.searchsorted(aln_off, a, "right")) - 1 for a in alns})
        assert tg[-1] == len(case[2]) - 1                # (one target may hold them all: 8193 alignments end in the target of 8191)
        return [w for t in tg for w in range(int(two[t]), int(two[t + 1]))]
    assert name == "win_3077"
    return sorted({w for mid in (1024, 2048) for w in range(mid - 8, mid + 8)} | set(range(n_win - 8, n_win)))


WITH_OPS = ("aln_8193", "aln_16385", "win_1025", "win_3077")
WITH_PILEUP = ("aln_8193", "aln_16385", "win_3077")


@pytest.mark.parametrize("name", list(BC.SIZE_CASES))
def test_device_build_equals_both_host_builds_at_the_sizes_of_its_loops(name):
    case = BC.SIZE_CASES[name]()                         # (asserts the count it is named for)
    sb = case[0]
    c = G.ctx()
    G.load_synth(c, sb)
    hc = api.HostContext(_lens(sb))
    try:
        jd, jh, ad = _compare(c, hc, case, name, with_ops=name in WITH_OPS)
    finally:
        hc.close()
    try:
        assert len(ad["ow"]) > 0
        if name == "holes":
            BC.check_holes(ad["win"])
            assert jd.skipped() == (3, 0)
        if name in WITH_PILEUP:
            jd.featurize(); jh.featurize()
            _same_pileup(jd, jh, _pileup_windows(name, case, ad))
    finally:
        jd.close(); jh.close()


@pytest.mark.parametrize("W", [AC.HAND_W, AC.HAND_W40])
def test_hand_cases_text_ops_and_both_host_builds_agree(W):
    """each hand case alone (a case cannot lean on its neighbours' slots) and all in one job: the device job from text, the device
    job from binary ops, the host build behind the device scan and the device-free host build are one job"""
    names, lst, want = BC.hand_set(W)                    # (asserts the stated overlap counts against the oracle)
    whole = BC.hand_case(W)
    sb = whole[0]
    c = G.ctx()
    G.load_synth(c, sb)
    hc = api.HostContext(_lens(sb))
    try:
        for i, name in [(None, f"hand W={W}")] + list(enumerate(names)):
            jd, jh, ad = _compare(c, hc, BC.hand_case(W, i), name, with_ops=True)
            jd.close(); jh.close()
            if i is None:
                assert sorted(set(ad["ow"]["qid"].tolist())) == [k + 1 for k, n in enumerate(names) if want.get(n, 1)]
            else:
                assert name not in want or len(ad["ow"]) == want[name], (name, len(ad["ow"]))
    finally:
        hc.close()
