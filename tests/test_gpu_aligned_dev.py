"""gpu: the device-resident hand-off from the aligner to the job builder — herro_align_overlaps_dev keeps every
record's ops on the device, herro_job_create_aligned builds the job from them through k_ops_scan (csrc/cigar_dev.hip), the binary
sibling of k_cigar_scan.  Everything is held to the text path: the job herro_job_create builds from the texts of the same ops, the
records herro_align_overlaps returns, the FASTA of the chain through align -> aligned_job_args -> create_job.  Both sides of the
hand-case comparison below are device builds through the same k_window_cuts: the hand cases (with more of them, and a set at W = 40) are
held to the host build in tests/test_gpu_build_sizes.py and, through it, to the oracle's extract_windows in tests/test_build_cases.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import aligned_dev_cases as AC  # noqa: E402
import gpu_common as G  # noqa: E402
from herro_amd import api, synth  # noqa: E402
from test_gpu_build_dev import CASES  # noqa: E402

pytestmark = pytest.mark.gpu


def _built(c, job):
    return c._l.herro_debug_job_dev_built(job.h)


# ---- 1. the scan kernel against the text path, from caller-supplied ops ---------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_jobs_from_binary_ops_equal_the_text_paths(name):
    cs = CASES[name]
    sb = synth.generate(cs["n"], cs["tl"], cs["ov"], seed=synth.SEED + 61 + sum(map(ord, name)), **cs["kw"])
    c = G.ctx()
    G.load_synth(c, sb)
    op_off, ops = AC.cigars_to_ops([sb.cigar(a) for a in range(len(sb.aln))])
    h = c.aligned_dev_from_ops(sb.aln[:, :9], op_off, ops)
    ja = c.create_job_aligned(sb.tgt_rid, sb.tgt_aln_off, np.arange(len(sb.aln), dtype=np.uint32), h, cs["W"])
    h.close()
    jt = api.job_from_synth(c, sb, cs["W"])
    try:
        assert _built(c, ja) == 1 and _built(c, jt) == 1
        a, _ = AC.same_jobs(c, ja, jt, name)
        assert len(a["ow"]) > 0 and len(a["ops"]) == len(ops)            # room for exactly n_ops per alignment
        ja.featurize(); jt.featurize()
        for w in range(jt.n_windows):
            x, y = ja.info(w), jt.info(w)
            assert (x.rid, x.wid, x.n_total_wins, x.length, x.n_alns, x.n_overlaps, x.n_supported, x.win_len) == \
                   (y.rid, y.wid, y.n_total_wins, y.length, y.n_alns, y.n_overlaps, y.n_supported, y.win_len), w
    finally:
        ja.close(); jt.close()


# ---- 2. hand cases at the kernel's own edges --------------------------------------------------------------------------------------------
def _hand(c, cases):
    seq, qual, off, rows = AC.hand_reads(cases)
    c.set_reads(seq, qual, off)
    pairs = [p for _, p in cases]
    n = [len(p) for p in pairs]
    op_off = np.concatenate([[0], np.cumsum(n)]).astype(np.uint64)
    ops = np.concatenate([AC.pairs_ops(p) for p in pairs])
    return rows, op_off, ops, [AC.pairs_text(p) for p in pairs]


def test_hand_cases_at_the_edges_of_the_scan_kernel():
    cases = AC.hand_cases()
    W = AC.HAND_W
    # the cases are what their names say
    n_ops = {k: len(p) for k, (_, p) in cases.items()}
    assert (n_ops["one_op"], n_ops["ops_64"], n_ops["ops_65"]) == (1, 64, 65) and n_ops["ops_201"] > 128
    t0, p = cases["cut_on_op_63"]
    t63 = t0 + sum(ln for ln, ty in p[:63] if ty != "I")
    assert p[63][1] == "D" and t63 // W < (t63 + p[63][0]) // W and len(p) > 65          # op 63 crosses a boundary; o1, o2 lie in the next step
    assert cases["one_op"][1][0][0] >= 3 * W and cases["tstart_odd"][0] % W != 0
    t0, p = cases["d_across_boundary"]
    assert p[1][1] == "D" and (t0 + p[0][0]) % W and (t0 + p[0][0]) // W < (t0 + p[0][0] + p[1][0]) // W
    t0, p = cases["i_before_boundary"]
    assert p[1][1] == "I" and (t0 + p[0][0]) % W == 0
    t0, p = cases["m_three_windows"]
    assert p[2] == (60, "M") and (t0 + 5 + 60) // W - (t0 + 5) // W >= 3
    c = G.ctx()
    rows, op_off, ops, texts = _hand(c, list(cases.values()))
    rid, off, rec = np.array([0], np.uint32), np.array([0, len(rows)], np.uint64), np.arange(len(rows), dtype=np.uint32)
    h = c.aligned_dev_from_ops(rows, op_off, ops)
    assert [h.cigar(r) for r in range(len(rows))] == texts
    ja = c.create_job_aligned(rid, off, rec, h, W)
    jt = c.create_job(rid, rows, off, texts, W)
    try:
        assert _built(c, ja) == 1 and _built(c, jt) == 1
        a, _ = AC.same_jobs(c, ja, jt, "hand")
        assert sorted(set(a["ow"]["qid"].tolist())) == list(range(1, len(rows) + 1))      # every case contributes windows
        # each alone, so that a case cannot lean on its neighbours' slots
        for i, name in enumerate(cases):
            j1 = c.create_job_aligned(rid, np.array([0, 1], np.uint64), np.array([i], np.uint32), h, W)
            j2 = c.create_job(rid, rows[i:i + 1], np.array([0, 1], np.uint64), [texts[i]], W)
            assert _built(c, j1) == 1, name
            AC.same_jobs(c, j1, j2, name)
            j1.close(); j2.close()
    finally:
        h.close(); ja.close(); jt.close()


def test_two_insertions_in_a_row_take_the_fallback():
    c = G.ctx()
    cases = [AC.hand_cases()["ops_65"], AC.INS_PAIR_CASE]
    rows, op_off, ops, texts = _hand(c, cases)
    rid, off, rec = np.array([0], np.uint32), np.array([0, 2], np.uint64), np.array([0, 1], np.uint32)
    h = c.aligned_dev_from_ops(rows, op_off, ops)
    ja = c.create_job_aligned(rid, off, rec, h, AC.HAND_W)
    h.close()
    jt = c.create_job(rid, rows, off, texts, AC.HAND_W)
    try:
        assert _built(c, ja) == 0                                        # CIG_INS_PAIR: the job went through the text of its ops
        a, t = AC.same_jobs(c, ja, jt, "ins pair")
        assert set(a["ow"]["qid"].tolist()) == {1, 2} and np.array_equal(a["ow"]["op_begin"], t["ow"]["op_begin"])
    finally:
        ja.close(); jt.close()


def test_a_zero_length_op_fails_with_the_text_paths_words():
    c = G.ctx()
    rows, op_off, ops, texts = _hand(c, [AC.ZERO_LEN_CASE])
    assert texts[0].startswith(b"30M0D")
    one = (np.array([0], np.uint32), np.array([0, 1], np.uint64))
    h = c.aligned_dev_from_ops(rows, op_off, ops)
    with pytest.raises(api.HerroError) as ea:
        c.create_job_aligned(*one, np.array([0], np.uint32), h, AC.HAND_W)
    with pytest.raises(api.HerroError) as et:
        c.create_job(one[0], rows, one[1], texts, AC.HAND_W)
    h.close()
    assert ea.value.code == et.value.code and str(ea.value) == str(et.value)
    assert c._l.herro_job_create_status(c.h) == et.value.code


# ---- 3. the aligner's handle --------------------------------------------------------------------------------------------------------------
_CHILD = r"""
import json, os, sys
sys.path.insert(0, os.path.join(sys.argv[1], "tests")); sys.path.insert(0, sys.argv[1])
import aligned_dev_cases as AC
from herro_amd import api
sb, rows = AC.align_batch()
c = api.Context(0)
c.set_reads(sb.seq, sb.qual, sb.off)
h = c.align_dev(rows)
print(json.dumps({"rows": h.rows.tolist(), "sc": h.scores.tolist(), "n_ops": h.n_ops.tolist(), "cig": [h.cigar(r).decode() for r in range(h.n)]}))
"""


def test_the_aligners_handle_equals_the_text_result():
    sb, rows = AC.align_batch()
    span = (rows[:, 3] - rows[:, 2]).astype(np.int64) + (rows[:, 8] - rows[:, 7])
    assert 280 <= len(rows) <= 320 and set(rows[:, 4].tolist()) == {0, 1} and span.max() >= 20000 and (span == 2).sum() == 1
    c = G.ctx()
    G.load_synth(c, sb)
    out, cig, sc, ok = c.align(rows)
    assert (~ok).sum() == 2 and not ok[-1] and not ok[-2] and ok[-3]     # exactly the intended failures; the one-base region aligns
    h = c.align_dev(rows)
    try:
        assert h.n == len(rows) and h.failed == 2
        assert np.array_equal(h.rows[:, :9], out[:, :9]) and not h.rows[:, 9].any()
        assert np.array_equal(h.scores, sc) and np.array_equal(h.ok, ok)
        got = [h.cigar(r) for r in range(h.n)]
        assert got == cig
        assert h.n_ops.tolist() == [len(AC.cigar_ops(x)) for x in cig]
    finally:
        h.close()
    env = dict(os.environ, HERRO_ALIGN_SCRATCH_MB="1")                   # many chunks (the 12 kb records run alone): the store grows chunk by chunk
    p = subprocess.run([sys.executable, "-c", _CHILD, G.ROOT], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    child = json.loads(p.stdout.strip().splitlines()[-1])
    assert child["rows"] == [r[:9] + [0] for r in out.tolist()] and child["sc"] == sc.tolist()
    assert child["cig"] == [x.decode() for x in cig] and child["n_ops"] == [len(AC.cigar_ops(x)) for x in cig]


# ---- 4. end to end --------------------------------------------------------------------------------------------------------------------------
def _chain(c, sb, W, batch_mode, dev):
    G.load_synth(c, sb)
    rids, rows, aln_off, _ = c.find_overlaps(max_occ=64, min_score=200)
    if dev:
        h = c.align_dev(rows)
        assert h.ok.all()
        j_rids, off2, rec = api.aligned_dev_job_args(rids, aln_off, h.ok)
        job = c.create_job_aligned(j_rids, off2, rec, h, W)
        h.close()                                                        # before featurize: the job owns a copy of its ops
        assert _built(c, job) == 1
    else:
        out, cig, _, ok = c.align(rows)
        j_rids, rows2, off2, cig2 = api.aligned_job_args(rids, aln_off, out, cig, ok)
        job = c.create_job(j_rids, rows2, off2, cig2, W)
    job.featurize()
    job.infer(64, batch_mode)
    job.consensus()
    logits = [job.logits(w) for w in range(job.n_windows) if job.info(w).n_supported]
    fasta = job.fasta([sb.read_name(int(r)) for r in j_rids])
    job.close()
    return fasta, logits


@pytest.mark.parametrize("W", [256, 4096])
@pytest.mark.parametrize("batch_mode", [0, 1])
def test_end_to_end_equals_the_chain_through_text(W, batch_mode):
    sb = synth.generate(3, 8192, 8, seed=81 + W, p_partial=0.2)
    c = G.ctx()
    want, want_lg = _chain(c, sb, W, batch_mode, dev=False)
    assert want.count(b">") >= sb.n_targets and len(want_lg) > 0
    for run in range(2):
        got, lg = _chain(c, sb, W, batch_mode, dev=True)
        assert got == want, run
        assert len(lg) == len(want_lg)
        for (i1, b1), (i2, b2) in zip(lg, want_lg):
            assert np.array_equal(i1.view(np.uint32), i2.view(np.uint32)) and np.array_equal(b1.view(np.uint32), b2.view(np.uint32))


# ---- 5. selection and refusal ------------------------------------------------------------------------------------------------------------
def test_selection_and_refusal():
    sb, rows = AC.align_batch()
    c = G.ctx()
    G.load_synth(c, sb)
    out, cig, sc, ok = c.align(rows)
    h = c.align_dev(rows)
    W = 256
    try:
        # a subset of the targets in another order, every second record of each
        order = [4, 0, 7, 2]
        groups = [np.arange(int(sb.tgt_aln_off[t]), int(sb.tgt_aln_off[t + 1]))[::2] for t in order]
        rec = np.concatenate(groups).astype(np.uint32)
        assert ok[rec].all()
        off = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.uint64)
        rids = sb.tgt_rid[order]
        ja = c.create_job_aligned(rids, off, rec, h, W)
        jt = c.create_job(rids, out[rec], off, [cig[r] for r in rec], W)
        assert _built(c, ja) == 1
        a, _ = AC.same_jobs(c, ja, jt, "subset")
        assert len(a["ow"]) > 0
        ja.close()
        c.host_build(True)
        try:
            jh = c.create_job_aligned(rids, off, rec, h, W)
        finally:
            c.host_build(False)
        assert _built(c, jh) == 0
        AC.same_jobs(c, jh, jt, "host build")
        jh.close(); jt.close()
        # refusals: a failed record, an index outside the handle
        bad = len(rows) - 1
        assert not ok[bad]
        tid = int(np.flatnonzero(sb.tgt_rid == rows[bad, 5])[0])
        with pytest.raises(api.HerroError) as e:
            c.create_job_aligned(sb.tgt_rid[tid:tid + 1], [0, 2], [int(sb.tgt_aln_off[tid]), bad], h, W)
        assert e.value.code == -1 and f"rec[1] = {bad}" in str(e.value) and "failed" in str(e.value)
        assert c._l.herro_job_create_status(c.h) == -1
        with pytest.raises(api.HerroError) as e:
            c.create_job_aligned(sb.tgt_rid[tid:tid + 1], [0, 2], [int(sb.tgt_aln_off[tid]), len(rows)], h, W)
        assert e.value.code == -1 and f"rec[1] = {len(rows)}" in str(e.value) and "outside" in str(e.value)
    finally:
        h.close()
