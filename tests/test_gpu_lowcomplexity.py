"""gpu: the front end — k_sketch, the radix sort, k_runs / k_expand, k_chain, k_extend, k_align, k_ops_scan — on low-complexity reads
(tests/lowcomplexity.py), bit for bit against the numpy specifications: homopolymers, short tandem repeats and tandem copies make the
events the kernels' tie and edge rules govern (tests/test_lowcomplexity_host.py counts them); the lopsided grid carries the band along
the matrix edge; a query equal to its own reverse complement ties the two strands; and the whole path reads -> FASTA runs on this
material against the oracle fed the GPU's rows and CIGARs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import align_ref as A  # noqa: E402
import aligned_dev_cases as AC  # noqa: E402
import extend_ref as E  # noqa: E402
import gpu_common as G  # noqa: E402
import lowcomplexity as LC  # noqa: E402
import overlap_ref as R  # noqa: E402
import test_lowcomplexity_host as H  # noqa: E402
from herro_amd import api, synth  # noqa: E402
from test_gpu_extend import LENGTHS, PARAMS  # noqa: E402
from test_gpu_overlap import _same  # noqa: E402

pytestmark = pytest.mark.gpu


def _load(c, reads, qual=None):
    seq = np.frombuffer(b"".join(reads), np.uint8)
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    c.set_reads(seq, np.full(len(seq), 40 + 33, np.uint8) if qual is None else qual, off)


def _load_working_set(c):
    ws, codes = H.low()
    c.set_reads(ws.seq, ws.qual, ws.off)
    return ws, codes


# ---- sketch -----------------------------------------------------------------------------------------------------------------------------
def test_sketch_equals_the_reference():
    ws, _ = H.low()
    extra, _, _ = LC.short_and_n_reads()
    reads = ws.reads[:8] + extra + ws.reads[8:]
    lens = np.array([len(r) for r in reads])
    assert (lens < 9).any() and (lens < 41).any() and (lens == 93).any() and any(b"N" in r for r in reads)
    codes = [R.store_codes(r) for r in reads]
    c = G.ctx()
    _load(c, reads)
    for k, w in ((25, 17), (16, 8), (6, 4), (30, 64)):
        h, rid, pos, st = c.sketch(k=k, w=w)
        rh, rr, rp, rs = R.sketch_store(codes, k, w)
        assert len(rh) > 2000
        assert h.tolist() == rh.tolist() and rid.tolist() == rr.tolist() and pos.tolist() == rp.tolist() and st.tolist() == rs.tolist(), (k, w)
        assert not (lens[rr] < k + w - 1).any()
        if k % 2 == 0:                                           # k-mers equal to their reverse complement: never selected
            assert sum(int((f == r).sum()) for f, r in (R.kmers(x, k) for x in codes)) >= 20


# ---- finder -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(H.PARAM_SETS)))
def test_overlaps_equal_the_reference_record_for_record(case):
    kw = H.PARAM_SETS[case]
    c = G.ctx()
    ws, codes = _load_working_set(c)
    st = {}
    want = R.find_overlaps(codes, stats=st, **kw)
    assert (st["minimizers"], st["anchors"], len(st["pairs"])) == H.FOUND[case][:3]
    got = c.find_overlaps(**kw)
    _same(got, want)
    assert (got[1][:, 4] == 0).any() and (got[1][:, 4] == 1).any()
    _same(c.find_overlaps(**kw), got)                            # a second run: identical


_CHILD = r"""
import json, os, sys
sys.path.insert(0, os.path.join(sys.argv[1], "tests")); sys.path.insert(0, sys.argv[1])
from herro_amd import api
import test_lowcomplexity_host as H
ws, _ = H.low()
c = api.Context(0)
c.set_reads(ws.seq, ws.qual, ws.off)
out = []
for case in (1, 3):
    rids, rows, off, sc = c.find_overlaps(**H.PARAM_SETS[case])
    out.append({"rids": rids.tolist(), "rows": rows.tolist(), "off": off.tolist(), "sc": sc.tolist()})
print(json.dumps(out))
"""


def test_a_small_scratch_budget_gives_the_same_records():
    """k = 15, w = 5: 35 654 anchors (14 068 at max_occ = 8) in chunks of ~8 000 — the chunk borders run through reads that hold a hash
    several times, and k_mask cuts by target range"""
    ws, codes = H.low()
    env = dict(os.environ, HERRO_OVL_SCRATCH_MB="1")
    p = subprocess.run([sys.executable, "-c", _CHILD, G.ROOT], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    child = json.loads(p.stdout.strip().splitlines()[-1])
    for got, case in zip(child, (1, 3)):
        rids, rows, off, sc = R.find_overlaps(codes, **H.PARAM_SETS[case])
        assert got["rids"] == rids.tolist() and got["off"] == off.tolist() and got["sc"] == sc.tolist() and got["rows"] == rows.tolist(), case


def test_a_query_equal_to_its_reverse_complement_gives_strand_0():
    pal, pcodes = H.palindrome()
    c = G.ctx()
    _load(c, pal)
    for kw in (H.PARAM_SETS[0], H.PARAM_SETS[1]):
        ch = LC.chains(pcodes, **kw)
        assert [x[:3] for x in ch] == [(0, 1, 0), (0, 1, 1)] and ch[0][3] == ch[1][3]        # the reference's two chains tie
        want = R.find_overlaps(pcodes, **kw)
        got = c.find_overlaps(**kw)
        _same(got, want)
        assert got[1][:, 4].tolist() == [0, 0] and got[3].tolist() == [ch[0][3]] * 2


# ---- extension --------------------------------------------------------------------------------------------------------------------------
def _extension_equals(c, codes, rows):
    for kw in PARAMS:
        want = E.extend_records(codes, rows, **kw)
        got = c.extend_overlaps(rows, **kw)
        for name, g, w in zip(("rows", "ext", "scores"), got, want):
            bad = np.flatnonzero((g != w).any(axis=1))
            assert len(bad) == 0, (kw, name, len(bad), int(bad[0]), rows[bad[0]].tolist(), g[bad[0]].tolist(), w[bad[0]].tolist())
            assert g.dtype == w.dtype
    return got


def test_extension_into_related_low_complexity_flanks():
    c = G.ctx()
    ws, codes = _load_working_set(c)
    rows = LC.shrunk_rows(np.random.default_rng(H.SHRINK_SEED), ws)
    assert len(rows) == 248 and set(rows[:, 4].tolist()) == {0, 1}
    _extension_equals(c, codes, rows)
    ext = c.extend_overlaps(rows)[1]
    assert (ext > 0).all(axis=1).sum() >= 100 and ext.max() > 63      # the reads agree again past the shrunk ends, some past the true stretch


def test_extension_into_homopolymer_and_repeat_flanks():
    reads, rows = LC.hand_flank_batch(np.random.default_rng(H.HAND_SEED), LENGTHS)
    assert len(rows) == len(LENGTHS) ** 2 and set(rows[:, 4].tolist()) == {0, 1}
    codes = [R.store_codes(r) for r in reads]
    c = G.ctx()
    _load(c, reads)
    _extension_equals(c, codes, rows)


def test_extension_follows_a_gap_wider_than_half_the_band():
    rd, rows, codes, _ = H.gapped()
    c = G.ctx()
    _load(c, rd)
    _extension_equals(c, codes, rows)


# ---- alignment --------------------------------------------------------------------------------------------------------------------------
def _alignment_equals(c, codes, rows, ref):
    """Context.align against the reference (rows, CIGAR text, score, ok) and every CIGAR valid; then the same records through
    align_overlaps_dev: the handle's ops are the text's"""
    out, cig, sc, ok = c.align(rows)
    r_out, r_cig, r_sc, r_ok, _ = ref
    bad = [i for i in range(len(rows)) if not (cig[i] == r_cig[i] and np.array_equal(out[i], r_out[i]) and int(sc[i]) == int(r_sc[i])
                                               and bool(ok[i]) == bool(r_ok[i]))]
    assert not bad, [(i, rows[i].tolist(), cig[i][:80], r_cig[i][:80], int(sc[i]), int(r_sc[i])) for i in bad[:5]]
    for r in np.flatnonzero(ok):
        ops = A.parse_cigar(cig[r])
        assert all(ln > 0 for ln, _ in ops), r
        assert all(a[1] != b[1] for a, b in zip(ops, ops[1:])), r
        assert ops[0][1] == A.M_ and ops[-1][1] == A.M_, r
        assert cig[r].decode().strip("0123456789MID") == ""
        T, Q = A.record_seqs(codes, out[r])
        assert A.score_cigar(ops, T, Q) == sc[r], r
        assert out[r, 9] == len(cig[r])
    for r in np.flatnonzero(~ok):
        assert cig[r] == b"" and sc[r] == np.iinfo(np.int32).min and np.array_equal(out[r, :9], rows[r, :9])
    h = c.align_dev(rows)
    assert h.n == len(rows) and h.failed == int((~ok).sum())
    assert np.array_equal(h.rows[:, :9], out[:, :9]) and np.array_equal(h.scores, sc) and np.array_equal(h.ok, ok)
    assert [h.cigar(r) for r in range(h.n)] == cig
    assert h.n_ops.tolist() == [len(AC.cigar_ops(x)) for x in cig]
    return out, cig, ok, h


def _job_equals_the_text_paths(c, h, out, cig, ok, W, tag):
    """a job from create_job_aligned against the job from the texts: the records grouped by target in the order given"""
    tid = out[:, 5].astype(np.int64)
    assert (np.diff(tid) >= 0).all()
    rids, counts = np.unique(tid, return_counts=True)
    aln_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    j_rids, off2, rec = api.aligned_dev_job_args(rids.astype(np.uint32), aln_off, ok)
    ja = c.create_job_aligned(j_rids, off2, rec, h, W)
    jt = c.create_job(j_rids, out[rec], off2, [cig[int(r)] for r in rec], W)
    try:
        a, _ = AC.same_jobs(c, ja, jt, tag)
        assert len(a["ow"]) > 0
    finally:
        ja.close(); jt.close()


def test_alignment_of_the_lopsided_grid():
    rd, rows, kinds, codes = H.grid()
    ref, _, _ = H.grid_aligned()
    assert LC.grid_net_indel_above(rows) == 208 and ref[3].all()
    c = G.ctx()
    _load(c, rd)
    out, cig, ok, h = _alignment_equals(c, codes, rows, ref)
    try:
        assert sum(1 for x in cig if len(A.parse_cigar(x)) == 1 and A.parse_cigar(x)[0][0] <= 2) >= 20     # one or two matches, the rest trimmed
        _job_equals_the_text_paths(c, h, out, cig, ok, AC.HAND_W, "grid")
    finally:
        h.close()


def test_alignment_across_a_gap_wider_than_half_the_band():
    rd, rows, codes, ref = H.gapped()
    c = G.ctx()
    _load(c, rd)
    out, cig, ok, h = _alignment_equals(c, codes, LC.whole_rows(rows), ref)
    h.close()
    assert ok.all()


def test_alignment_of_the_working_sets_true_pairs():
    c = G.ctx()
    ws, codes = _load_working_set(c)
    rows = LC.true_rows(ws)
    ref, _, n_indels = H.low_aligned()
    assert len(rows) == 62 and n_indels == H.SHIFTED[1][1]
    out, cig, ok, h = _alignment_equals(c, codes, rows, ref)
    try:
        assert ok.all()
        _job_equals_the_text_paths(c, h, out, cig, ok, 256, "true pairs")
    finally:
        h.close()


# ---- the whole path ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,batch_mode", [(256, 0), (1024, 1)])
def test_reads_to_fasta_on_low_complexity_reads(W, batch_mode):
    c = G.ctx()
    ws, codes = _load_working_set(c)
    rids, rows, aln_off, _ = c.find_overlaps(max_occ=64, min_score=100)
    rows_e, ext, _ = c.extend_overlaps(rows)
    assert ext.sum() > 0
    h = c.align_dev(rows_e)
    failed = h.failed
    j_rids, off2, rec = api.aligned_dev_job_args(rids, aln_off, h.ok)
    job = c.create_job_aligned(j_rids, off2, rec, h, W)
    rows2 = h.rows[rec]
    cig2 = [h.cigar(int(r)) for r in rec]
    h.close()
    n_ins = sum(x.count(b"I") for x in cig2)
    print(dict(W=W, records=len(rows), failed=failed, insertions=n_ins, windows=job.n_windows))
    assert failed == 0 and len(rows2) == len(rows) == 150 and n_ins >= 1000
    job.featurize()
    # the oracle fed the GPU's rows and CIGARs
    blob = b"".join(cig2)
    lens = np.array([len(x) for x in cig2], np.uint64)
    rows10 = rows2.astype(np.uint32).copy()
    rows10[:, 9] = lens
    sb = synth.SynthBatch(seq=ws.seq, qual=ws.qual, off=ws.off, aln=rows10, cig=np.frombuffer(blob + b"\0", np.uint8).copy(),
                          cig_off=np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64), tgt_aln_off=off2, tgt_rid=j_rids)
    store = G.O.store_from_synth(sb)
    assert G.compare_features(job, sb, store, W) > 0
    job.infer(64, batch_mode)
    job.consensus()
    w = n_fasta = 0
    for t in range(sb.n_targets):
        rid, orows, ocigs = G.O.target_alignments(sb, t)
        res = store.extract_features(rid, orows, ocigs, W)
        lg = [job.logits(w + wi)[1] for wi in range(len(res)) if job.info(w + wi).n_supported]
        w += len(res)
        lg = np.concatenate(lg) if lg else np.zeros((0, 5), np.float32)
        got = job.consensus_fasta(t, sb.read_name(rid))
        assert got == res.consensus_fasta(lg), f"FASTA mismatch, target {t}"
        n_fasta += got.count(">")
    assert n_fasta >= 1
    job.close()
