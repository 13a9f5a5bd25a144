"""gpu: herro_find_overlaps (csrc/overlap_dev.hip) — minimizer seeding and chaining on the resident read store — against its
numpy restatement (tests/overlap_ref.py) record for record, the recall / span conditions of tests/test_overlap_host.py on the
GPU's output, the scratch budget, and the whole path without any overlap input: find -> align -> create_job -> featurize ->
infer -> consensus -> FASTA against the oracle fed the same rows and CIGARs."""
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gpu_common as G  # noqa: E402
import overlap_ref as R  # noqa: E402
from test_overlap_host import SETS, evaluate  # noqa: E402
from herro_amd import api, synth  # noqa: E402

pytestmark = pytest.mark.gpu

_CACHE = {}


def _codes(sb):
    return [R.store_codes(sb.read_seq(i)) for i in range(sb.n_reads)]


def _batch():
    """32 groups of 13 reads at 4096 bp (both strands, partial overlaps, 0.5 .. 8 % error, long indels) and one of 9 reads >= 30 kb"""
    if "b" not in _CACHE:
        sb = synth.merge([
            synth.generate(10, 4096, 12, seed=51, p_partial=0.3, min_partial_len=1024),                              # ~1.6 % error
            synth.generate(6, 4096, 12, seed=52, p_sub=0.01, p_ins=0.01, p_del=0.01, p_partial=0.3),                 # 3 %
            synth.generate(4, 4096, 12, seed=53, p_sub=0.03, p_ins=0.025, p_del=0.025, p_partial=0.2),               # 8 %
            synth.generate(6, 4096, 12, seed=54, p_sub=0.002, p_ins=0.0015, p_del=0.0015),                           # 0.5 %
            synth.generate(6, 4096, 12, seed=55, p_long_indel=0.003, p_partial=0.2),                                 # long indels
            synth.generate(1, 30000, 8, seed=56, flank_min=200, flank_max=400),                                      # >= 30 kb
        ])
        _CACHE["b"] = (sb, _codes(sb))
    return _CACHE["b"]


def _same(got, want):
    g_rids, g_rows, g_off, g_sc = got
    r_rids, r_rows, r_off, r_sc = want
    assert g_rids.tolist() == r_rids.tolist()
    assert g_off.tolist() == r_off.tolist()
    bad = [i for i in range(min(len(g_rows), len(r_rows))) if not np.array_equal(g_rows[i], r_rows[i]) or int(g_sc[i]) != int(r_sc[i])]
    assert not bad and len(g_rows) == len(r_rows), (len(g_rows), len(r_rows), [(i, g_rows[i].tolist(), int(g_sc[i]), r_rows[i].tolist(), int(r_sc[i])) for i in bad[:5]])
    assert g_rows.dtype == np.uint32 and g_rows.shape[1] == 10 and (g_rows[:, 9] == 0).all()


def test_sketch_equals_the_reference():
    sb = synth.merge([
        synth.generate(3, 2048, 6, seed=61, p_n_base=0.002, p_partial=0.3),
        synth.generate(2, 40, 4, seed=62, flank_min=0, flank_max=6),          # reads around k + w - 1 = 41 bases, all below 94
        synth.generate(1, 9000, 3, seed=63, p_n_base=0.0005),
    ])
    lens = np.diff(sb.off.astype(np.int64))
    assert (lens < 41).any() and (lens >= 41).any() and (lens < 19).sum() < len(lens)
    assert any(set(sb.read_seq(i)) - set(b"ACGT") for i in range(sb.n_reads))
    codes = _codes(sb)
    c = G.ctx()
    G.load_synth(c, sb)
    for k, w in ((25, 17), (15, 5), (31, 64)):
        h, rid, pos, st = c.sketch(k=k, w=w)
        rh, rr, rp, rs = R.sketch_store(codes, k, w)
        assert len(rh) > 100
        assert h.tolist() == rh.tolist() and rid.tolist() == rr.tolist() and pos.tolist() == rp.tolist() and st.tolist() == rs.tolist(), (k, w)
        assert set(rr[lens[rr] < k + w - 1].tolist()) == set()
    h0 = c.sketch()                                                             # the defaults are k = 25, w = 17
    assert h0[0].tolist() == R.sketch_store(codes, 25, 17)[0].tolist()


def test_overlaps_equal_the_reference_record_for_record():
    sb, codes = _batch()
    c = G.ctx()
    G.load_synth(c, sb)
    got = c.find_overlaps(max_occ=64, min_score=100)
    st = {}
    want = R.find_overlaps(codes, max_occ=64, min_score=100, stats=st)
    print(json.dumps({"records": len(want[1]), "anchors": st["anchors"], "minimizers": st["minimizers"]}))
    assert len(want[1]) >= 2 * 2000
    _same(got, want)
    rows = got[1]
    assert (rows[:, 4] == 0).any() and (rows[:, 4] == 1).any()
    assert (rows[:, 8] - rows[:, 7]).max() >= 25000                            # the >= 30 kb group
    _same(c.find_overlaps(max_occ=64, min_score=100), got)                      # a second run: identical
    _CACHE["found"] = got
    # other parameters: k = 15, w = 5 and a narrow band / short gap
    _same(c.find_overlaps(k=15, w=5, max_occ=64, min_score=60, bandwidth=20, max_gap=300, min_anchors=5),
          R.find_overlaps(codes, k=15, w=5, max_occ=64, min_score=60, bandwidth=20, max_gap=300, min_anchors=5))


def test_max_occ_must_stay_above_the_read_depth():
    """33 reads deep: max_occ = 24 cuts true minimizers (67 165 of 75 617 anchors stay) and still finds all 528 pairs"""
    sb = synth.generate(1, 2048, 32, seed=31)
    codes = _codes(sb)
    c = G.ctx()
    G.load_synth(c, sb)
    full, cut = {}, {}
    R.find_overlaps(codes, max_occ=128, min_score=100, stats=full)
    want = R.find_overlaps(codes, max_occ=24, min_score=100, stats=cut)
    assert (full["anchors"], cut["anchors"]) == (75617, 67165)
    assert len(cut["pairs"]) == 528 == 33 * 32 // 2
    _same(c.find_overlaps(max_occ=24, min_score=100), want)
    _same(c.find_overlaps(max_occ=16, min_score=100), R.find_overlaps(codes, max_occ=16, min_score=100))


def _tandem_pair():
    """2 400 random bp + a 40-bp unit x 30 + 2 400 random bp, two copies with 1 % substitutions each"""
    rng = np.random.default_rng(5)
    u = rng.integers(0, 4, 40)
    g = np.concatenate([rng.integers(0, 4, 2400), np.tile(u, 30), rng.integers(0, 4, 2400)])
    reads = []
    for i in range(2):
        r = g.copy()
        m = rng.random(len(r)) < 0.01
        r[m] = (r[m] + rng.integers(1, 4, m.sum())) & 3
        reads.append(bytes(b"ACGT"[x] for x in r))
    return reads


def test_the_lookback_limit_is_the_kernels_too():
    """A tandem repeat that survives the frequency cut puts more than 64 off-diagonal anchors between two anchors of the true
    diagonal: the chain with the look-back of 64 scores less than an unlimited one — and the kernel gives the former."""
    reads = _tandem_pair()
    codes = [R.store_codes(r) for r in reads]
    kw = dict(k=15, w=5, max_occ=4096, min_score=100)
    s64, sinf = {}, {}
    want = R.find_overlaps(codes, stats=s64, **kw)
    R.find_overlaps(codes, lookback=None, stats=sinf, **kw)
    a, b = s64["pairs"][(0, 1)], sinf["pairs"][(0, 1)]
    print(json.dumps({"anchors": s64["anchors"], "lookback 64": a[:1] + a[6:], "unlimited": b[:1] + b[6:]}))
    assert s64["anchors"] > 5000 and a[0] < b[0] and a[6] < b[6]
    seq = np.frombuffer(b"".join(reads), np.uint8)
    off = np.array([0, len(reads[0]), len(reads[0]) + len(reads[1])], np.uint64)
    c = G.ctx()
    c.set_reads(seq, np.full(len(seq), 40 + 33, np.uint8), off)
    _same(c.find_overlaps(**kw), want)


_CHILD = r"""
import json, os, sys
sys.path.insert(0, os.path.join(sys.argv[1], "tests")); sys.path.insert(0, sys.argv[1])
import numpy as np
from herro_amd import api, synth
import test_gpu_overlap as T
sb, _ = T._batch()
c = api.Context(0)
c.set_reads(sb.seq, sb.qual, sb.off)
rids, rows, off, sc = c.find_overlaps(max_occ=64, min_score=100)
print(json.dumps({"rids": rids.tolist(), "rows": rows.tolist(), "off": off.tolist(), "sc": sc.tolist()}))
"""


def test_scratch_budget_and_errors():
    sb, codes = _batch()
    c = G.ctx()
    if "found" not in _CACHE:
        G.load_synth(c, sb)
        _CACHE["found"] = c.find_overlaps(max_occ=64, min_score=100)
    rids, rows, off, sc = _CACHE["found"]
    env = dict(os.environ, HERRO_OVL_SCRATCH_MB="1")      # ~8 000 anchors per chunk: dozens of read-id ranges
    p = subprocess.run([sys.executable, "-c", _CHILD, G.ROOT], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    child = json.loads(p.stdout.strip().splitlines()[-1])
    assert child["rids"] == rids.tolist() and child["off"] == off.tolist() and child["sc"] == sc.tolist()
    assert child["rows"] == rows.tolist()
    # errors
    fresh = api.Context(0)
    for call in (fresh.find_overlaps, fresh.sketch):
        with pytest.raises(api.HerroError) as e:
            call()
        assert e.value.code == -6                          # HERRO_E_STATE: no reads
    for bad in (dict(k=32), dict(w=0), dict(w=65), dict(k=4)):
        with pytest.raises(api.HerroError) as e:
            fresh.find_overlaps(**bad)
        assert e.value.code == -1, bad                     # HERRO_E_INVALID before anything else
    import ctypes as C
    h = C.c_void_p()
    p32 = api.OverlapParams(k=32)
    assert api.lib().herro_find_overlaps(c.h, C.byref(p32), C.byref(h)) == -1
    fresh.close()
    # a store without any overlap, and one without any minimizer
    lone = synth.generate(1, 300, 1, seed=71, flank_min=0, flank_max=4)
    c.set_reads(lone.seq[:int(lone.off[1])], lone.qual[:int(lone.off[1])], lone.off[:2])
    r = c.find_overlaps(min_score=100)
    assert len(r[0]) == 0 and r[1].shape == (0, 10) and r[2].tolist() == [0] and len(r[3]) == 0
    c.set_reads(lone.seq[:30], lone.qual[:30], np.array([0, 30], np.uint64))
    assert len(c.sketch()[0]) == 0 and len(c.find_overlaps()[1]) == 0


@pytest.mark.parametrize("case", range(len(SETS)))
def test_recall_and_span_of_the_gpu_output(case):
    kw, (k, w), least = SETS[case]
    sb = synth.generate(**kw)
    c = G.ctx()
    G.load_synth(c, sb)
    rids, rows, off, sc = c.find_overlaps(k=k, w=w, max_occ=64, min_score=100)
    pairs = {}
    for r, s in zip(rows.tolist(), sc.tolist()):
        qid, qlen, qs, qe, strand, tid, tlen, ts, te, _ = r
        if tid < qid:
            pairs[(tid, qid)] = (s, strand, ts, te, qs, qe)
    assert 2 * len(pairs) == len(rows)
    miss, wrong, cross, cov = evaluate(sb, pairs)
    print(json.dumps({"case": case, "pairs": len(pairs), "missed": miss, "wrong_strand": wrong, "cross_group": cross, "min_coverage": cov}))
    assert (miss, wrong, cross) == (0, 0, 0)
    assert cov >= least


@pytest.mark.parametrize("W,batch_mode", [(256, 0), (4096, 1)])
def test_end_to_end_without_any_overlap_input(W, batch_mode):
    sb = synth.generate(3, 8192, 8, seed=81 + W, p_partial=0.2)
    c = G.ctx()
    G.load_synth(c, sb)
    rids, rows, aln_off, sc = c.find_overlaps(max_occ=64, min_score=200)
    assert set(sb.tgt_rid.tolist()) <= set(rids.tolist())                      # every target of the synthetic set ...
    assert rids.tolist() == list(range(sb.n_reads))                             # ... and every other read of a group: the queries overlap each other
    out, cig, asc, ok = c.align(rows)
    failed = [(rows[i].tolist(), int(sc[i])) for i in np.flatnonzero(~ok)]
    assert not failed, failed[:5]                                               # an anchor span begins and ends on an exact k-mer match
    j_rids, rows2, off2, cig2 = api.aligned_job_args(rids, aln_off, out, cig, ok)
    assert np.array_equal(j_rids, rids) and off2.tolist() == aln_off.tolist()
    job = c.create_job(j_rids, rows2, off2, cig2, W)
    assert job.skipped() == (0, 0)
    job.featurize()
    blob = b"".join(cig2)
    lens = np.array([len(x) for x in cig2], np.uint64)
    sb2 = dataclasses.replace(sb, aln=rows2.astype(np.uint32), cig=np.frombuffer(blob + b"\0", np.uint8).copy(),
                              cig_off=np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64), tgt_aln_off=off2, tgt_rid=j_rids)
    store = G.O.store_from_synth(sb2)
    assert G.compare_features(job, sb2, store, W) > 0
    job.infer(64, batch_mode)
    job.consensus()
    w = 0
    for t in range(sb2.n_targets):
        rid, orows, ocigs = G.O.target_alignments(sb2, t)
        res = store.extract_features(rid, orows, ocigs, W)
        lg = []
        for wi in range(len(res)):
            if job.info(w + wi).n_supported:
                lg.append(job.logits(w + wi)[1])
        w += len(res)
        lg = np.concatenate(lg) if lg else np.zeros((0, 5), np.float32)
        assert job.consensus_fasta(t, sb.read_name(rid)) == res.consensus_fasta(lg), f"FASTA mismatch, target {t}"
    job.close()
