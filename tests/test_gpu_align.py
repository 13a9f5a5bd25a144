"""gpu: herro_align_overlaps (csrc/align_dev.hip) — the base-level alignment of overlaps given by coordinates only — against its
numpy restatement (tests/align_ref.py) bit for bit, the validity of every CIGAR, its quality against the generator's true
alignments, the path align -> create_job -> featurize -> infer -> consensus -> FASTA against the oracle fed the same CIGARs,
chunking of the scratch and the error codes."""
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import align_ref as A  # noqa: E402
import gpu_common as G  # noqa: E402
from herro_amd import api, synth  # noqa: E402

pytestmark = pytest.mark.gpu

_CACHE = {}


def _batch():
    """> 5 000 records: both strands and partial overlaps, 0.5 .. 8 % error, long indels, ~30 kb overlaps, records of a handful of
    bases and records that fail (one side empty)."""
    if "b" in _CACHE:
        return _CACHE["b"]
    parts = [
        synth.generate(64, 1024, 32, seed=11, p_partial=0.3, min_partial_len=64),                                   # ~1.6 % error
        synth.generate(16, 1024, 32, seed=17, p_sub=0.01, p_ins=0.01, p_del=0.01, p_partial=0.3),                   # 3 %
        synth.generate(20, 1024, 32, seed=12, p_sub=0.03, p_ins=0.025, p_del=0.025, p_partial=0.2),                 # 8 %
        synth.generate(20, 1024, 32, seed=13, p_sub=0.002, p_ins=0.0015, p_del=0.0015),                             # 0.5 %
        synth.generate(20, 1024, 32, seed=14, p_long_indel=0.003, p_partial=0.2),                                   # long indels
        synth.generate(2, 30000, 8, seed=15, flank_min=200, flank_max=400),                                          # >= 30 kb
    ]
    sb = synth.merge(parts)
    rows = sb.aln[:, :9].copy()
    rng = np.random.default_rng(16)
    extra = []
    for a in rng.choice(len(rows), 800, replace=False):   # sub-regions of a handful of bases (the same offsets on both reads)
        r = rows[a].copy()
        span = int(min(r[3] - r[2], r[8] - r[7]))
        ln = int(rng.integers(1, 40))
        if span <= ln:
            continue
        o = int(rng.integers(0, span - ln))
        if r[4] == 0:
            r[2], r[3] = r[2] + o, r[2] + o + ln
        else:
            r[3], r[2] = r[3] - o, r[3] - o - ln
        r[7], r[8] = r[7] + o, r[7] + o + ln + int(rng.integers(0, 3))
        extra.append(r)
    for a in rng.choice(len(rows), 40, replace=False):    # one side empty: nothing but an indel, which the trim drops
        r = rows[a].copy()
        if a % 2:
            r[3] = r[2]
        else:
            r[8] = r[7]
        extra.append(r)
    allrows = np.concatenate([rows, np.array(extra, np.uint32)])
    codes = [A.store_codes(sb.read_seq(i)) for i in range(sb.n_reads)]
    _CACHE["b"] = (sb, allrows, codes)
    return _CACHE["b"]


def _reference():
    if "ref" not in _CACHE:
        sb, rows, codes = _batch()
        _CACHE["ref"] = A.align_records(codes, rows)
    return _CACHE["ref"]


def _gpu(c, sb, rows):
    G.load_synth(c, sb)
    return c.align(rows)


def test_bit_exact_against_the_reference():
    sb, rows, codes = _batch()
    assert len(rows) >= 5000
    c = G.ctx()
    out, cig, sc, ok = _gpu(c, sb, rows)
    r_out, r_cig, r_sc, r_ok, _ = _reference()
    assert r_ok.sum() > 4500 and (~r_ok).sum() >= 40
    bad = [i for i in range(len(rows)) if not (cig[i] == r_cig[i] and np.array_equal(out[i], r_out[i]) and int(sc[i]) == int(r_sc[i])
                                               and bool(ok[i]) == bool(r_ok[i]))]
    assert not bad, [(i, rows[i].tolist(), cig[i][:80], r_cig[i][:80], int(sc[i]), int(r_sc[i])) for i in bad[:5]]
    D = (rows[:, 3] - rows[:, 2]).astype(np.int64) + (rows[:, 8] - rows[:, 7])
    assert D.max() >= 60000 and (D[ok] <= 12).any()


def test_every_cigar_is_valid():
    sb, rows, codes = _batch()
    c = G.ctx()
    out, cig, sc, ok = _gpu(c, sb, rows)
    for r in np.flatnonzero(ok):
        ops = A.parse_cigar(cig[r])
        assert all(ln > 0 for ln, _ in ops), r
        assert all(a[1] != b[1] for a, b in zip(ops, ops[1:])), r
        assert ops[0][1] == A.M_ and ops[-1][1] == A.M_, r
        assert cig[r].decode().strip("0123456789MID") == ""
        T, Q = A.record_seqs(codes, out[r])
        assert A.score_cigar(ops, T, Q) == sc[r], r      # consumes exactly the trimmed regions and re-scores to the reported score
        assert out[r, 9] == len(cig[r])
    for r in np.flatnonzero(~ok):
        assert cig[r] == b"" and sc[r] == np.iinfo(np.int32).min and np.array_equal(out[r, :9], rows[r, :9])


def _columns(ops, n, q0, t0):
    """target column of every query base (Q orientation) under ops starting at (t0, q0); -1: inserted or outside"""
    col = np.full(n, -1, np.int64)
    t, q = t0, q0
    for ln, ty in ops:
        if ty == A.M_:
            col[q:q + ln] = np.arange(t, t + ln)
            t += ln
            q += ln
        elif ty == A.I_:
            q += ln
        else:
            t += ln
    return col


def test_quality_against_the_true_alignments():
    """At ~1 % substitutions / insertions / deletions: >= 99 % of records score at least the truth, >= 99 % of query bases land in the
    truth's target column once the truth went through the same fix_cigar."""
    sb = synth.generate(24, 2048, 32, seed=21, p_sub=0.0033, p_ins=0.0033, p_del=0.0034)
    rows = sb.aln[:, :9]
    codes = [A.store_codes(sb.read_seq(i)) for i in range(sb.n_reads)]
    c = G.ctx()
    out, cig, sc, ok = _gpu(c, sb, rows)
    better = same = total = 0
    for r in range(len(rows)):
        T, Q = A.record_seqs(codes, rows[r])
        truth = A.parse_cigar(sb.cigar(r))
        t_sc = A.score_cigar(truth, T, Q)
        fixed, tsh, qsh = A.fix_cigar(truth, T, Q)
        want = _columns(fixed, len(Q), qsh, tsh)
        if ok[r]:
            better += int(sc[r]) + _dropped(rows[r], out[r]) >= t_sc      # both on the untrimmed regions
            q0 = int(out[r, 2] - rows[r, 2]) if rows[r, 4] == 0 else int(rows[r, 3] - out[r, 3])
            got = _columns(A.parse_cigar(cig[r]), len(Q), q0, int(out[r, 7] - rows[r, 7]))
        else:
            got = np.full(len(Q), -1, np.int64)
        same += int((got == want).sum())
        total += len(Q)
    frac_rec, frac_base = better / len(rows), same / total
    print(json.dumps({"records": len(rows), "score_ge_truth": frac_rec, "bases_in_truth_column": frac_base}))
    assert frac_rec >= 0.99 and frac_base >= 0.99, (frac_rec, frac_base)


def _dropped(row_in, row_out):
    """gap cost of what the trim dropped (the truth is scored on the untrimmed regions)"""
    cost = 0
    for d in (int(row_out[7] - row_in[7]), int(row_in[8] - row_out[8]), int(row_out[2] - row_in[2]), int(row_in[3] - row_out[3])):
        if d:
            cost -= A.GAP_OPEN + A.GAP_EXT * d
    return cost


@pytest.mark.parametrize("W,batch_mode", [(256, 0), (4096, 1)])
def test_end_to_end_on_gpu_made_cigars(W, batch_mode):
    sb = synth.generate(4, 8192, 16, seed=31 + W, p_partial=0.2)
    c = G.ctx()
    fastas = []
    for run in range(2):
        out, cig, sc, ok = _gpu(c, sb, sb.aln[:, :9])
        rids, rows2, off2, cig2 = api.aligned_job_args(sb.tgt_rid, sb.tgt_aln_off, out, cig, ok)
        assert ok.all()
        job = c.create_job(rids, rows2, off2, cig2, W)
        job.featurize()
        # the oracle on a batch whose rows and CIGARs are the GPU's
        blob = b"".join(cig2)
        lens = np.array([len(x) for x in cig2], np.uint64)
        sb2 = dataclasses.replace(sb, aln=rows2.astype(np.uint32), cig=np.frombuffer(blob, np.uint8).copy(),
                                  cig_off=np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64), tgt_aln_off=off2)
        store = G.O.store_from_synth(sb2)
        if run == 0:
            assert G.compare_features(job, sb2, store, W) > 0
        job.infer(64, batch_mode)
        job.consensus()
        text = []
        w = 0
        for t in range(sb.n_targets):
            rid, orows, ocigs = G.O.target_alignments(sb2, t)
            res = store.extract_features(rid, orows, ocigs, W)
            lg = []
            for wi in range(len(res)):
                if job.info(w + wi).n_supported:
                    lg.append(job.logits(w + wi)[1])
            w += len(res)
            lg = np.concatenate(lg) if lg else np.zeros((0, 5), np.float32)
            got = job.consensus_fasta(t, sb.read_name(rid))
            if run == 0:
                assert got == res.consensus_fasta(lg), f"FASTA mismatch, target {t}"
            text.append(got)
        fastas.append(("".join(text), cig))
        job.close()
    assert fastas[0] == fastas[1]


_CHILD = r"""
import json, os, sys
sys.path.insert(0, os.path.join(sys.argv[1], "tests")); sys.path.insert(0, sys.argv[1])
import numpy as np
from herro_amd import api, synth
sb = synth.generate(6, 4096, 16, seed=41, p_partial=0.3)
c = api.Context(0)
c.set_reads(sb.seq, sb.qual, sb.off)
out, cig, sc, ok = c.align(sb.aln[:, :9])
print(json.dumps({"out": out.tolist(), "cig": [x.decode() for x in cig], "sc": sc.tolist()}))
"""


def test_chunking_and_errors():
    env = dict(os.environ, HERRO_ALIGN_SCRATCH_MB="1")
    p = subprocess.run([sys.executable, "-c", _CHILD, G.ROOT], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    child = json.loads(p.stdout.strip().splitlines()[-1])
    sb = synth.generate(6, 4096, 16, seed=41, p_partial=0.3)
    c = G.ctx()
    out, cig, sc, ok = _gpu(c, sb, sb.aln[:, :9])
    assert child["out"] == out.tolist() and child["cig"] == [x.decode() for x in cig] and child["sc"] == sc.tolist()
    # errors
    fresh = api.Context(0)
    with pytest.raises(api.HerroError) as e:
        fresh.align(sb.aln[:4, :9])
    assert e.value.code == -6
    fresh.close()
    bad = sb.aln[:3, :9].copy()
    bad[1, 3] = bad[1, 1] + 5          # qend past the read
    with pytest.raises(api.HerroError) as e:
        c.align(bad)
    assert e.value.code == -1 and "record 1" in str(e.value)
    bad = sb.aln[:3, :9].copy()
    bad[2, 5] = sb.n_reads + 3         # target outside the store
    with pytest.raises(api.HerroError) as e:
        c.align(bad)
    assert e.value.code == -1 and "record 2" in str(e.value)
