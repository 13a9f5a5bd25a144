"""gpu: herro_aligned_dev_mirror (k_mirror, csrc/align_dev.hip; DESIGN.md §9, "Mirrored records") bit for bit against tests/mirror_ref.py
— on hand cases and op counts around the 64-lane wave through herro_aligned_dev_from_ops, on the aligner's own handles (random reads,
low-complexity pairs, the lopsided grid), and as a pipeline step: reads -> FASTA with one alignment per read pair, against the oracle."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import align_ref as A  # noqa: E402
import frontend_cases as FC  # noqa: E402
import gpu_common as G  # noqa: E402
import lowcomplexity as LC  # noqa: E402
import mirror_cases as MC  # noqa: E402
import mirror_ref as MR  # noqa: E402
import test_lowcomplexity_host as H  # noqa: E402
from herro_amd import api, synth  # noqa: E402

pytestmark = pytest.mark.gpu

INT32_MIN = -(1 << 31)


def _equals_the_reference(h, m, codes, tag):
    """m = h.mirror(): records [0, n) are h's, records [n, 2n) what mirror_ref makes of h's own rows, CIGARs and scores; every
    mirrored CIGAR consumes its two spans and scores what the handle says.  Returns everything compared, as bytes-comparable lists."""
    n = h.n
    assert m.n == 2 * n, tag
    src_cig = MC.handle_ops(h)
    got_cig = MC.handle_ops(m)
    assert np.array_equal(m.rows[:n], h.rows) and np.array_equal(m.scores[:n], h.scores) and np.array_equal(m.n_ops[:n], h.n_ops), tag
    assert got_cig[:n] == src_cig, tag
    w_rows, w_cig, w_sc, w_ok = MR.mirror_records(codes, h.rows, src_cig, h.scores)
    bad = [r for r in range(n) if not (got_cig[n + r] == w_cig[r] and np.array_equal(m.rows[n + r], w_rows[r]) and int(m.scores[n + r]) == int(w_sc[r])
                                       and bool(m.ok[n + r]) == bool(w_ok[r]))]
    assert not bad, (tag, [(r, h.rows[r].tolist(), src_cig[r][:60], got_cig[n + r][:60], w_cig[r][:60], m.rows[n + r].tolist(), w_rows[r].tolist(),
                            int(m.scores[n + r]), int(w_sc[r])) for r in bad[:4]])
    assert m.n_ops[n:].tolist() == [len(A.parse_cigar(x)) for x in w_cig], tag
    assert m.failed == h.failed + int((~w_ok).sum()) and not m.rows[:, 9].any(), tag
    for r in np.flatnonzero(w_ok):
        T, Q = A.record_seqs(codes, m.rows[n + r])
        assert A.score_cigar(A.parse_cigar(got_cig[n + r]), T, Q) == int(m.scores[n + r]) - int(h.scores[r]) + _score(codes, h, r, src_cig), (tag, r)
    return [m.rows.tolist(), m.scores.tolist(), m.n_ops.tolist(), got_cig]


def _score(codes, h, r, src_cig):
    T, Q = A.record_seqs(codes, h.rows[r])
    return A.score_cigar(A.parse_cigar(src_cig[r]), T, Q)


# ---- 1. caller-supplied ops: the hand cases and the op counts ------------------------------------------------------------------------------
def test_hand_cases_and_op_counts_from_caller_supplied_ops():
    names, reads, rows, off, ops, want = MC.hand()
    counted = MC.counted(np.random.default_rng(21))
    r2, rows2, off2, ops2 = MC.build(counted)
    rows2 = rows2.copy()
    rows2[:, [0, 5]] += len(reads)
    all_reads = reads + r2
    all_rows = np.concatenate([rows, rows2])
    all_off = np.concatenate([off, off2[1:] + off[-1]])
    all_ops = np.concatenate([ops, ops2])
    assert sorted(set(np.diff(off2).astype(int).tolist())) == [1, 2, 3, 63, 64, 65, 201] and set(rows2[:, 4].tolist()) == {0, 1}
    codes = [A.store_codes(r) for r in all_reads]
    c = G.ctx()
    c.set_reads(*MC.store(all_reads))
    h = c.aligned_dev_from_ops(all_rows, all_off, all_ops)
    n = h.n
    type3 = names.index("type_3")
    runs = []
    for run in range(2):
        m = h.mirror()
        try:
            # the hand cases: the CIGARs written out (type 3 has no text for mirror_ref to parse: judged here alone)
            got = MC.handle_ops(m)
            for i, name in enumerate(names):
                w_row, w_cig = want[i]
                assert m.rows[n + i, :9].tolist() == w_row.tolist(), name
                assert got[n + i] == (w_cig or b"") and bool(m.ok[n + i]) == (w_cig is not None), (name, got[n + i])
                if w_cig is None:
                    assert m.scores[n + i] == INT32_MIN and m.n_ops[n + i] == 0, name
            assert got[type3] == b"5M1?5M" and not m.ok[n + type3]
            # everything but the type-3 record against the reference
            keep = np.array([r for r in range(n) if r != type3])
            src_cig = MC.handle_ops(h)
            w_rows, w_cig, w_sc, w_ok = MR.mirror_records(codes, h.rows[keep], [src_cig[r] for r in keep], h.scores[keep])
            for k, r in enumerate(keep):
                assert got[n + r] == w_cig[k] and m.rows[n + r].tolist() == w_rows[k].tolist() and int(m.scores[n + r]) == int(w_sc[k]) \
                    and bool(m.ok[n + r]) == bool(w_ok[k]), (r, got[n + r][:80], w_cig[k][:80])
            assert got[:n] == src_cig and np.array_equal(m.rows[:n], h.rows) and np.array_equal(m.n_ops[:n], h.n_ops)
            assert m.failed == h.failed + int((~w_ok).sum()) + 1
            moved = sum(1 for k, r in enumerate(keep) if r >= len(names) and w_cig[k] != A.cigar_text(MR.mirror_ops(A.parse_cigar(src_cig[r]), int(h.rows[r, 4]))))
            assert moved >= 8                                              # the two-letter reads make the shift run at every op count
            runs.append([m.rows.tolist(), m.scores.tolist(), m.n_ops.tolist(), got])
        finally:
            m.close()
    h.close()
    assert runs[0] == runs[1]


def test_records_past_one_slice_equal_the_reference():
    """The host sends the records through in slices (SLICE of frontend_api.hip): 37 records more than one slice, so the loop turns
    twice and the second turn is a short one.  Six records of one to three ops, tiled (about two million ops in the store)."""
    reads, rows, off, ops = MC.build(MC.counted(np.random.default_rng(22), counts=(1, 2, 3)))
    codes = [A.store_codes(r) for r in reads]
    k = len(rows)
    cnt = np.diff(off).astype(np.int64)
    assert k == 6 and sorted(set(cnt.tolist())) == [1, 2, 3] and set(rows[:, 4].tolist()) == {0, 1}
    c = G.ctx()
    c.set_reads(*MC.store(reads))
    h0 = c.aligned_dev_from_ops(rows, off, ops)                        # the untiled records: their CIGAR texts for the reference
    src_cig = MC.handle_ops(h0)
    w_rows, w_cig, w_sc, w_ok = MR.mirror_records(codes, h0.rows, src_cig, h0.scores)
    src_rows, src_scores = h0.rows.copy(), h0.scores.copy()
    h0.close()
    n = FC.slice_records() + 37
    assert n == (1 << 20) + 37
    idx = np.arange(n) % k
    t_off = np.concatenate([[0], np.cumsum(cnt[idx])]).astype(np.uint64)
    first = np.repeat(off[idx].astype(np.int64) - t_off[:-1].astype(np.int64), cnt[idx])
    t_ops = ops[first + np.arange(int(t_off[-1]))]                     # record r's ops are those of record idx[r]
    h = c.aligned_dev_from_ops(rows[idx], t_off, t_ops)
    m = h.mirror()
    try:
        assert m.n == 2 * n
        w_nops = np.array([len(A.parse_cigar(x)) for x in w_cig], np.uint32)
        assert np.array_equal(m.rows, np.concatenate([src_rows[idx], w_rows[idx]]))
        assert np.array_equal(m.scores.astype(np.int64), np.concatenate([src_scores[idx].astype(np.int64), w_sc[idx]]))
        assert np.array_equal(m.n_ops, np.concatenate([cnt[idx].astype(np.uint32), w_nops[idx]]))
        assert np.array_equal(m.ok, np.concatenate([np.ones(n, bool), w_ok[idx]]))
        assert m.failed == h.failed + int((~w_ok[idx]).sum()) and h.failed == 0
        # the text: the 64 mirrors around the first one of the second slice, the first and the last mirror
        lo = n + FC.slice_records() - 32
        for r in list(range(lo, lo + 64)) + [n, 2 * n - 1]:
            assert m.cigar(r) == w_cig[idx[r - n]], (r, m.cigar(r), w_cig[idx[r - n]])
        assert m.cigar(n - 1) == src_cig[idx[n - 1]] and m.cigar(0) == src_cig[0]
    finally:
        h.close(); m.close()


# ---- 2. the aligner's handles ----------------------------------------------------------------------------------------------------------------
def _random_batch():
    """~300 records of 1-3 kb: both strands, 0.5 .. 8 % error, long indels of 70-100 bases"""
    sb = synth.merge([
        synth.generate(4, 1024, 24, seed=211, p_partial=0.3, min_partial_len=64, flank_min=20, flank_max=200),
        synth.generate(4, 2048, 24, seed=212, p_sub=0.03, p_ins=0.025, p_del=0.025, p_partial=0.2, flank_min=20, flank_max=200),
        synth.generate(3, 3000, 24, seed=213, p_sub=0.002, p_ins=0.0015, p_del=0.0015, flank_min=20, flank_max=200),
        synth.generate(2, 2048, 16, seed=214, p_long_indel=0.002, flank_min=20, flank_max=200),
    ])
    return sb, sb.aln[:, :9].copy()


def _aligned_and_mirrored(c, codes, rows, tag, min_moved=0):
    h = c.align_dev(rows)
    m = h.mirror()
    try:
        out = _equals_the_reference(h, m, codes, tag)
        src_cig = out[3][:h.n]
        moved = [0, 0]                                                    # records whose mirrored ops the normalisation changed, by strand
        for r in np.flatnonzero(h.ok):
            s = int(h.rows[r, 4])
            moved[s] += out[3][h.n + r] != A.cigar_text(MR.mirror_ops(A.parse_cigar(src_cig[r]), s))
        assert moved[1] >= min_moved, (tag, moved)
        return out, h.failed, m.failed, moved
    finally:
        h.close(); m.close()


def _all_three_sets(c):
    res = []
    sb, rows = _random_batch()
    span = (rows[:, 3] - rows[:, 2]).astype(np.int64)
    assert len(rows) == 296 and set(rows[:, 4].tolist()) == {0, 1} and span.min() < 1100 and span.max() > 2800
    G.load_synth(c, sb)
    codes = [A.store_codes(sb.read_seq(i)) for i in range(sb.n_reads)]
    out, hf, mf, _ = _aligned_and_mirrored(c, codes, rows, "random", min_moved=20)
    assert hf == 0 and mf == 0
    assert max(ln for x in out[3] for ln, t in A.parse_cigar(x) if t != A.M_) >= 70
    res.append(out)
    ws, wcodes = H.low()
    c.set_reads(ws.seq, ws.qual, ws.off)
    true = LC.true_rows(ws)
    pick = np.concatenate([np.flatnonzero(true[:, 4] == 1)[:10], np.flatnonzero(true[:, 4] == 0)[:10]])
    assert len(pick) == 20
    out, hf, mf, _ = _aligned_and_mirrored(c, wcodes, true[np.sort(pick)], "true pairs", min_moved=5)
    assert hf == 0 and mf == 0
    res.append(out)
    rd, grows, _, gcodes = H.grid()
    assert len(grows) == 400
    c.set_reads(*MC.store(rd))
    out, hf, mf, moved = _aligned_and_mirrored(c, gcodes, grows, "grid")
    assert hf == 0 and mf == 0 and moved == [0, 45]                       # what the reference moves on the grid: strand 1 only
    res.append(out)
    return res


def test_mirrors_of_the_aligners_records_equal_the_reference_twice():
    c = G.ctx()
    first = _all_three_sets(c)
    second = _all_three_sets(c)
    assert first == second


# ---- 3. reads -> FASTA with one alignment per pair ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,batch_mode", [(256, 0), (1024, 1)])
def test_reads_to_fasta_through_the_pair_path(W, batch_mode):
    sb = synth.generate(2, 3000, 5, seed=231 + W, flank_min=100, flank_max=300)
    assert sb.n_reads == 12
    c = G.ctx()
    G.load_synth(c, sb)
    rids, rows, aln_off, _ = c.find_overlaps(max_occ=64, min_score=200)
    prim, rec_of_row = api.pair_rows(rows)
    assert len(rows) >= 40 and 2 * len(prim) == len(rows)                 # every row the finder emits has its mate
    rows_e, ext, _ = c.extend_overlaps(rows[prim])
    h = c.align_dev(rows_e)
    m = h.mirror()
    h.close()                                                            # the mirrored handle owns its store
    assert m.n == 2 * len(prim) and m.failed == 0
    j_rids, off2, rec = api.paired_job_args(rids, aln_off, rec_of_row, m.ok)
    assert j_rids.tolist() == rids.tolist() and off2.tolist() == aln_off.tolist()        # as many alignments per target as the finder gave it
    job = c.create_job_aligned(j_rids, off2, rec, m, W)
    rows2 = m.rows[rec]
    cig2 = [m.cigar(int(r)) for r in rec]
    np_ = len(prim)
    mates = np.flatnonzero(rec >= np_)
    assert len(mates) == np_
    assert np.array_equal(rows2[mates][:, 5:9], m.rows[rec[mates] - np_][:, 0:4])          # a mirror's target span is its primary's query span
    assert np.array_equal(rows2[:, 5], rows[:, 5]) and np.array_equal(rows2[:, 0], rows[:, 0])
    m.close()
    assert c._l.herro_debug_job_dev_built(job.h) == 1
    job.featurize()
    blob = b"".join(cig2)
    lens = np.array([len(x) for x in cig2], np.uint64)
    rows10 = rows2.astype(np.uint32).copy()
    rows10[:, 9] = lens
    sb2 = synth.SynthBatch(seq=sb.seq, qual=sb.qual, off=sb.off, aln=rows10, cig=np.frombuffer(blob + b"\0", np.uint8).copy(),
                           cig_off=np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64), tgt_aln_off=off2, tgt_rid=j_rids)
    store = G.O.store_from_synth(sb2)
    assert G.compare_features(job, sb2, store, W) > 0                     # window infos and features
    job.infer(64, batch_mode)
    job.consensus()
    w = n_fasta = 0
    for t in range(sb2.n_targets):
        rid, orows, ocigs = G.O.target_alignments(sb2, t)
        res = store.extract_features(rid, orows, ocigs, W)
        lg = [job.logits(w + wi)[1] for wi in range(len(res)) if job.info(w + wi).n_supported]
        w += len(res)
        lg = np.concatenate(lg) if lg else np.zeros((0, 5), np.float32)
        got = job.consensus_fasta(t, sb2.read_name(rid))
        assert got == res.consensus_fasta(lg), f"FASTA mismatch, target {t}"
        n_fasta += got.count(">")
    assert n_fasta >= 1
    job.close()


# ---- 4. errors ------------------------------------------------------------------------------------------------------------------------------
def test_errors_and_the_empty_handle():
    names, reads, rows, off, ops, _ = MC.hand()
    c = G.ctx()
    c.set_reads(*MC.store(reads))
    e0 = c.aligned_dev_from_ops(np.zeros((0, 9), np.uint32), np.zeros(1, np.uint64), np.zeros(0, np.uint32))
    m = e0.mirror()
    assert m.n == 0 and m.failed == 0
    m.close(); e0.close()
    h = c.aligned_dev_from_ops(rows, off, ops)
    other = api.Context(0)
    try:
        out = api.C.c_void_p()
        assert c._l.herro_aligned_dev_mirror(other.h, h.h, api.C.byref(out)) == -1 and "another context" in other.last_error()
        h2 = other.aligned_dev_from_ops(rows, off, ops)                   # no reads set on `other`
        with pytest.raises(api.HerroError) as e:
            h2.mirror()
        assert e.value.code == -6 and "herro_set_reads" in str(e.value)   # HERRO_E_STATE
        h2.close()
    finally:
        other.close()
    bad = rows.copy()
    bad[3, 3] = bad[3, 1] + 1                                            # a query end past its read
    hb = c.aligned_dev_from_ops(bad, off, ops)
    with pytest.raises(api.HerroError) as e:
        hb.mirror()
    assert e.value.code == -1 and "record 3" in str(e.value)
    hb.close(); h.close()
