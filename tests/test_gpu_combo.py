"""gpu: the finder's options in combination — the occurrence cut as a fraction, the rescue, the core mask and the chain look-back set together
(k_occ_pick feeding k_resc_kind, k_chain_far on the anchors of k_expand_resc inside the chunk cuts of a small scratch budget, the mask on top;
csrc/overlap_dev.hip) — against the composition of the references in tests/combo_cases.py, record for record: find_overlaps,
find_overlap_pairs with the extension, the 1 MiB budget against the default one byte for byte, and on the trials with the longest look-back the
alignment, its mirror and the windows built from them.  tests/test_combo_host.py shows on the CPU that the trials reach what is claimed here."""
import os
import re
import sys
import tempfile
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import align_ref as A  # noqa: E402
import combo_cases as CB  # noqa: E402
import gpu_common as G  # noqa: E402
import mirror_ref as MR  # noqa: E402
import pair_cases as PC  # noqa: E402
from herro_amd import api, synth  # noqa: E402

pytestmark = pytest.mark.gpu

T = CB.trials()
PARTS = 6
BUDGET = "HERRO_OVL_SCRATCH_MB"


def _ctx():
    c = G.ctx()
    c.set_seed_rescue(None)
    c.set_chain_lookback(0)
    return c


def _plain(c):
    """the shared context as the other modules expect it: rescue off, look-back 64"""
    c.set_seed_rescue(None)
    c.set_chain_lookback(0)
    assert c.chain_lookback == 64 and getattr(c, "_seed_rescue", (0, 0)) == (0, 0)


def _load(c, t):
    seq, qual, off, codes = CB.reads(t["set"])
    c.set_reads(seq, qual, off)
    c.set_seed_rescue(*(t["rescue"] or (None,)))                              # the context's setting; the look-back goes with each call
    fkw = dict(t["fkw"], lookback=t["lookback"], **(dict(occ_frac_ppm=t["ppm"]) if t["ppm"] else {}))
    ext = dict(extend=False) if t["extend"] is None else dict(extend=True, **t["extend"])
    return codes, fkw, ext, CB.mask(t["core"], len(codes))


def _budget(monkeypatch, mb):
    if mb is None:
        monkeypatch.delenv(BUDGET, raising=False)
    else:
        monkeypatch.setenv(BUDGET, str(mb))


def _stderr_of(fn):
    """(fn(), what the library wrote to stderr meanwhile)"""
    sys.stderr.flush()
    with tempfile.TemporaryFile() as f:
        saved = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            out = fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        return out, f.read().decode(errors="replace")


def _same_rows(got, want, tag):
    for g, w, f in zip(got, want, ("rids", "rows", "aln_off", "scores")):
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, f, g.shape, w.shape)
        bad = np.flatnonzero((g != w).reshape(len(g), -1).any(axis=1)) if g.size else []
        assert not len(bad), (tag, f, [(int(i), g[i].tolist(), w[i].tolist()) for i in bad[:4]])


def _one_trial(c, t, monkeypatch):
    tag = CB.tag(t)
    codes, fkw, ext, m = _load(c, t)
    st = CB.reference(t)[1]
    cut, rescued = st["cut"], int(st["rescued"].sum())
    _budget(monkeypatch, t["budget"])
    got = c.find_overlaps(core=m, **fkw)
    assert (c.last_occ_cut, c.last_rescued) == (cut, rescued), tag
    _same_rows(got, CB.expected_rows(t), tag)
    p = c.find_overlap_pairs(core=m, **ext, **fkw)
    try:
        assert (p.occ_cut, p.rescued) == (cut, rescued), tag
        PC.assert_same_fields(PC.pairs_fields(p), CB.expected_pairs(t), tag)
        pb = PC.pairs_bytes(p)
        p2 = c.find_overlap_pairs(core=m, **ext, **fkw)                        # a second call: the same bytes
        try:
            assert PC.pairs_bytes(p2) == pb, tag
        finally:
            p2.close()
    finally:
        p.close()
    if t["budget"] is not None:                                               # the twin under the default budget: the same bytes
        _budget(monkeypatch, None)
        twin = c.find_overlaps(core=m, **fkw)
        assert [x.tobytes() for x in twin] == [x.tobytes() for x in got], tag
        q = c.find_overlap_pairs(core=m, **ext, **fkw)
        try:
            assert PC.pairs_bytes(q) == pb and (q.occ_cut, q.rescued) == (cut, rescued), tag
        finally:
            q.close()
    assert c.chain_lookback == 64, tag                                        # the keyword left the context's look-back alone
    return len(got[1]), len(CB.reference(t)[0][1])


# ---- 1. find_overlaps and find_overlap_pairs ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("part", range(PARTS))
def test_the_finder_and_the_pairs_equal_the_composed_reference(part, monkeypatch):
    c = _ctx()
    t0 = time.perf_counter()
    try:
        for t in T[part::PARTS]:
            rows, unmasked = _one_trial(c, t, monkeypatch)
            print(f"{CB.tag(t)}: {rows} records of {unmasked}, cut {c.last_occ_cut}, rescued {c.last_rescued}")
    finally:
        _plain(c)
    print(f"part {part}: {time.perf_counter() - t0:.1f} s")


# ---- 2. the small budget cuts several chunks ------------------------------------------------------------------------------------------------
def test_a_budget_of_1_mib_cuts_several_chunks_on_six_trials(monkeypatch):
    c = _ctx()
    monkeypatch.setenv("HERRO_OVL_STATS", "1")
    seen = {}
    try:
        for t in T:
            if t["budget"] is None:
                continue
            codes, fkw, ext, m = _load(c, t)
            _budget(monkeypatch, t["budget"])
            got, err = _stderr_of(lambda: c.find_overlaps(core=m, **fkw))
            chunks = [int(x) for x in re.findall(r"^OVL .* chunks=(\d+)$", err, re.M)]
            assert len(chunks) == 1, (CB.tag(t), err[-500:])
            seen[t["number"]] = chunks[0]
            assert (len(re.findall(r"^OVLCHAIN lookback=%d " % t["lookback"], err, re.M)) == 1) == (t["lookback"] != 64), (CB.tag(t), err[-500:])
            assert ("OVLRESC" in err) == (t["rescue"] is not None) and ("OVLOCC" in err) == (t["ppm"] != 0), (CB.tag(t), err[-500:])
            _same_rows(got, CB.expected_rows(t), CB.tag(t))
    finally:
        _plain(c)
    print(dict(chunks_at_1_mib=seen))
    assert sum(1 for n in seen.values() if n > 1) >= 6, seen
    assert seen == {t["number"]: CB.chunks(t) for t in T if t["budget"] is not None}      # the chunk rule as include/herro_amd.h states it


# ---- 3. alignment, mirror and windows on the longest look-backs -----------------------------------------------------------------------------
MAX_ALIGNED_PAIRS = 64      # the numpy aligner takes about 0.1 s a pair


def _aligned_trials():
    """eight trials with the rescue on and the longest look-back that keep a pair under their mask (and no more than the reference aligns in
    a few seconds); the two with the most pairs go on to the windows"""
    n_pairs = lambda t: len(CB.expected_pairs(dict(t, extend=None))["primaries"])                # noqa: E731
    on = [t for t in T if t["rescue"] is not None and 0 < n_pairs(t) <= MAX_ALIGNED_PAIRS]
    chosen = sorted(on, key=lambda t: (-t["lookback"], t["number"]))[:8]
    return chosen, [t["number"] for t in sorted(chosen, key=lambda t: -n_pairs(t))[:2]]


def _align_equals_the_reference(c, t, p, codes, features):
    tag = CB.tag(t)
    n = p.n_pairs
    m = p.align()
    try:
        out, cigs, sc, ok, _ = A.align_records(codes, p.primaries, threads=4)
        w_rows, w_cigs, w_sc, w_ok = MR.mirror_records(codes, out, cigs, sc)
        want_rows, want_cig = np.concatenate([out[:, :9], w_rows[:, :9]]), list(cigs) + list(w_cigs)
        want_sc, want_ok = np.concatenate([sc, w_sc]), np.concatenate([ok, w_ok])
        assert m.n == 2 * n and m.failed == int((~want_ok).sum()), tag
        got_cig = [m.cigar(r) for r in range(m.n)]
        bad = [r for r in range(m.n) if not (np.array_equal(m.rows[r, :9], want_rows[r]) and int(m.scores[r]) == int(want_sc[r]) and bool(m.ok[r]) == bool(want_ok[r])
                                             and got_cig[r] == want_cig[r] and int(m.n_ops[r]) == len(A.parse_cigar(want_cig[r])))]
        assert not bad, (tag, [(r, m.rows[r].tolist(), want_rows[r].tolist(), int(m.scores[r]), int(want_sc[r]), got_cig[r][:60], want_cig[r][:60]) for r in bad[:4]])
        assert not m.rows[:, 9].any(), tag
        windows = 0
        if features:                                                          # reads to windows: the oracle fed the GPU's rows and CIGARs
            W = 256
            seq, qual, off, _ = CB.reads(t["set"])
            job = c.create_job_paired(p, m, W)
            try:
                j_rids, off2, rec = api.paired_job_args(p.rids, p.aln_off, p.rec_of_row, m.ok)
                assert len(rec) > 0, tag
                job.featurize()
                rows10 = m.rows[rec].astype(np.uint32).copy()
                cig2 = [got_cig[int(r)] for r in rec]
                lens = np.array([len(x) for x in cig2], np.uint64)
                rows10[:, 9] = lens
                sb = synth.SynthBatch(seq=seq, qual=qual, off=off, aln=rows10, cig=np.frombuffer(b"".join(cig2) + b"\0", np.uint8).copy(),
                                      cig_off=np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64), tgt_aln_off=off2, tgt_rid=j_rids)
                windows = G.compare_features(job, sb, G.O.store_from_synth(sb), W)
                assert windows > 0, tag
            finally:
                job.close()
        return int(want_ok.sum()), windows
    finally:
        m.close()


@pytest.mark.parametrize("i", range(8))
def test_alignment_mirror_and_windows_on_the_longest_lookbacks(i, monkeypatch):
    chosen, with_windows = _aligned_trials()
    assert len(chosen) == 8 and chosen[0]["lookback"] == 1024 and min(t["lookback"] for t in chosen) > 64 and len(with_windows) == 2
    t = chosen[i]
    c = _ctx()
    t0 = time.perf_counter()
    try:
        codes, fkw, ext, m = _load(c, t)
        _budget(monkeypatch, t["budget"])
        p = c.find_overlap_pairs(core=m, **ext, **fkw)
        try:
            PC.assert_same_fields(PC.pairs_fields(p), CB.expected_pairs(t), CB.tag(t))
            aligned, windows = _align_equals_the_reference(c, t, p, codes, t["number"] in with_windows)
            assert aligned > 0
        finally:
            p.close()
        print(f"{CB.tag(t)}: {p.n_pairs} pairs, {aligned} of {2 * p.n_pairs} records aligned, {windows} windows compared, {time.perf_counter() - t0:.1f} s")
    finally:
        _plain(c)


# ---- 4. afterwards ---------------------------------------------------------------------------------------------------------------------------
def test_the_shared_context_is_plain_afterwards():
    """rescue off and look-back 64: what a context that never had either setting returns, on a set where both matter"""
    c = G.ctx()
    t = next(t for t in T if t["set"] == "T0+T2")
    seq, qual, off, codes = CB.reads("T0+T2")
    c.set_reads(seq, qual, off)
    assert c.chain_lookback == 64
    kw = dict(k=15, w=5, max_occ=64, min_score=60)
    got = c.find_overlaps(**kw)
    assert c.last_rescued == 0 and c.last_occ_cut == 64
    _same_rows(got, CB.reference(dict(t, fkw=kw, ppm=0, rescue=None, lookback=64))[0], "plain")
