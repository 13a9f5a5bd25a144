"""-m gpu: herro_extend_overlaps (k_extend) bit for bit against tests/extend_ref.py, the reads -> FASTA pipeline
with the extension step against the oracle and against the same chain without it, and the error codes."""
import dataclasses
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gpu_common as G  # noqa: E402
import extend_ref as E  # noqa: E402
import frontend_cases as FC  # noqa: E402
from herro_amd import api, synth  # noqa: E402

pytestmark = pytest.mark.gpu

COMP = bytes.maketrans(b"ACGTN", b"TGCAN")
LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 300, 600)      # the band's half width, its width, and past it
SPAN = 60


def _rand(rng, n) -> bytes:
    return bytes(b"ACGT"[x] for x in rng.integers(0, 4, n))


def _mutate(rng, seq: bytes, p: float) -> bytes:
    out = bytearray()
    for b in seq:
        x = rng.random()
        if x < p / 3:
            continue                                        # deletion
        if x < 2 * p / 3:
            out.append(b"ACGT"[rng.integers(0, 4)])         # insertion in front of the base
        elif x < p:
            out.append(b"ACGT"[(b"ACGT".index(b) + 1 + rng.integers(0, 3)) % 4])
            continue
        out.append(b)
    return bytes(out)


def _flanks(rng, a: int, b: int, kind: int):
    """(target flank of a bases, query flank of b bases) written away from the span.  Both come from one ancestor, so the shorter one
    ends on its read's end while they still agree (T only / Q only; both when a == b and nothing was inserted or deleted); kind 1 puts
    a 70-100-base indel into flanks long enough for the band to follow it, kind 2 makes the two unrelated, kind 3 lets them agree
    for four bases only."""
    if kind == 2:
        return _rand(rng, a), _rand(rng, b)
    if kind == 3:
        head = _rand(rng, 4)
        return (head + b"A" * a)[:a], (head + b"C" * b)[:b]
    anc = _rand(rng, max(a, b) + 160)
    p = float(rng.choice([0.0, 0.005, 0.02, 0.05, 0.08]))
    t, q = _mutate(rng, anc, p / 2), _mutate(rng, anc, p / 2)
    if kind == 1 and min(a, b) >= 300:
        g = int(rng.integers(70, 101))
        at = int(rng.integers(60, 140))
        if rng.random() < 0.5:
            t = t[:at] + _rand(rng, g) + t[at:]
        else:
            q = q[:at] + _rand(rng, g) + q[at:]
    return t[:a], q[:b]


def build_batch(seed=130):
    """~200 records: every pair of LENGTHS as (target, query) flank lengths on the right side and, permuted, on the left; both strands."""
    rng = np.random.default_rng(seed)
    reads, rows = [], []
    combos = [(a, b) for a in LENGTHS for b in LENGTHS]
    perm = rng.permutation(len(combos))
    for x, (a, b) in enumerate(combos):
        for strand in (0, 1):
            la, lb = combos[int(perm[(x + 7 * strand) % len(combos)])]
            kind_r = 1 if min(a, b) >= 300 else int(rng.choice([0, 0, 0, 0, 2, 3]))
            kind_l = 1 if min(la, lb) >= 300 else int(rng.choice([0, 0, 0, 0, 2, 3]))
            tr, qr = _flanks(rng, a, b, kind_r)
            tl, ql = _flanks(rng, la, lb, kind_l)
            core = _rand(rng, SPAN)
            t = tl[::-1] + core + tr                        # (a left flank is written away from the span: reversed into read order)
            q = ql[::-1] + core + qr
            if rng.random() < 0.15:                         # non-ACGT bases: the store's codes decide, whatever they are
                k = int(rng.integers(0, len(q)))
                q = q[:k] + b"N" + q[k + 1:]
                k = int(rng.integers(0, len(t)))
                t = t[:k] + b"NN"[:len(t) - k] + t[k + 2:]
            qs = len(ql)
            if strand:
                q = q.translate(COMP)[::-1]
                qs = len(q) - len(ql) - SPAN
            rows.append([len(reads) + 1, len(q), qs, qs + SPAN, strand, len(reads), len(t), len(tl), len(tl) + SPAN])
            reads += [t, q]
    return reads, np.array(rows, np.uint32)


_CACHE = {}


def _batch():
    if "b" not in _CACHE:
        reads, rows = build_batch()
        _CACHE["b"] = (reads, rows, [E.store_codes(r) for r in reads])
    return _CACHE["b"]


def _load(c, reads):
    seq = np.frombuffer(b"".join(reads), np.uint8)
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    c.set_reads(seq, np.full(len(seq), 40, np.uint8), off)


PARAMS = [dict(), dict(max_ext=50), dict(zdrop=30)]


def test_extension_equals_the_reference_bit_for_bit():
    reads, rows, codes = _batch()
    assert len(rows) == 200 and set(rows[:, 4].tolist()) == {0, 1}
    c = G.ctx()
    _load(c, reads)
    seen_stop = set()
    for kw in PARAMS:
        st = {}
        want = E.extend_records(codes, rows, stats=st, **kw)
        got = c.extend_overlaps(rows, **kw)
        for name, g, w in zip(("rows", "ext", "scores"), got, want):
            bad = np.flatnonzero((g != w).any(axis=1))
            assert len(bad) == 0, (kw, name, len(bad), int(bad[0]), rows[bad[0]].tolist(), g[bad[0]].tolist(), w[bad[0]].tolist())
            assert g.dtype == w.dtype
        again = c.extend_overlaps(rows, **kw)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again)), kw
        ext = got[1]
        if not kw:
            assert (ext == 0).any() and (ext >= 600).any() and ((ext > 128) & (ext < 600)).any()
            assert (got[2] > 0).sum() > 250
            # the 70-100-base indels were followed: the two lengths of a side differ by that much
            assert (np.abs(ext[:, 0].astype(int) - ext[:, 1]) >= 70).sum() + (np.abs(ext[:, 2].astype(int) - ext[:, 3]) >= 70).sum() >= 8
        if kw.get("max_ext") == 50:
            assert ext.max() == 50
        if kw.get("zdrop") == 30:
            seen_stop = set(st["last"].ravel().tolist())
    assert {16, 32} <= seen_stop                             # z-drop fired at its first and at its second check


def test_records_past_one_slice_equal_the_reference():
    """The host sends the records through in slices (SLICE of frontend_api.hip): 37 records more than one slice, so the loop turns
    twice and the second turn is a short one.  The batch's 200 records, tiled; max_ext = 64 keeps a side at 64 x 64 cells."""
    reads, rows, codes = _batch()
    n = FC.slice_records() + 37
    assert n == (1 << 20) + 37
    idx = np.arange(n) % len(rows)
    want = E.extend_records(codes, rows, max_ext=64)
    assert want[1].max() == 64 and (want[1][idx[n - 37:]] > 0).any()        # the cap binds, and the short turn has work to do
    c = G.ctx()
    _load(c, reads)
    got = c.extend_overlaps(rows[idx], max_ext=64)
    for name, g, w in zip(("rows", "ext", "scores"), got, want):
        assert g.dtype == w.dtype and g.shape == (n,) + w.shape[1:], name
        bad = np.flatnonzero((g != w[idx]).any(axis=1))
        assert len(bad) == 0, (name, len(bad), int(bad[0]), g[bad[0]].tolist(), w[idx[bad[0]]].tolist())


def _chain(c, sb, W, extend):
    """reads -> job through find_overlaps [-> extend_overlaps] -> align_dev -> create_job_aligned; the job, its rows and CIGARs"""
    G.load_synth(c, sb)
    rids, rows, aln_off, _ = c.find_overlaps(max_occ=64, min_score=100)
    if extend:
        rows_e, ext, _ = c.extend_overlaps(rows)
        assert (rows_e[:, 7] <= rows[:, 7]).all() and (rows_e[:, 8] >= rows[:, 8]).all() and ext.sum() > 0
        rows = rows_e
    h = c.align_dev(rows)
    failed = h.failed
    j_rids, off2, rec = api.aligned_dev_job_args(rids, aln_off, h.ok)
    job = c.create_job_aligned(j_rids, off2, rec, h, W)
    rows2 = h.rows[rec]
    cig2 = [h.cigar(int(r)) for r in rec]
    h.close()
    return job, j_rids, off2, rows2, cig2, failed


def _pairs(job, of_reads):
    """(overlap, window) pairs of a job from its window infos, and the windows with alignments among those of the reads `of_reads`"""
    infos = [job.info(w) for w in range(job.n_windows)]
    return sum(i.n_alns for i in infos), sum(1 for i in infos if i.n_alns > 0 and i.rid in of_reads)


@pytest.mark.parametrize("W", [256, 1024, 4096])
def test_reads_to_fasta_with_the_extension_step(W):
    """At W = 4096 "a window with alignments where the chain without the step has none" is asked of the set's own 4096-bp targets:
    every anchor span on them is shorter than the read, so none passes the windowing's span test.  The finder also makes every
    query read (5-6 kb) a target, and a span between two of those can cover such a read's first window without any extension
    (48 windows in this set), so the job as a whole is never empty."""
    sb = synth.generate(n_targets=2, target_len=4096, n_overlaps=12, seed=91)
    targets = set(sb.tgt_rid.tolist())
    c = G.ctx()
    plain, *_ = _chain(c, sb, W, extend=False)
    base_pairs, base_windows = _pairs(_featurized(plain), targets)
    plain.close()
    job, j_rids, off2, rows2, cig2, failed = _chain(c, sb, W, extend=True)
    assert failed == 0
    job.featurize()
    pairs, windows = _pairs(job, targets)
    print(dict(W=W, pairs_without=base_pairs, pairs_with=pairs, windows_without=base_windows, windows_with=windows))
    assert pairs > base_pairs
    if W == 4096:
        assert base_windows == 0 and windows >= 1
    # the oracle fed the same rows and CIGARs
    blob = b"".join(cig2)
    lens = np.array([len(x) for x in cig2], np.uint64)
    rows10 = rows2.astype(np.uint32).copy()
    rows10[:, 9] = lens
    sb2 = dataclasses.replace(sb, aln=rows10, cig=np.frombuffer(blob + b"\0", np.uint8).copy(),
                              cig_off=np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64), tgt_aln_off=off2, tgt_rid=j_rids)
    store = G.O.store_from_synth(sb2)
    assert G.compare_features(job, sb2, store, W) > 0
    job.infer(64, 0)
    job.consensus()
    w = 0
    for t in range(sb2.n_targets):
        rid, orows, ocigs = G.O.target_alignments(sb2, t)
        res = store.extract_features(rid, orows, ocigs, W)
        lg = [job.logits(w + wi)[1] for wi in range(len(res)) if job.info(w + wi).n_supported]
        w += len(res)
        lg = np.concatenate(lg) if lg else np.zeros((0, 5), np.float32)
        assert job.consensus_fasta(t, sb.read_name(rid)) == res.consensus_fasta(lg), f"FASTA mismatch, target {t}"
    job.close()


def _featurized(job):
    job.featurize()
    return job


def test_error_codes_with_and_without_reads():
    reads, rows, _ = _batch()
    fresh = api.Context(0)
    try:
        with pytest.raises(api.HerroError) as e:
            fresh.extend_overlaps(rows[:4])
        assert e.value.code == -6                              # HERRO_E_STATE: no reads
        with pytest.raises(api.HerroError) as e:
            fresh.extend_overlaps(rows[:0])
        assert e.value.code == -6                              # n = 0 as herro_align_overlaps
        with pytest.raises(api.HerroError) as e:
            fresh.extend_overlaps(rows[:4], max_ext=(1 << 20) + 1)
        assert e.value.code == -1 and "max_ext" in str(e.value)   # before anything else
    finally:
        fresh.close()
    c = G.ctx()
    _load(c, reads)
    out, ext, sc = c.extend_overlaps(rows[:0])
    assert out.shape == (0, 10) and ext.shape == (0, 4) and sc.shape == (0, 2)
    bad = rows[:3].copy()
    bad[1, 3] = bad[1, 1] + 5                                  # qend past the read
    with pytest.raises(api.HerroError) as e:
        c.extend_overlaps(bad)
    assert e.value.code == -1 and "herro_extend_overlaps: record 1" in str(e.value)
    bad = rows[:3].copy()
    bad[2, 5] = len(reads) + 3                                 # target outside the store
    with pytest.raises(api.HerroError) as e:
        c.extend_overlaps(bad)
    assert e.value.code == -1 and "record 2" in str(e.value)
    bad = rows[:3].copy()
    bad[0, 4] = 2
    with pytest.raises(api.HerroError) as e:
        c.extend_overlaps(bad)
    assert e.value.code == -1 and "record 0" in str(e.value) and "strand" in str(e.value)
    with pytest.raises(api.HerroError) as e:
        c.extend_overlaps(rows[:3], max_ext=(1 << 20) + 1)
    assert e.value.code == -1
    got = c.extend_overlaps(rows[:3])                          # the context is as usable as before
    assert got[0].shape == (3, 10)
