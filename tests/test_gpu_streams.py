"""-m gpu: the context on a caller's stream and across stream switches (herro_set_stream; the contract is include/herro_amd.h's,
DESIGN.md section 16).

Every other GPU test runs on the context's own stream and fetches a result right behind the call it tests.  Here the stream is varied:

1. every leg — the job path and the front end — on a created torch stream gives the bytes of the own stream, and on the caller's stream is
   held to its reference as well (features and FASTA against the oracle, logits of the stand-alone forward against the fp32 twin, found rows
   against overlap_ref.find_overlaps, alignments against align_ref.align_records); then set_stream(None) and set_stream(0): the same bytes;
2. the work really is on the caller's stream: behind a blocker queued on that stream (torch.cuda._sleep) and an event recorded behind the
   blocker, herro_job_featurize / herro_job_infer / herro_job_consensus return with the event PENDING (they only queue) and the fetch behind
   each with it complete, and every entry that drains its stream returns with it complete.  What this can tell apart: a build whose
   herro_set_stream ignores its argument (made by hand, run once on an MI355X, not kept) fails the three job-path steps and fasta_dev — they
   return within a millisecond with the event pending — and passes test 1.  The other nine draining entries pass under that build too: they
   take their scratch with hipMalloc and give it back with hipFree inside the call, and hipFree waits for every stream of the device, the
   caller's blocked one included, whichever stream the launches went to (the job path and fasta_dev recycle their memory through the
   context's free lists and make no such call).  For those nine the assertion is the contract a caller relies on — on return, whatever it
   queued before is complete — and not evidence of where the launches went;
3. a switch orders: work queued on stream A behind a blocker, a switch to B (or to the own stream), and what then runs on B — or the memory
   that is recycled there — sees that work complete: the bytes of the unswitched run.  (herro_set_stream waits for the stream it leaves.
   Without that wait the consensus kernels would read offsets whose upload is still queued, and ensure_sib would free buffers under running
   kernels: this part is never run against a library without the wait.)

Each test makes its own api.Context(0) and closes it, so a failure never leaves the suite's shared context on a foreign stream.

Inputs.  Job leg: synth.generate(16, 3 * 1024 + 50, 14, seed=31, flank_min=60, flank_max=90, p_partial=0.25) at W = 1024 (64 windows, at most 7
informative rows), and in the same read store two targets with p_snp=0.03 as a job of its own.  A window of 1024 positions of which 3 % differ
holds ~31 informative rows, never 64, so those two targets (4096 + 50 bases) are cut at W = 4096: 106 and 133 informative rows in their
first windows — sibling tiles, and ensure_sib's buffers, are part of the run.  Front end: read set A of tests/pair_cases.py, PC.DEFAULTS.

Blocker length (measured on an MI355X, wall clock around each call on the own stream, one run):
  find_adapters 0.8 ms, find_overlaps 4.1, find_overlap_pairs 2.1, OverlapPairs.align 4.4, extend_overlaps 0.2, OverlapPairs.cluster 1.6,
  AlignedDev.paf 0.9, cut_store 0.7, fasta_dev 0.7, model_forward 0.3; featurize 0.06, infer 0.06, logits 0.2, consensus 0.01,
  consensus_fasta 3.2 (first call of each in a fresh context; a second call is never slower).  Slowest: 4.4 ms; 20 times that is 87 ms.
The blocker is BLOCK_MS = 200 ms (45 times the slowest leg): at least 20 times the slowest leg, never below 100 ms, never above 1 s.
torch.cuda._sleep is calibrated with torch events when the module is imported (2.40 M cycles per millisecond there; a blocker asked for as
200 ms measured 200.7 ms).  Behind such a blocker featurize returned after 0.05 ms, the second infer after 0.04 ms and consensus after 0.01 ms
with the event pending; infer, logits and consensus_fasta after 199.9 - 200.0 ms with it complete: no entry waits where the code says it does not.
"""
import os
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import align_ref as A  # noqa: E402
import gpu_common as G  # noqa: E402
import overlap_ref as R  # noqa: E402
import pair_cases as PC  # noqa: E402
from herro_amd import api, model_io, synth  # noqa: E402

pytestmark = pytest.mark.gpu

BLOCK_MS = 200.0
TOL = 1e-3                     # the logit contract of the shipped precision (BASELINE.json north_star), as everywhere in the suite
W_SMALL, W_BIG = 1024, 4096
SMALL, BIG = tuple(range(16)), (16, 17)
JOBS = (("small", W_SMALL, SMALL), ("big", W_BIG, BIG))
FRONT_W = 256
CHOP = dict(chop_len=700, min_length=100, line_width=60)
_CACHE = {}


# ---- the blocker ---------------------------------------------------------------------------------------------------------------------------
def _calibrate():
    """cycles of torch.cuda._sleep per millisecond, by torch events (None without a GPU: the module is imported wherever the suite is collected)"""
    try:
        import torch
        if not torch.cuda.is_available():
            return None
    except Exception:
        return None
    s = torch.cuda.Stream()
    n, ms = 1 << 20, 0.0
    with torch.cuda.stream(s):
        torch.cuda._sleep(1000)                                    # (loads the kernel)
        while True:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch.cuda._sleep(n)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            if ms >= 20.0 or n >= 1 << 36:
                break
            n *= 4
    return n / ms


_CYCLES_PER_MS = _calibrate()


def _stream():
    import torch
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0                                      # (0 is the legacy default stream: herro_set_stream reads it as NULL)
    return s


def _block(s, ms=None):
    """a blocker of BLOCK_MS on stream s and the event recorded behind it"""
    import torch
    with torch.cuda.stream(s):
        torch.cuda._sleep(int((BLOCK_MS if ms is None else ms) * _CYCLES_PER_MS))
        marker = torch.cuda.Event()
        marker.record()
    return marker


def _ctx():
    c = api.Context(0)
    try:
        path, _ = model_io.default_model_file(G.CACHE)
        c.load_model(path)
        c.set_precision(api.DEFAULT_PRECISION)
    except Exception:
        c.close()
        raise
    return c


# ---- bytes of whatever an entry returns --------------------------------------------------------------------------------------------------------
def _bytes(x):
    if isinstance(x, (bytes, bytearray)):
        return bytes(x)
    if isinstance(x, str):
        return x.encode()
    if isinstance(x, np.ndarray):
        return str(x.dtype).encode() + b":" + repr(x.shape).encode() + b":" + np.ascontiguousarray(x).tobytes()
    if isinstance(x, (tuple, list)):
        return b"(" + b"|".join(_bytes(y) for y in x) + b")"
    if isinstance(x, dict):
        return _bytes([(k, x[k]) for k in sorted(x)])
    if isinstance(x, (int, np.integer, bool)):
        return repr(int(x)).encode()
    raise TypeError(type(x))


def _same(got, want, tag):
    assert list(got) == list(want), tag
    for k in want:
        assert got[k] == want[k], (tag, k, len(got[k]), len(want[k]))


# ---- the job leg -------------------------------------------------------------------------------------------------------------------------------
def _job_inputs():
    if "job" not in _CACHE:
        a = synth.generate(16, 3 * 1024 + 50, 14, seed=31, flank_min=60, flank_max=90, p_partial=0.25)
        d = synth.generate(2, 4096 + 50, 14, seed=32, flank_min=60, flank_max=90, p_snp=0.03)
        sb = synth.merge([a, d])
        assert sb.n_targets == 18
        _CACHE["job"] = (sb, G.O.store_from_synth(sb))
    return _CACHE["job"]


def _ids(sb, ts):
    return [sb.read_name(int(sb.tgt_rid[t])) for t in ts]


def _forward_batch(wins):
    """model_forward's arguments from encoded window copies (collate padding as inference.rs:86-97)"""
    lmax = max(g.info.length for g in wins)
    bases = np.full((len(wins), lmax, 31), 11, np.uint8)
    quals = np.full((len(wins), lmax, 31), 126, np.uint8)
    lens, flat = [], []
    for k, g in enumerate(wins):
        bases[k, :g.info.length] = g.bases
        quals[k, :g.info.length] = g.quals
        tidx = np.flatnonzero(g.bases[:, 0] != 4)
        lens.append(len(g.sup_pos))
        flat.extend((tidx[g.sup_pos.astype(np.int64)] + g.sup_ins).tolist())
    return bases, quals, np.array(lens, np.int32), np.array(flat, np.int32)


def _twin_logits(batch):
    """the fp32 twin on the forward batch: computed once"""
    if "twin" not in _CACHE:
        import model_ref as MR
        _, raw = model_io.default_model_file(G.CACHE)
        _CACHE["twin"] = MR.run_batch(MR.build(raw, model_io.Hyper()), *batch)
    return _CACHE["twin"]


def _job_leg(c, check=False):
    """create_job -> featurize -> infer(16, 1) -> consensus -> fasta, fasta_dev with a chop_len, window() copies, logits(), model_forward on
    the stream the context is on: {name: bytes}.  check: every result against its reference as well."""
    sb, store = _job_inputs()
    G.load_synth(c, sb)
    out = {}
    for tag, W, ts in JOBS:
        job = api.job_from_synth(c, sb, W, targets=ts)
        try:
            ids = _ids(sb, ts)
            job.featurize()
            job.infer(16, 1)
            nsup = np.array([job.info(w).n_supported for w in range(job.n_windows)])
            if tag == "small":
                assert job.n_windows == 64 and 0 < nsup.max() <= 64
            else:
                assert nsup.max() > 64, "the case needs a window on sibling tiles"
            lg = [job.logits(w) for w in range(job.n_windows)]          # (before any window copy: the model read k_rfq's receptive fields)
            out[tag + ".nsup"] = _bytes(nsup)
            out[tag + ".logits"] = _bytes(lg)
            job.consensus()
            out[tag + ".fasta"] = job.fasta(ids)
            out[tag + ".fasta_dev"] = job.fasta_dev(ids, **CHOP)
            out[tag + ".consensus_fasta"] = _bytes([job.consensus_fasta(t, ids[t]) for t in range(len(ids))])
            assert out[tag + ".fasta"].count(b">") == len(ids) and out[tag + ".fasta_dev"].count(b"_sliding:") > len(ids)
            wins = [job.window(w) for w in range(job.n_windows)]
            out[tag + ".windows"] = _bytes([(g.bases, g.quals, g.sup_pos, g.sup_ins, g.qids) for g in wins])
            if tag == "small":
                sel = [int(w) for w in np.flatnonzero(nsup > 0)[:4]] + [int(np.argmax(nsup))]
                batch = _forward_batch([job.window(w, encoded=True) for w in sel])
                info, base = c.model_forward(*batch)
                out["forward"] = _bytes((info, base))
            if check:
                assert G.compare_features(job, sb, store, W, targets=ts) == job.n_windows
                w = 0
                for k, t in enumerate(ts):                                   # FASTA == the oracle's decode of the same logits
                    rid, rows, cigs = G.O.target_alignments(sb, t)
                    res = store.extract_features(rid, rows, cigs, W)
                    part = [lg[w + wi][1] for wi in range(len(res)) if nsup[w + wi]]
                    want = res.consensus_fasta(np.concatenate(part) if part else np.zeros((0, 5), np.float32))
                    assert want and job.consensus_fasta(k, ids[k]) == want, (tag, t)
                    w += len(res)
                if tag == "small":
                    ti, tb = _twin_logits(batch)
                    assert info.shape == ti.shape and base.shape == tb.shape and len(info) >= 5
                    err = max(float(np.abs(info - ti).max()), float(np.abs(base - tb).max()))
                    print(f"model_forward on the caller's stream against the fp32 twin: max abs logit error {err:.3e}")
                    assert err <= TOL
        finally:
            job.close()
    return out


# ---- the front end -----------------------------------------------------------------------------------------------------------------------------
def _front_inputs():
    if "front" not in _CACHE:
        rs = PC.set_a()
        codes = [R.store_codes(rs.read_seq(i)) for i in range(rs.n_reads)]
        lens = np.diff(rs.off.astype(np.int64))
        names = [rs.read_name(i).encode() for i in range(rs.n_reads)]
        adapter = rs.read_seq(3)[1000:1024]                                # 24 bases of read 3: it has hits
        pieces = np.zeros(rs.n_reads, api.PIECE_DTYPE)
        for i, n in enumerate(lens):
            pieces[i] = (i, 40 + i, int(n) - 25)
        _CACHE["front"] = (rs, codes, lens, names, adapter, pieces)
    return _CACHE["front"]


def _front_refs():
    """the CPU references of the front end on set A, once: found rows, and the alignments of `rows` when asked"""
    rs, codes = _front_inputs()[:2]
    if "find_ref" not in _CACHE:
        _CACHE["find_ref"] = R.find_overlaps(codes, **PC.DEFAULTS)
    return _CACHE["find_ref"]


def _align_ref(rows):
    codes = _front_inputs()[1]
    key = ("align_ref", rows.tobytes())
    if key not in _CACHE:
        _CACHE[key] = A.align_records(codes, rows, threads=8)
    return _CACHE[key]


def _same_rows(got, want, tag):
    for g, w, f in zip(got, want, ("rids", "rows", "aln_off", "scores")):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (tag, f, g.shape, w.shape)


def _handle_fields(m):
    return (m.rows, m.scores, m.n_ops, [m.cigar(r) for r in range(m.n)])


def _front_leg(c, check=False):
    """set_reads, find_adapters, find_overlaps with and without an index in parts, find_overlap_pairs(extend=True) -> align -> mirror ->
    create_job_paired -> FASTA, extend_overlaps, OverlapPairs.cluster, AlignedDev.paf, cut_store (and the finder on the cut store) on the stream
    the context is on: {name: bytes}.  check: found rows and alignments against their CPU references as well."""
    rs, codes, lens, names, adapter, pieces = _front_inputs()
    out = {}
    PC.load(c, rs)
    hits, hits_off = c.find_adapters([adapter])
    assert len(hits) >= 1
    out["adapters"] = _bytes((hits, hits_off))
    found = c.find_overlaps(**PC.DEFAULTS)
    out["find"] = _bytes(found)
    parts = c.find_overlaps(index_kmers=int(lens.sum()) // 3, **PC.DEFAULTS)
    assert c.last_index_blocks >= 2
    out["find_parts"] = _bytes(parts)
    p = c.find_overlap_pairs(**PC.DEFAULTS)
    assert p.n_pairs >= 20 and p.ext.any()
    out["pairs"] = PC.pairs_bytes(p)
    m = p.align()
    assert m.n == 2 * p.n_pairs and m.failed == 0
    out["align"] = _bytes(_handle_fields(m))
    h = c.align_dev(p.primaries)
    hm = h.mirror()
    out["mirror"] = _bytes(_handle_fields(hm))
    assert out["mirror"] == out["align"]
    prim, _ = api.pair_rows(found[1], exact_ids=True)
    ext = c.extend_overlaps(found[1][prim].reshape(len(prim), 10))
    out["extend"] = _bytes(ext)
    cl = p.cluster(2)
    out["cluster"] = _bytes((cl.part, cl.rank, cl.comp, cl.level, cl.part_stats, cl.mask(0), cl.mask(1)))
    out["paf"] = m.paf(names)
    assert out["paf"].count(b"\n") == m.n and b"cg:Z:" in out["paf"]
    jp = c.create_job_paired(p, m, FRONT_W)
    try:
        jp.featurize(); jp.infer(64, 1); jp.consensus()
        out["paired.fasta"] = jp.fasta([n.decode() for n in names])
        assert out["paired.fasta"].count(b">") > 0
    finally:
        jp.close()
    if check:
        want = _front_refs()
        _same_rows(found, want, "find_overlaps")
        _same_rows(parts, want, "find_overlaps, index in parts")
        assert np.array_equal(ext[0], p.primaries)                          # (the handle's primaries ARE the extended rows: aligned below)
        r_out, r_cig, r_sc, r_ok, _ = _align_ref(p.primaries)
        assert r_ok.all()
        for r in range(p.n_pairs):
            assert np.array_equal(m.rows[r, :9], r_out[r, :9]) and m.cigar(r) == r_cig[r] and int(m.scores[r]) == int(r_sc[r]), r
    for x in (p, m, h, hm, cl):
        x.close()
    c.cut_store(pieces)
    out["cut"] = _bytes(c.store_arrays())
    out["cut.find"] = _bytes(c.find_overlaps(**PC.DEFAULTS))
    if check:
        cut_codes = [codes[i][40 + i:int(lens[i]) - 25] for i in range(len(codes))]
        _same_rows(c.find_overlaps(**PC.DEFAULTS), R.find_overlaps(cut_codes, **PC.DEFAULTS), "find_overlaps on the cut store")
    return out


def _own(which):
    """the leg on the context's own stream, in a context of its own: the unswitched bytes, computed once and left unchanged"""
    if ("own", which) not in _CACHE:
        c = _ctx()
        try:
            _CACHE["own", which] = (_job_leg if which == "job" else _front_leg)(c)
        finally:
            c.close()
    return _CACHE["own", which]


# ---- 1. every leg on a caller's stream -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["job", "front"])
def test_every_leg_on_a_callers_stream_equals_its_reference_and_the_own_stream(which):
    leg = _job_leg if which == "job" else _front_leg
    want = _own(which)
    c = _ctx()
    try:
        ext = _stream()
        c.set_stream(ext.cuda_stream)
        _same(leg(c, check=True), want, (which, "caller's stream"))
        c.set_stream(None)
        _same(leg(c), want, (which, "set_stream(None)"))
        c.set_stream(ext.cuda_stream)
        c.set_stream(0)                                                       # handle 0 is NULL: the own stream again
        _same(leg(c), want, (which, "set_stream(0)"))
    finally:
        c.close()


# ---- 2. the work really is on the caller's stream ------------------------------------------------------------------------------------------------
def _pairs(c):
    return c.find_overlap_pairs(**PC.DEFAULTS)


def _pairs_aligned(c):
    p = _pairs(c)
    return p, p.align()


def _inferred_small(c):
    sb, _ = _job_inputs()
    G.load_synth(c, sb)
    job = api.job_from_synth(c, sb, W_SMALL, targets=SMALL)
    job.featurize(); job.infer(16, 1); job.consensus()
    return job


def _forward_args(c):
    job = _inferred_small(c)
    try:
        nsup = np.array([job.info(w).n_supported for w in range(job.n_windows)])
        return _forward_batch([job.window(int(w), encoded=True) for w in np.flatnonzero(nsup > 0)[:4]])
    finally:
        job.close()


# name: (reads, what is prepared in front of the blocker, the entry); every entry here drains its stream before it returns.  Only fasta_dev tells a
# library that launches elsewhere apart (module docstring, 2.): the others also wait for the device when they free their scratch.
DRAINING = {
    "find_adapters": ("front", lambda c: None, lambda c, s: c.find_adapters([_front_inputs()[4]])),
    "find_overlaps": ("front", lambda c: None, lambda c, s: c.find_overlaps(**PC.DEFAULTS)),
    "find_overlap_pairs": ("front", lambda c: None, lambda c, s: _pairs(c).close()),
    "align": ("front", _pairs, lambda c, p: p.align().close()),
    "extend_overlaps": ("front", lambda c: _pairs(c).primaries, lambda c, rows: c.extend_overlaps(rows)),
    "cluster": ("front", _pairs, lambda c, p: p.cluster(2).close()),
    "paf": ("front", _pairs_aligned, lambda c, pm: pm[1].paf(_front_inputs()[3])),
    "cut_store": ("front", lambda c: None, lambda c, s: c.cut_store(_front_inputs()[5])),
    "fasta_dev": ("job", _inferred_small, lambda c, job: job.fasta_dev(_ids(_job_inputs()[0], SMALL), **CHOP)),
    "model_forward": ("job", _forward_args, lambda c, batch: c.model_forward(*batch)),
}


@pytest.mark.parametrize("name", list(DRAINING))
def test_an_entry_that_drains_its_stream_waits_for_the_callers_stream(name):
    reads, prepare, entry = DRAINING[name]
    c = _ctx()
    state = None
    try:
        ext = _stream()
        c.set_stream(ext.cuda_stream)
        if reads == "front":
            PC.load(c, _front_inputs()[0])
        state = prepare(c)
        marker = _block(ext)
        t0 = time.perf_counter()
        entry(c, state)
        done = marker.query()
        print(f"{name}: returned {1e3 * (time.perf_counter() - t0):.1f} ms behind a blocker of {BLOCK_MS:.0f} ms, marker complete: {done}")
        assert done, f"{name} returned with the caller's stream still blocked: its work is not on that stream"
    finally:
        for x in (state if isinstance(state, tuple) else (state,)):
            if hasattr(x, "close"):
                x.close()
        c.close()


# the job path: (what runs in front of the blocker, the call that only queues, the fetch that waits); the job is created in front of the blocker
JOB_STEPS = {
    # herro_job_featurize returns at once (k_rows .. k_rfq queued); herro_job_infer waits for ev_counts, recorded behind them
    "featurize_infer": (lambda job: None, lambda job: job.featurize(), lambda job: job.infer(16, 1)),
    # the counts are on the host: the descriptor upload and the model are only queued; herro_job_window_logits waits for them
    "infer_logits": (lambda job: (job.featurize(), job.info(0)), lambda job: job.infer(16, 1), lambda job: job.logits(0)),
    # k_consensus is only queued; herro_job_consensus_fasta fetches the corrected bases behind it
    "consensus_fasta": (lambda job: (job.featurize(), job.infer(16, 1), job.logits(0)), lambda job: job.consensus(),
                        lambda job: job.consensus_fasta(0, _ids(_job_inputs()[0], SMALL)[0])),
}


@pytest.mark.parametrize("step", list(JOB_STEPS))
def test_the_job_path_queues_on_the_callers_stream_and_its_fetches_wait_for_it(step):
    before, queues, fetch = JOB_STEPS[step]
    sb, _ = _job_inputs()
    c = _ctx()
    job = None
    try:
        ext = _stream()
        c.set_stream(ext.cuda_stream)
        G.load_synth(c, sb)
        job = api.job_from_synth(c, sb, W_SMALL, targets=SMALL)
        before(job)
        marker = _block(ext)
        queues(job)
        assert not marker.query(), f"{step}: the blocker is too short, or the first call waited for the stream"   # (never a vacuous pass below)
        fetch(job)
        assert marker.query(), f"{step}: the fetch returned with the caller's stream still blocked: the work queued before it is not on that stream"
    finally:
        if job is not None:
            job.close()
        c.close()


# ---- 3. a switch orders ----------------------------------------------------------------------------------------------------------------------------
def _logits_bytes(job):
    return _bytes([job.logits(w) for w in range(job.n_windows)])


def test_switch_between_infer_and_consensus():
    sb, _ = _job_inputs()
    want = _own("job")
    c = _ctx()
    job = None
    try:
        a, b = _stream(), _stream()
        c.set_stream(a.cuda_stream)
        G.load_synth(c, sb)
        job = api.job_from_synth(c, sb, W_SMALL, targets=SMALL)
        job.featurize()
        job.info(0)                                                           # (the counts are on the host: infer below only queues)
        marker = _block(a)
        job.infer(16, 1)                                                      # the blob — sup_off in it — and the model: queued on A behind the blocker
        pending = not marker.query()
        c.set_stream(b.cuda_stream)
        assert pending and marker.query(), "the switch did not wait for what was queued on the stream it left"
        job.consensus()
        assert job.fasta(_ids(sb, SMALL)) == want["small.fasta"]
        assert _logits_bytes(job) == want["small.logits"]
    finally:
        if job is not None:
            job.close()
        c.close()


def test_switch_to_the_own_stream_between_featurize_and_infer():
    sb, _ = _job_inputs()
    want = _own("job")
    c = _ctx()
    job = None
    try:
        a = _stream()
        c.set_stream(a.cuda_stream)
        G.load_synth(c, sb)
        job = api.job_from_synth(c, sb, W_SMALL, targets=SMALL)
        marker = _block(a)
        job.featurize()                                                       # k_rfq, the early gather, is queued on A behind the counts' event
        pending = not marker.query()
        c.set_stream(None)
        assert pending and marker.query()
        job.infer(16, 1)
        assert _logits_bytes(job) == want["small.logits"]
    finally:
        if job is not None:
            job.close()
        c.close()


def test_two_jobs_inferred_on_either_side_of_a_switch_share_the_scratch():
    """job 1 has no window above 64 informative rows, job 2 has: the sibling buffers are first made (ensure_sib) behind the switch, and the
    model scratch of the context grows there, while job 1's model is queued on the stream that was left"""
    sb, _ = _job_inputs()
    want = _own("job")
    c = _ctx()
    j1 = j2 = None
    try:
        a, b = _stream(), _stream()
        c.set_stream(a.cuda_stream)
        G.load_synth(c, sb)
        j1 = api.job_from_synth(c, sb, W_SMALL, targets=SMALL)
        j2 = api.job_from_synth(c, sb, W_BIG, targets=BIG)
        j1.featurize()
        j1.info(0)
        marker = _block(a)
        j1.infer(16, 1)
        pending = not marker.query()
        c.set_stream(b.cuda_stream)
        assert pending and marker.query()
        j2.featurize()
        j2.infer(16, 1)
        assert _logits_bytes(j2) == want["big.logits"]
        assert _logits_bytes(j1) == want["small.logits"]
    finally:
        for j in (j1, j2):
            if j is not None:
                j.close()
        c.close()


def test_a_job_freed_behind_a_switch_gives_its_arena_to_the_next_job():
    sb, _ = _job_inputs()
    want = _own("job")
    c = _ctx()
    job = nxt = None
    try:
        a, b = _stream(), _stream()
        c.set_stream(a.cuda_stream)
        G.load_synth(c, sb)
        job = api.job_from_synth(c, sb, W_SMALL, targets=SMALL)
        job.featurize()
        job.info(0)
        marker = _block(a)
        job.infer(16, 1)
        pending = not marker.query()
        c.set_stream(b.cuda_stream)
        assert pending and marker.query()
        job.close()                                                           # herro_job_free waits for B alone: A must be idle by now
        job = None
        nxt = api.job_from_synth(c, sb, W_SMALL, targets=SMALL)                # the same size: the recycled arenas
        nxt.featurize()
        nxt.infer(16, 1)
        assert _logits_bytes(nxt) == want["small.logits"]
    finally:
        for j in (job, nxt):
            if j is not None:
                j.close()
        c.close()


def test_front_end_calls_on_either_side_of_a_switch():
    rs, codes, lens, names, adapter, pieces = _front_inputs()
    want = _own("front")
    c = _ctx()
    p = m = None
    try:
        a, b = _stream(), _stream()
        c.set_stream(a.cuda_stream)
        PC.load(c, rs)
        marker = _block(a)
        p = c.find_overlap_pairs(**PC.DEFAULTS)
        assert marker.query()
        c.set_stream(b.cuda_stream)
        m = p.align()
        assert PC.pairs_bytes(p) == want["pairs"] and _bytes(_handle_fields(m)) == want["align"]
        c.set_stream(a.cuda_stream)
        c.cut_store(pieces)
        c.set_stream(b.cuda_stream)
        assert _bytes(c.find_overlaps(**PC.DEFAULTS)) == want["cut.find"]
        assert _bytes(c.store_arrays()) == want["cut"]
    finally:
        for x in (p, m):
            if x is not None:
                x.close()
        c.close()
