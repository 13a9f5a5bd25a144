"""-m gpu: jobs (featurize -> infer -> consensus) behind models whose receptive field is not the default model's five rows.

herro_job_featurize and herro_job_infer pick their code by half = 2 * (kw / 2): a kw 1 model (one row) reads compact records gathered with
half 0 — never by k_rows; a kw 5 / 7 model (9 / 13 rows) reads the job's own planes, which a lean featurize only fills when infer asks
(k_layout<true> + k_tokens) and whose qualities k_quals<false> writes around the informative rows only, with the collate padding reproduced by
addressing.  The stand-alone entry (herro_model_forward, dense [B, L, 31] planes) never takes any of that.  rf_cases.py has the models, the
inputs and the census of what they reach (held by test_rf_cases.py without a device).

References: the dense fp32 twin on explicit batches collated from the ORACLE's windows in the job's own grouping (1e-3 for a mode a caller
can select — the contract; 1e-4 for mode 0, as test_model_forward_vs_twin holds it), the oracle's cells byte for byte, and the job against
itself bit for bit where two routes must read the same cells."""
import time
from types import SimpleNamespace

import numpy as np
import pytest

import gpu_common as G
import oracle_lib as O
import rf_cases as R
from herro_amd import api, model_io
from test_gpu_lean import records_against_the_oracles_cells

pytestmark = pytest.mark.gpu
TOL, TOL_F32 = 1e-3, 1e-4
WIDE = [n for n in R.MODELS if R.half_of(n) > 2]       # the planes
POINT = [n for n in R.MODELS if R.half_of(n) == 0]     # compact records of one row


@pytest.fixture(scope="module")
def zoo(tmp_path_factory):
    """name -> the model of rf_cases.MODELS in a context of its own (loaded once per module, closed behind the last test)"""
    d = tmp_path_factory.mktemp("rf_models")
    made = {}

    def get(name):
        if name not in made:
            path, raw, hp = R.export_model(name, d)
            c = api.Context(0)
            t0 = time.time()
            c.load_model(path)
            print(f"{name}: loaded and calibrated in {time.time() - t0:.2f} s -> mode {c.precision()}")
            made[name] = SimpleNamespace(c=c, path=path, raw=raw, hp=hp, chosen=c.precision())
        m = made[name]
        m.c.set_precision(m.chosen)
        m.c.featurize_planes(False)
        return m

    yield get
    for m in made.values():
        m.c.close()


def _job(c, inp, seed_shift=0, targets=None):
    sb = R.generate(inp, seed_shift)
    return api.job_from_synth(c, sb, R.W, targets=targets)


def _logits(job):
    """[(info, base) or None per window] of the job's last model pass"""
    return [job.logits(w) if job.info(w).n_supported else None for w in range(job.n_windows)]


def _same_bits(a, b, tag):
    assert len(a) == len(b), tag
    for w, (x, y) in enumerate(zip(a, b)):
        assert (x is None) == (y is None), (tag, w)
        if x is not None:
            assert np.array_equal(x[0].view(np.uint32), y[0].view(np.uint32)) and np.array_equal(x[1].view(np.uint32), y[1].view(np.uint32)), \
                (tag, w, float(np.abs(x[1] - y[1]).max()))


def _is_the_oracles_job(job, wins):
    assert job.n_windows == len(wins)
    for w, m in enumerate(wins):
        wi = job.info(w)
        assert (wi.length, wi.n_supported) == (m.len, m.n_sup), (w, wi.length, wi.n_supported, m.len, m.n_sup)


@pytest.mark.parametrize("name", list(R.MODELS))
def test_job_logits_against_the_dense_twin(zoo, name):
    """(i) every batch of both inputs, both batch sizes, both groupings, collated from the oracle's windows (11 / 126 up to the batch's longest
    window, rows from get_target_indices) through the twin, against the job's logits — in the mode the load chose, mode 1 and mode 0.  Mode 0
    is the sharp one: a receptive-field row taken from the wrong place moves a logit by far more than 1e-4."""
    import model_ref as MR
    m = zoo(name)
    c = m.c
    kw, rows, f16 = R.MODELS[name][0]["kw"], R.MODELS[name][1], R.MODELS[name][2]
    d = c.describe_model()
    assert f"conv kw {kw} " in d and f"receptive field of an informative row: {rows} rows" in d, d
    if f16:
        assert "in front of the f16 MFMA stack" in d and m.chosen >= 4, d
    else:
        assert "mode 1" in d and m.chosen == 1, d
        with pytest.raises(api.HerroError):
            c.set_precision(4)
    twin = MR.build(m.raw, m.hp)
    modes = [m.chosen] + [p for p in (1, 0) if p != m.chosen]
    worst = {p: 0.0 for p in modes}
    bad = []
    n_rows = 0
    try:
        for inp in R.INPUTS:
            wins, off, _ = R.windows(inp)
            G.load_synth(c, R.generate(inp))
            job = _job(c, inp)
            try:
                for batch in R.BATCHES:
                    for mode in R.MODES:
                        ref = {}
                        for mem, _ in R.groups(wins, off, batch, mode):
                            bases, quals, lens, flat = R.collate([wins[w] for w in mem])
                            ti, tb = MR.run_batch(twin, bases, quals, lens, flat)
                            o = 0
                            for w, k in zip(mem, lens):
                                ref[w] = (ti[o:o + k], tb[o:o + k])
                                o += k
                        for p in modes:
                            c.set_precision(p)
                            job.featurize()
                            job.infer(batch, mode)
                            _is_the_oracles_job(job, wins)
                            err = 0.0
                            for w, (ti, tb) in ref.items():
                                gi, gb = job.logits(w)
                                err = max(err, float(np.abs(gi - ti).max()), float(np.abs(gb - tb).max()))
                                n_rows += len(ti)
                            print(f"{name} {inp} batch {batch} mode {mode} precision {p}: max abs logit error {err:.3e}")
                            worst[p] = max(worst[p], err)
                            if not err <= (TOL_F32 if p == 0 else TOL):
                                bad.append((inp, batch, mode, p, err))
            finally:
                job.close()
    finally:
        c.set_precision(m.chosen)
    print(f"{name}: max abs logit error per precision mode {({p: f'{e:.3e}' for p, e in worst.items()})} over {n_rows} rows")
    assert n_rows > 0 and not bad, bad


@pytest.mark.parametrize("name", POINT)
def test_one_row_records_are_the_oracles_cells(zoo, name):
    """(ii) kw 1: the records the model reads (k_rfq<5> with half 0; read out before anything asks for planes) against the oracle's cells, byte
    for byte; a pipelining caller gets the same records and the same logits — k_rows gathers for five-row fields only."""
    m = zoo(name)
    c = m.c
    n_cells = 0
    for inp in R.INPUTS:
        wins, _, _ = R.windows(inp)
        G.load_synth(c, R.generate(inp))
        job, other = _job(c, inp), None
        try:
            job.featurize()
            job.infer(5, 1)
            assert not job.rf_fused()
            recs = [job.rf_records(w) for w in range(job.n_windows)]
            lone = _logits(job)
            _is_the_oracles_job(job, wins)
            for w, mw in enumerate(wins):
                n_cells += records_against_the_oracles_cells(recs[w], mw.ow, (name, inp, w), half=0)
            other = _job(c, inp, targets=[0])
            other.featurize()                      # a pending job: the caller pipelines
            job.featurize()
            job.infer(5, 1)
            assert job.rf_fused() is False
            for w in range(job.n_windows):
                assert np.array_equal(job.rf_records(w), recs[w]), (name, inp, w)
            _same_bits(_logits(job), lone, (name, inp, "pipelined"))
        finally:
            if other is not None:
                other.close()
            job.close()
    assert n_cells > 0


def _fill_arenas_with_foreign_bytes(c):
    """Jobs of other data, served on the planes path with their complete planes written, then closed: their arenas go to the context's free
    list, and the next jobs of that size or less start on those bytes instead of on whatever a fresh allocation holds."""
    c.featurize_planes(True)
    try:
        for inp in R.INPUTS:                      # the same shapes from other seeds, two of each: the lean and the planes job below are open together
            G.load_synth(c, R.generate(inp, 1))
            jobs = [_job(c, inp, 1) for _ in range(2)]
            try:
                for j in jobs:
                    j.featurize()
                    j.infer(5, 1)
                    j.window(0)
            finally:
                for j in jobs:
                    j.close()
    finally:
        c.featurize_planes(False)


@pytest.mark.parametrize("name", WIDE)
def test_partially_filled_planes_against_complete_ones(zoo, name):
    """(iii) kw 5 / 7: infer behind a lean featurize fills token planes and writes qualities around the informative rows only.  On an arena
    that served other jobs before (an unwritten cell holds foreign bytes), the logits of that pass equal, to the bit, those of a pass over
    the complete planes (materialised by job.window and held to the oracle bit for bit), and those of a fresh featurize after that — on the
    lean path and on the planes path.  `dense` has the window of 91 informative rows: two passes of k_quals<false> at half 6."""
    m = zoo(name)
    c = m.c
    _fill_arenas_with_foreign_bytes(c)
    for inp in R.INPUTS:
        sb = R.generate(inp)
        store = O.store_from_synth(sb)
        G.load_synth(c, sb)
        jobs, first = [], {}
        try:
            for planes in (False, True):
                c.featurize_planes(planes)
                job = _job(c, inp)          # (the previous one stays open: this one cannot get its arena back)
                jobs.append(job)
                job.featurize()
                job.infer(5, 1)
                first[planes] = _logits(job)
                assert sum(x is not None for x in first[planes]) >= 4
                assert G.compare_features(job, sb, store, R.W) == len(R.windows(inp)[0])
                job.infer(5, 1)
                _same_bits(_logits(job), first[planes], (name, inp, planes, "complete planes"))
                job.featurize()
                job.infer(5, 1)
                _same_bits(_logits(job), first[planes], (name, inp, planes, "featurized again"))
            _same_bits(first[False], first[True], (name, inp, "lean against planes"))
        finally:
            c.featurize_planes(False)
            for j in jobs:
                j.close()


@pytest.mark.parametrize("name", list(R.MODELS))
def test_job_against_the_stand_alone_entry(zoo, name):
    """(iv) every batch once more through herro_model_forward, as dense planes collated from the job's own windows — in modes 0 and 1 ONLY.
    kw 5 / 7 read planes through the same front-end kernels on both routes and only the addressing differs: mode 0, and mode 1 on the
    layer-by-layer kernels, equal to the bit.  kw 1 reads compact records against planes, the same arithmetic in different kernels: 1e-4,
    as test_model_forward_tiling_edges holds such pairs.  Mode 1 with the f16 stack's encoder shapes runs the fused bf16x3 stack (k_layers),
    which is not bit-stable between the two routes, and not because of the front end: a window's place in its 64-token tile follows from
    what shares the launch (plan_tiles), and the tile's attention sums over 16-key blocks aligned to the tile, so the same window at
    another offset rounds differently — held to 1e-4 like the pair above (measured 6e-6).
    The f16 tier the load chose is NOT compared here.  The same tile effect is there of the size of the tier's own rounding (measured between
    the routes: 4.6e-5 for kw5_f16, up to 1.4e-4 for kw1_f16 in mode 5), so neither bit-equality nor 1e-4 can be asked of it, and any bound
    that holds says less than the 1e-3 against the twin that test_job_logits_against_the_dense_twin asks of the job's f16 logits; the
    addressing this check is about is the front end's, which is the same code in every mode."""
    m = zoo(name)
    c = m.c
    wide, f16 = name in WIDE, R.MODELS[name][2]
    worst = {}
    n_rows = 0
    try:
        for inp in R.INPUTS:
            wins, off, _ = R.windows(inp)
            G.load_synth(c, R.generate(inp))
            job = _job(c, inp)
            try:
                for batch, mode in ((3, 0), (5, 1)):
                    for p in (0, 1):
                        bits = wide and (p == 0 or not f16)
                        c.set_precision(p)
                        job.featurize()
                        job.infer(batch, mode)
                        got = _logits(job)          # (before anything asks for the planes)
                        gws = {w: job.window(w, encoded=True) for w in range(job.n_windows) if wins[w].n_sup}
                        for mem, _ in R.groups(wins, off, batch, mode):
                            lmax = max(gws[w].info.length for w in mem)
                            bases = np.full((len(mem), lmax, 31), 11, np.uint8)
                            quals = np.full((len(mem), lmax, 31), 126, np.uint8)
                            lens, flat = [], []
                            for k, w in enumerate(mem):
                                g = gws[w]
                                bases[k, :g.info.length] = g.bases
                                quals[k, :g.info.length] = g.quals
                                tidx = np.flatnonzero(g.bases[:, 0] != 4)
                                lens.append(len(g.sup_pos))
                                flat.extend((tidx[g.sup_pos] + g.sup_ins).tolist())
                            si, sbase = c.model_forward(bases, quals, np.array(lens, np.int32), np.array(flat, np.int32))
                            o = 0
                            for k, w in enumerate(mem):
                                gi, gb = got[w]
                                ai, ab = si[o:o + lens[k]], sbase[o:o + lens[k]]
                                o += lens[k]
                                n_rows += lens[k]
                                e = max(float(np.abs(gi - ai).max()), float(np.abs(gb - ab).max()))
                                worst[p] = max(worst.get(p, 0.0), e)
                                if bits:
                                    assert np.array_equal(gi.view(np.uint32), ai.view(np.uint32)) and np.array_equal(gb.view(np.uint32), ab.view(np.uint32)), \
                                        (name, inp, batch, mode, p, w, e)
                                else:
                                    assert e <= TOL_F32, (name, inp, batch, mode, p, w, e)
            finally:
                job.close()
    finally:
        c.set_precision(m.chosen)
        print(f"{name}: job against herro_model_forward, max abs difference per precision mode {({p: f'{e:.3e}' for p, e in worst.items()})} over {n_rows} rows")
    assert n_rows > 0


OUT_OF_STEP = [   # (model at featurize, model at infer, another featurized job is pending)
    ("default", "kw5_f16", False),     # records gathered for five rows, the model wants planes
    ("default", "kw5_f16", True),
    ("default", "kw1_f16", False),     # k_rfq's early gather carries half 2
    ("default", "kw1_f16", True),      # ... and so does k_rows' fused one
    ("kw1_f16", "default", False),     # an early gather with half 0
    ("kw1_f16", "default", True),
    ("kw5_f16", "default", False),     # nothing gathered at featurize
    (None, "default", False),          # featurized before any model was loaded
    (None, "kw1_f16", False),
    (None, "kw5_f16", False),
]


@pytest.mark.parametrize("first,second,pipelined", OUT_OF_STEP)
def test_model_loaded_between_featurize_and_infer(tmp_path, first, second, pipelined):
    """(v) the gathers are keyed to the half width current at featurize time: a job featurized under one model (or none) and inferred under
    another must give the logits, to the bit, of a job featurized and inferred under the second."""
    def path(n):
        return model_io.default_model_file(G.CACHE)[0] if n == "default" else R.export_model(n, tmp_path)[0]
    sb = R.generate("edges")
    c = api.Context(0)
    job = other = fresh = None
    try:
        G.load_synth(c, sb)
        if first is not None:
            c.load_model(path(first))
        job = _job(c, "edges")
        if pipelined:
            other = _job(c, "edges", targets=[0])
            other.featurize()
        job.featurize()
        c.load_model(path(second))
        job.infer(5, 1)
        got = _logits(job)
        fused = job.rf_fused()
        if other is not None:
            other.close()
            other = None
        fresh = _job(c, "edges")
        fresh.featurize()
        fresh.infer(5, 1)
        want = _logits(fresh)
        assert sum(x is not None for x in want) > 5
        _same_bits(got, want, (first, second, pipelined))
        assert not fused                       # what k_rows gathered, if anything, was for another field
    finally:
        for j in (job, other, fresh):
            if j is not None:
                j.close()
        c.close()


def test_consensus_behind_a_nine_row_model(zoo):
    """(vi) kw5_f16: consensus on the device and the FASTA of every target against the oracle's decode of the job's own logits."""
    m = zoo("kw5_f16")
    c = m.c
    some = False
    for inp in R.INPUTS:
        sb = R.generate(inp)
        wins, off, results = R.windows(inp)
        G.load_synth(c, sb)
        job = _job(c, inp)
        try:
            job.featurize()
            job.infer(3, 0)
            wants = []
            for t, (rid, res) in enumerate(results):
                lg = [job.logits(w)[1] for w in range(off[t], off[t + 1]) if wins[w].n_sup]
                want = res.consensus_fasta(np.concatenate(lg) if lg else np.zeros((0, 5), np.float32))
                assert job.consensus_fasta(t, sb.read_name(rid)) == want, (inp, t)      # host decode of the device planes + logits
                wants.append((t, rid, want))
            job.consensus()                                                              # consensus.rs on the device
            for t, rid, want in wants:
                assert job.consensus_fasta(t, sb.read_name(rid)) == want, (inp, t, "device")
            some = some or any(w for _, _, w in wants)
        finally:
            job.close()
    assert some
