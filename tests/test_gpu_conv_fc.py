"""-m gpu: the two front ends of the f16 model give the same bits.

k_conv_fc (csrc/model_h.hip) runs the conv stack and the FC projection in one kernel, with the conv output in LDS; k_conv_m + k_fc_r run them as
two kernels with that output in HBM.  Every element of the FC output sees the same MFMAs in the same order on both paths, so the logits must be
equal bit for bit: herro_debug_set_conv_fc(0) against (1) at the token counts where a clamp, a store guard or the second tile of the fused
kernel can go wrong, on the stand-alone forward (cells from the planes) and on jobs (16-byte records from k_rfq and from k_rows' own gather);
a model whose conv stack the f16 kernels do not serve keeps its path whatever the switch says; and the automatic choice changes no bit (at these sizes it
takes the two kernels on a real device: launches the rule itself gives to k_conv_fc are in test_gpu_front_plan.py)."""
import numpy as np
import pytest

import gpu_common as G
import oracle_lib as O
import rf_cases as R
from herro_amd import api, model_io, synth

pytestmark = pytest.mark.gpu

L_WIN = 48                                   # rows of a window of the stand-alone batches
TOKENS = [1, 15, 16, 17, 127, 128, 129, 257]  # one under / at / over a block of 16 pairs and a tile of 128 tokens; 257: a third tile of one token


@pytest.fixture(scope="module")
def loaded():
    """(context of its own, the precision herro_load_model chose)"""
    c = api.Context(0)
    path, _ = model_io.default_model_file(G.CACHE)
    c.load_model(path)
    chosen = c.precision()
    yield c, chosen
    c.conv_fc(-1)
    c.close()


def _batch(n_tok, short):
    """Dense planes [B, L_WIN, 31] with n_tok informative rows in all.  Rows 0, 1, L - 2, L - 1 come first in every window (fields that reach outside [0, lmax):
    zero rows of the convolution).  short: window 1 has real cells in rows [0, 20) only and the collate padding (token 11, quality 126) behind them, and informative
    rows on both sides of that edge, and fewer informative rows than its neighbours."""
    g = np.random.default_rng(0x5be0cd19 + n_tok + 1000 * short)
    per = 40
    lens = []
    left = n_tok
    while left > 0:
        k = min(per, left)
        if short and len(lens) == 1:
            k = min(9, left)
        lens.append(k)
        left -= k
    B = len(lens)
    bases = g.integers(0, 11, (B, L_WIN, 31)).astype(np.uint8)
    quals = g.integers(33, 94, (B, L_WIN, 31)).astype(np.uint8)
    if short and B > 1:
        bases[1, 20:] = 11
        quals[1, 20:] = 126
    idx = []
    for b, k in enumerate(lens):
        first = [0, 1, L_WIN - 2, L_WIN - 1, 18, 19, 20, 21, 22]          # the window's ends; the rows around the padding edge of the short window
        rest = [r for r in g.permutation(L_WIN).tolist() if r not in first]
        idx += sorted((first + rest)[:k])
    return bases, quals, np.array(lens, np.int32), np.array(idx, np.int32)


@pytest.mark.parametrize("which", ["chosen", "mode4"])
@pytest.mark.parametrize("n_tok", TOKENS + ["129_short"])
def test_forward_bits_at_exact_token_counts(loaded, n_tok, which):
    c, chosen = loaded
    short = isinstance(n_tok, str)
    n = 129 if short else n_tok
    bases, quals, lens, idx = _batch(n, short)
    assert int(lens.sum()) == n and len(idx) == n
    if short:
        assert lens[1] < lens[0] and (bases[1, 20:] == 11).all() and (quals[1, 20:] == 126).all()
        assert {18, 19, 20, 21, 22} <= set(idx[lens[0]:lens[0] + lens[1]].tolist())
    c.set_precision(chosen if which == "chosen" else 4)
    assert c.precision() >= 4          # the f16 front end is what the switch selects between
    try:
        c.conv_fc(0)
        i0, b0 = c.model_forward(bases, quals, lens, idx)
        c.conv_fc(1)
        i1, b1 = c.model_forward(bases, quals, lens, idx)
    finally:
        c.conv_fc(-1)
    assert np.isfinite(i0).all() and np.isfinite(b0).all() and float(np.abs(b0).max()) > 0
    assert np.array_equal(i0, i1) and np.array_equal(b0, b1)


# two small jobs at W 256
JOBS = {
    "alone": dict(n=2, tl=600, ov=12, seed=synth.SEED + 3301, kw=dict(flank_min=30, flank_max=60, p_sub=0.03, p_ins=0.03, p_del=0.03, p_partial=0.2, p_snp=0.05)),   # 78 informative rows
    "pipelined": dict(n=2, tl=700, ov=16, seed=synth.SEED + 3302, kw=dict(flank_min=30, flank_max=60, p_snp=0.1, p_ins=0.02)),                                       # 135: a second tile of 7 tokens
}
W_JOB = 256


def _informative_rows(sb):
    """informative rows of the job's windows, from the oracle: no device"""
    store = O.store_from_synth(sb)
    n = []
    for t in range(sb.n_targets):
        rid, rows, cigs = O.target_alignments(sb, t)
        res = store.extract_features(rid, rows, cigs, W_JOB)
        n += [len(res.window(wi).sup_pos) for wi in range(len(res))]
    return n


def _gen(name):
    cs = JOBS[name]
    return synth.generate(cs["n"], cs["tl"], cs["ov"], seed=cs["seed"], **cs["kw"])


def test_the_jobs_have_the_token_counts_the_tests_need():
    tot = {name: sum(_informative_rows(_gen(name))) for name in JOBS}
    assert all(0 < t < 300 for t in tot.values()), tot
    assert any(t % 16 for t in tot.values()), tot


def _run(c, job, ids, mode, pipelined, sb):
    other = None
    try:
        c.conv_fc(mode)
        if pipelined:
            other = api.job_from_synth(c, sb, W_JOB, targets=[0])
            other.featurize()                      # a pending job: k_rows gathers the receptive fields itself
        job.featurize()
        job.infer(64, 1)
        fused_gather = job.rf_fused()
        job.consensus()
        logits = [job.logits(w) if job.info(w).n_supported else None for w in range(job.n_windows)]
        logits = [None if x is None else (x[0].copy(), x[1].copy()) for x in logits]
        return logits, job.fasta(ids), fused_gather
    finally:
        c.conv_fc(-1)
        if other is not None:
            other.close()


def _same(a, b, tag):
    assert len(a) == len(b) > 0, tag
    n = 0
    for w, (x, y) in enumerate(zip(a, b)):
        assert (x is None) == (y is None), (tag, w)
        if x is not None:
            assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]), (tag, w)
            n += len(x[0])
    return n


@pytest.mark.parametrize("name", list(JOBS))
def test_job_bits_records_from_both_gathers(loaded, name):
    c, chosen = loaded
    sb = _gen(name)
    rows = _informative_rows(sb)
    assert 0 < sum(rows) < 300, rows
    if name == "pipelined":
        assert sum(rows) % 16 or sum(_informative_rows(_gen("alone"))) % 16
    c.set_precision(chosen)
    c.featurize_planes(False)
    G.load_synth(c, sb)
    ids = [f"read{t}" for t in range(sb.n_targets)]
    job = api.job_from_synth(c, sb, W_JOB)
    try:
        pipe = name == "pipelined"
        two, fa_two, g0 = _run(c, job, ids, 0, pipe, sb)
        one, fa_one, g1 = _run(c, job, ids, 1, pipe, sb)
        assert g0 == g1 == pipe              # k_rfq's records behind a job on its own, k_rows' own for a caller that pipelines
        assert _same(two, one, name) == sum(rows)
        assert fa_one == fa_two
        if pipe:
            auto, fa_auto, _ = _run(c, job, ids, -1, pipe, sb)      # whichever path the rule picks
            assert _same(two, auto, "automatic") == sum(rows) and fa_auto == fa_two
    finally:
        job.close()


@pytest.mark.parametrize("precision", ["chosen", 1])
def test_a_model_the_f16_conv_kernels_do_not_serve_keeps_its_path(tmp_path, precision):
    path, _, _ = R.export_model("kw1_f16", tmp_path)
    c = api.Context(0)
    try:
        c.load_model(path)
        if precision != "chosen":
            c.set_precision(precision)
        sb = R.generate("edges")
        G.load_synth(c, sb)
        job = api.job_from_synth(c, sb, R.W)
        ids = [f"read{t}" for t in range(sb.n_targets)]
        two, fa_two, _ = _run(c, job, ids, 0, False, sb)
        one, fa_one, _ = _run(c, job, ids, 1, False, sb)
        assert _same(two, one, "kw1_f16") > 0 and fa_one == fa_two
        job.close()
    finally:
        c.close()
