"""-m gpu: the front end's large-launch paths, reached at a few hundred tokens.

What launch_model_h and launch_front_generic launch follows from the launch's tokens and the compute units of the device (csrc/infer_plan.h front_end_plan;
the rule itself: tests/test_front_plan_host.py).  On a device of 256 units a test-sized launch takes one trip through k_conv_m's stride loop, k_fc_r<4>, and
never k_conv_fc by the rule.  herro_debug_set_front_cu tells the FRONT END ALONE that the device has one or two units, so 65 tokens are a large launch: the
conv loops iterate (k_conv_m on planes and on records, k_conv_w in precision 1), k_fc_r runs at every height (4, 5, 6: the deep pipeline; 7, 8: the shallow
one; 5 and 7: a single row block; partial, full and several tiles each) and the rule picks k_conv_fc.  The encoder stack behind keeps the device's tile plan.

The reference of every case is the same batch on the same context with the hooks off and the two kernels selected: every FC output element sees the same MFMA
chain whatever the tile height, grid or kernel, so the logits must be EQUAL.  One case per height is also held to the dense twin (1e-3, as test_gpu_model.py),
so that equal to a wrong baseline does not pass.  Every case reads back what was launched (herro_debug_front_last) and fails unless it is the launch the case
was written for."""
import numpy as np
import pytest

import gpu_common as G
import test_gpu_conv_fc as CF
from herro_amd import api, model_io, synth

pytestmark = pytest.mark.gpu
TOL = 1e-3


@pytest.fixture(scope="module")
def loaded():
    """(context of its own, the precision herro_load_model chose)"""
    c = api.Context(0)
    path, _ = model_io.default_model_file(G.CACHE)
    c.load_model(path)
    chosen = c.precision()
    yield c, chosen
    c.conv_fc(-1)
    c.front_cu(0)
    c.close()


def _trips(p):
    """trips of k_conv_m's busiest wave (four waves a workgroup, one unit per wave and trip)"""
    return -(-p.conv_units // (4 * p.conv_grid))


_REF = {}


def _forward(c, precision, n_tok, cu, mode):
    """(info, base, what the front end launched) of the batch of n_tok tokens (test_gpu_conv_fc._batch: window ends first, a short window with collate
    padding from 50 tokens on, exact counts).  cu 0, mode 0 is the reference: computed once per batch and precision, never written to afterwards."""
    key = (precision, n_tok)
    if (cu, mode) == (0, 0) and key in _REF:
        return _REF[key]
    short = n_tok >= 50
    bases, quals, lens, idx = CF._batch(n_tok, short)
    assert int(lens.sum()) == n_tok == len(idx) and (not short or (bases[1, 20:] == 11).all())
    c.set_precision(precision)
    try:
        c.front_cu(cu)
        c.conv_fc(mode)
        info, base = c.model_forward(bases, quals, lens, idx)
        ran = c.front_last()
    finally:
        c.front_cu(0)
        c.conv_fc(-1)
    if (cu, mode) == (0, 0):
        if precision >= 4:   # the launch the suite's model tests make: one conv trip, height 4, two kernels
            assert not ran.fused and ran.fc_rows == 64 and ran.fc_grid == -(-n_tok // 64) and ran.conv_units == -(-n_tok * 31 // 16) and _trips(ran) == 1, ran
        else:                # k_conv_w: one tile of 128 pairs per workgroup
            assert ran == api.FrontPlan(False, 0, 0, -(-n_tok * 31 // 128), -(-n_tok * 31 // 128)), ran
        assert np.isfinite(info).all() and np.isfinite(base).all() and float(np.abs(base).max()) > 0
        info.setflags(write=False)
        base.setflags(write=False)
        _REF[key] = (info, base, ran)
    return info, base, ran


def _precision(loaded, which):
    c, chosen = loaded
    p = chosen if which == "chosen" else 4
    assert p >= 4            # the f16 front end
    return c, p


# (compute units, tokens, height in 16-row blocks): for every height one row (4 only), a tile one row short, full tiles, and two or more tiles whose last holds a few rows
HEIGHTS = [(1, 1, 4), (1, 63, 4), (1, 64, 4),
           (1, 65, 5), (1, 79, 5), (1, 80, 5), (1, 129, 5),
           (1, 81, 6), (1, 95, 6), (1, 96, 6), (1, 161, 6), (1, 257, 6),
           (1, 97, 7), (1, 111, 7), (1, 112, 7), (1, 193, 7), (1, 513, 7),
           (1, 113, 8), (1, 127, 8), (1, 128, 8), (1, 225, 8), (1, 256, 8),
           (2, 65, 4), (2, 127, 4), (2, 128, 4), (2, 129, 5), (2, 160, 5), (2, 257, 5), (2, 161, 6), (2, 192, 6), (2, 321, 6),
           (2, 193, 7), (2, 224, 7), (2, 385, 7), (2, 225, 8), (2, 256, 8), (2, 449, 8)]


def test_the_height_cases_cover_every_instance_and_shape():
    for nb in (4, 5, 6, 7, 8):
        mine = [(cu, n) for cu, n, b in HEIGHTS if b == nb]
        rows = 16 * nb
        assert any(n == rows - 1 for _, n in mine) and any(n % rows == 0 for _, n in mine), nb     # a single tile a row short of full; full tiles only
        assert any(n > rows and 0 < n % rows <= rows - 16 for _, n in mine), nb                    # several tiles, in the last one a row block without a row
    for cu, n, nb in HEIGHTS:   # the rule, not the table, decides
        assert api.debug_front_end_plan(n, cu, 0).fc_rows == 16 * nb, (cu, n, nb)


@pytest.mark.parametrize("which", ["chosen", "mode4"])
@pytest.mark.parametrize("cu,n_tok,nb", HEIGHTS)
def test_every_tile_height_gives_the_bits_of_height_4(loaded, cu, n_tok, nb, which):
    c, p = _precision(loaded, which)
    i0, b0, _ = _forward(c, p, n_tok, 0, 0)
    i1, b1, ran = _forward(c, p, n_tok, cu, 0)
    assert ran == api.debug_front_end_plan(n_tok, cu, 0), ran
    assert not ran.fused and ran.fc_rows == 16 * nb and ran.fc_grid == -(-n_tok // (16 * nb)) and ran.conv_grid <= 3 * cu, ran
    assert np.array_equal(i0, i1) and np.array_equal(b0, b1)


@pytest.mark.parametrize("which", ["chosen", "mode4"])
@pytest.mark.parametrize("n_tok,nb", [(64, 4), (129, 5), (257, 6), (513, 7), (225, 8)])
def test_one_case_per_height_against_the_twin(loaded, n_tok, nb, which):
    import model_ref as MR
    c, p = _precision(loaded, which)
    info, base, ran = _forward(c, p, n_tok, 1, 0)
    assert not ran.fused and ran.fc_rows == 16 * nb and _trips(ran) >= 2, ran
    bases, quals, lens, idx = CF._batch(n_tok, n_tok >= 50)
    ti, tb = MR.run_batch(G.twin(), bases, quals, lens, idx)
    assert info.shape == ti.shape and base.shape == tb.shape
    err = max(float(np.abs(info - ti).max()), float(np.abs(base - tb).max()))
    print(f"height {nb}, {n_tok} tokens, precision {p}: max abs logit error against the twin {err:.3e}")
    assert err <= TOL


# 1953 pairs (63 tokens) are no multiple of 16 and 123 units no multiple of the sweep of 12; 192 tokens are 31 sweeps exactly; 513 tokens 83 trips
@pytest.mark.parametrize("which", ["chosen", "mode4"])
@pytest.mark.parametrize("n_tok,trips", [(17, 3), (63, 11), (100, 17), (192, 31), (513, 83)])
def test_conv_loop_on_planes(loaded, n_tok, trips, which):
    c, p = _precision(loaded, which)
    i0, b0, _ = _forward(c, p, n_tok, 0, 0)
    i1, b1, ran = _forward(c, p, n_tok, 1, 0)
    assert not ran.fused and ran.conv_grid == 3 and ran.conv_units == -(-n_tok * 31 // 16) and _trips(ran) == trips >= 2, ran
    assert np.array_equal(i0, i1) and np.array_equal(b0, b1)


@pytest.mark.parametrize("n_tok,grid,units", [(1, 1, 2), (3, 2, 6)])
def test_conv_waves_without_a_unit(loaded, n_tok, grid, units):
    c, p = _precision(loaded, "chosen")
    i0, b0, _ = _forward(c, p, n_tok, 0, 0)
    i1, b1, ran = _forward(c, p, n_tok, 1, 0)
    assert (ran.conv_grid, ran.conv_units) == (grid, units) and units < 4 * grid, ran
    assert np.array_equal(i0, i1) and np.array_equal(b0, b1)


# k_conv_w (precision 1): tiles of 128 pairs, two workgroups on one unit.  5 tokens: one tile each; 63: 8 trips; 257: 63 tiles, 32 trips and 31
@pytest.mark.parametrize("n_tok,tiles", [(1, 1), (5, 2), (63, 16), (257, 63)])
def test_conv_w_loop_on_planes(loaded, n_tok, tiles):
    c, _ = loaded
    i0, b0, _ = _forward(c, 1, n_tok, 0, 0)
    i1, b1, ran = _forward(c, 1, n_tok, 1, 0)
    assert ran == api.FrontPlan(False, 0, 0, min(tiles, 2), tiles), ran
    assert np.array_equal(i0, i1) and np.array_equal(b0, b1)


@pytest.mark.parametrize("n_tok,fused", [(90, False), (91, True), (128, True), (129, False), (216, False), (217, True), (256, True), (257, False)])
def test_the_rule_picks_the_kernel_and_changes_no_bit(loaded, n_tok, fused):
    c, p = _precision(loaded, "chosen")
    i0, b0, _ = _forward(c, p, n_tok, 0, 0)
    i1, b1, ran = _forward(c, p, n_tok, 1, -1)
    assert ran == api.debug_front_end_plan(n_tok, 1, -1) and ran.fused == fused, ran
    if fused:
        assert ran == api.FrontPlan(True, 128, -(-n_tok // 128), 0, 0), ran
    else:
        assert ran.fc_rows > 64 and _trips(ran) >= 2, ran
    assert np.array_equal(i0, i1) and np.array_equal(b0, b1)


# ---- jobs: 16-byte records from k_rfq (a job on its own) and from k_rows' own gather (behind a pending job) ------------------------------------------------
# the two W 256 jobs of test_gpu_conv_fc.py (78 and 135 informative rows) and one whose total the rule gives to k_conv_fc on one unit and on two
AUTO = dict(n=3, tl=700, ov=16, seed=synth.SEED + 3403, kw=dict(flank_min=30, flank_max=60, p_snp=0.1, p_ins=0.02))   # 238 informative rows


def _gen(name):
    cs = AUTO if name == "auto" else CF.JOBS[name]
    return synth.generate(cs["n"], cs["tl"], cs["ov"], seed=cs["seed"], **cs["kw"])


def test_the_jobs_have_the_token_counts_the_tests_need():
    tot = {name: sum(CF._informative_rows(_gen(name))) for name in ("alone", "pipelined", "auto")}
    for name in ("alone", "pipelined"):                     # several conv trips on one unit, two kernels by the rule
        p = api.debug_front_end_plan(tot[name], 1, -1)
        assert not p.fused and _trips(p) >= 3, (name, tot, p)
    assert any(t * 31 % 16 for t in tot.values()), tot
    for cu in (1, 2):                                       # one round of two tiles on two units, two rounds on one
        assert api.debug_front_end_plan(tot["auto"], cu, -1) == api.FrontPlan(True, 128, 2, 0, 0), tot
    assert tot["auto"] % 128 and tot["auto"] % 16, tot


def _job_run(c, job, ids, sb, cu, mode, pipelined):
    try:
        c.front_cu(cu)
        logits, fasta, gather = CF._run(c, job, ids, mode, pipelined, sb)
        return logits, fasta, gather, c.front_last()
    finally:
        c.front_cu(0)
        c.conv_fc(-1)


@pytest.mark.parametrize("precision", ["chosen", 1])
@pytest.mark.parametrize("name", ["alone", "pipelined"])
def test_conv_loops_on_records_from_both_gathers(loaded, name, precision):
    c, chosen = loaded
    sb = _gen(name)
    n = sum(CF._informative_rows(sb))
    c.set_precision(chosen if precision == "chosen" else 1)
    c.featurize_planes(False)
    G.load_synth(c, sb)
    ids = [f"read{t}" for t in range(sb.n_targets)]
    job = api.job_from_synth(c, sb, CF.W_JOB)
    try:
        pipe = name == "pipelined"
        ref, fa_ref, g0, ran0 = _job_run(c, job, ids, sb, 0, 0, pipe)
        got, fa_got, g1, ran = _job_run(c, job, ids, sb, 1, 0, pipe)
        if precision == "chosen":
            assert c.precision() >= 4 and g0 == g1 == pipe      # k_rfq's records behind a job on its own, k_rows' own for a caller that pipelines
            assert not ran0.fused and ran0.fc_rows == 64 and _trips(ran0) == 1, ran0
            assert ran == api.debug_front_end_plan(n, 1, 0) and ran.conv_grid == 3 and _trips(ran) >= 3 and ran.fc_rows == 80, ran
        else:
            tiles = -(-n * 31 // 128)
            assert ran0 == api.FrontPlan(False, 0, 0, tiles, tiles) and ran == api.FrontPlan(False, 0, 0, 2, tiles) and tiles >= 4, (ran0, ran)
        assert CF._same(ref, got, name) == n
        assert fa_got == fa_ref
    finally:
        job.close()


@pytest.mark.parametrize("cu,pipelined", [(1, False), (1, True), (2, False)])
def test_a_job_the_rule_gives_to_the_fused_kernel(loaded, cu, pipelined):
    c, chosen = loaded
    sb = _gen("auto")
    n = sum(CF._informative_rows(sb))
    c.set_precision(chosen)
    assert c.precision() >= 4
    c.featurize_planes(False)
    G.load_synth(c, sb)
    ids = [f"read{t}" for t in range(sb.n_targets)]
    job = api.job_from_synth(c, sb, CF.W_JOB)
    try:
        ref, fa_ref, g0, ran0 = _job_run(c, job, ids, sb, 0, 0, pipelined)
        got, fa_got, g1, ran = _job_run(c, job, ids, sb, cu, -1, pipelined)
        assert g0 == g1 == pipelined
        assert not ran0.fused and ran0.fc_rows == 64 and _trips(ran0) == 1, ran0
        assert ran == api.FrontPlan(True, 128, -(-n // 128), 0, 0) and ran.fc_grid == 2, ran
        assert CF._same(ref, got, "auto") == n
        assert fa_got == fa_ref
    finally:
        job.close()
