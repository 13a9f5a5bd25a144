"""-m gpu: the feature kernels where their packed fields end and their fallbacks begin (width_cases.py), against the oracle.

The cases: a slice with a query span of 2^16 (k_cols scans target and query advance separately) that is dropped for its 66 000-base insertion (the
event's 16-bit lengths are clamped) at the smallest and at a large instantiation of k_cols; such a slice that is KEPT (1300 insertions of 50 bases);
a column whose directory words fit in front and are flagged behind (4 200 events in one slice: k_rfq counts for exactly the flagged words, with no
environment switch); the largest window the format admits (8192 positions of 51 rows, 408 tiles, every 6-bit field of sup_nr at its maximum).
test_width_cases.py proves without a device that each case reaches its switch and that no other data set of the suite does.

On each case, what test_gpu_capacity.py checks on its cases, with its helpers: the receptive-field records of the lean path (k_rfq behind a job on its own,
k_rows for a pipelining caller), read out before anything asks for the planes, against cells cut from the oracle's [L', 31] arrays; the lean path equal
to the planes path (informative rows, logits bit for bit, FASTA); features bit-exact on every window; the three decoders equal to the oracle decoding
the job's own logits; logits within 1e-3 of the fp32 twin.  Then the device-built descriptors against the host build, and the directory words of a
mixed column read back."""
import numpy as np
import pytest

import gpu_common as G
import test_gpu_capacity as Cap
import width_cases as Wc
from herro_amd import api, model_io
from test_gpu_cigar_scan import _same_jobs
from test_gpu_lean import records_against_the_oracles_cells

pytestmark = pytest.mark.gpu
TOL = Cap.TOL   # the existing contract of the shipped precision against the fp32 twin
_CASE = {}


def _case(name):
    """(SynthBatch, W, oracle store, per target (rid, FeatResult, [OracleWindow])): built once, shared by the tests, left unchanged"""
    if name not in _CASE:
        sb, W = Wc.build(name)
        _CASE[name] = (sb, W) + Cap._oracle(sb, W)
    return _CASE[name]


def _twin_errors(orc, logits):
    """Cap._twin_errors with the rows no receptive field reaches cut out of the twin's input (width_cases.compact_twin_inputs, held equal to the uncut
    batch by test_width_cases.py): the same batch of all informative windows, the same collate padding, the same logits."""
    import model_ref as MR
    wins, w = [], 0
    for _, _, ows in orc:
        for ow in ows:
            if len(ow.sup_pos):
                wins.append((w, ow))
            w += 1
    assert 0 < len(wins) <= 64
    inp = []
    for _, ow in wins:
        enc = Wc.TOKMAP[ow.bases]
        tidx = np.flatnonzero(enc[:, 0] != 4)
        inp.append((enc, ow.quals, tidx[ow.sup_pos.astype(np.int64)] + ow.sup_ins))
    bases, quals, lens, idx, pos = Wc.compact_twin_inputs(inp, 2 * (model_io.Hyper().kw // 2))
    ti, tb = MR.run_batch(Cap._twin(), bases, quals, lens, idx, gemm=True, positions_flat=pos)
    e_info = e_base = 0.0
    o = 0
    for k, (w, _) in enumerate(wins):
        gi, gb = logits[w]
        e_info = max(e_info, float(np.abs(gi - ti[o:o + lens[k]]).max()))
        e_base = max(e_base, float(np.abs(gb - tb[o:o + lens[k]]).max()))
        o += lens[k]
    return e_info, e_base


@pytest.mark.parametrize("name", list(Wc.CASES))
def test_width_case_against_the_oracle(name):
    lim = Wc.limits()
    sb, W, store, orc = _case(name)
    ows = [ow for _, _, wins in orc for ow in wins]
    c = G.ctx()
    G.load_synth(c, sb)
    ids = [sb.read_name(rid) for rid, _, _ in orc]
    job = api.job_from_synth(c, sb, W)
    assert job.skipped() == (0, 0) and job.n_windows == len(ows)
    other = None
    n_cells = 0
    try:
        # ---- lean path, a job on its own: k_rfq's records, read out before anything asks for a token plane
        c.featurize_planes(False)
        job.featurize()
        job.infer(64, 1)
        assert not job.rf_fused()
        for w, ow in enumerate(ows):
            n_cells += records_against_the_oracles_cells(job.rf_records(w), ow, (name, "k_rfq", w))
        lean = Cap._results(job)
        Cap._check_decoders(job, sb, orc, lambda w: lean[w][6], (name, "lean"))
        fa_lean = job.fasta(ids)
        # ---- with another job pending: k_rows gathers the records itself (and leaves a window above the rows it stages to k_rfq, alone)
        other = api.job_from_synth(c, sb, W, targets=[0])
        other.featurize()
        job.featurize()
        job.infer(64, 1)
        fused, left = job.rf_fused(), job.rf_left()
        for w, ow in enumerate(ows):
            n_cells += records_against_the_oracles_cells(job.rf_records(w), ow, (name, "k_rows", w))
        lean2 = Cap._results(job)
        other.close(); other = None
        job.consensus()
        fa_lean2 = job.fasta(ids)
        # ---- planes path: features bit-exact on every window, k_consensus
        c.featurize_planes(True)
        job.featurize()
        assert G.compare_features(job, sb, store, W) == job.n_windows
        job.infer(64, 1)
        planes = Cap._logits(job)
        want = Cap._check_decoders(job, sb, orc, lambda w: planes[w][1], (name, "planes"))
        fa_planes = job.fasta(ids)
        plan_rows = [(job.info(w).length, job.info(w).n_supported) for w in range(job.n_windows)]
    finally:
        c.featurize_planes(False)
        if other is not None:
            other.close()
    big = sum(1 for ow in ows if len(ow.sup_pos) > lim["RW_SUPCAP"])
    assert fused and left == big == (1 if name == "largest_window_w8192" else 0), (fused, left, big)
    assert n_cells > 0
    assert fa_lean == fa_lean2 == fa_planes == "".join(want).encode()
    for w, (a, a2, ow) in enumerate(zip(lean, lean2, ows)):
        assert a[:5] == a2[:5], (name, w)
        assert np.array_equal(a[5], a2[5]) and np.array_equal(a[6], a2[6]), (name, w, "logits differ between the two gathers")
        assert (a[0], a[1]) == plan_rows[w] == (ow.bases.shape[0], len(ow.sup_pos)), (name, w, "rows differ from the planes path or the oracle")
        assert np.array_equal(a[5], planes[w][0]) and np.array_equal(a[6], planes[w][1]), (name, w, "logits differ from the planes path")
        assert a[2] == ow.n_alns and a[3] == ow.sup_pos.tolist() and a[4] == ow.sup_ins.tolist(), (name, w)
    # ---- logits against the fp32 twin on the oracle's features
    e_info, e_base = _twin_errors(orc, planes)
    print(f"{name}: rows {[a[0] for a in lean]} informative {[a[1] for a in lean]} alignments {[a[2] for a in lean]}; {n_cells} receptive-field cells; "
          f"twin error info {e_info:.2e} base {e_base:.2e}")
    assert max(e_info, e_base) <= TOL, (name, e_info, e_base)
    job.close()


@pytest.mark.parametrize("name", list(Wc.CASES))
def test_device_built_descriptors_equal_the_host_build(name):
    """The op lists and query spans of the width cases through k_cigar_scan, k_window_cuts and build_dev.hip (the event scratch it sizes from the ops included):
    every descriptor field and every slice's ops equal to the device-free host build."""
    sb, W, _, _ = _case(name)
    c = G.ctx()
    G.load_synth(c, sb)
    hc = api.HostContext((sb.off[1:] - sb.off[:-1]).astype(np.uint32))
    jd = api.job_from_synth(c, sb, W)
    jh = api.job_from_synth(hc, sb, W)
    try:
        assert c._l.herro_debug_job_dev_built(jd.h) == 1
        assert _same_jobs(hc, jd, jh) == len(Wc.census(sb, W)[0])
        assert jd.skipped() == jh.skipped() == (0, 0)
    finally:
        jd.close(); jh.close(); hc.close()


@pytest.mark.parametrize("name", ["directory_events_w8192", "largest_window_w8192", "kept_wide_slice_w2048"])
def test_directory_words_fit_in_front_and_are_flagged_behind(name, monkeypatch):
    """The directory words k_cols wrote for the carriers' columns, read back, against the host census (width_cases.directory_words): query index | events << 20
    where both fit, 0xffffffff from the first word with 4 095 events in front — word 128 of 256 in both 8192-base cases, nowhere in kept_wide_slice.  Without
    the debug switch: the mix is the input's."""
    monkeypatch.delenv("HERRO_DEBUG_CDIR_OVERFLOW", raising=False)
    lim = Wc.limits()
    cs = Wc.CASES[name]
    sb, W, _, _ = _case(name)
    nw = (W + 31) // 32
    arr = Wc.host_job(sb, W)
    c = G.ctx()
    G.load_synth(c, sb)
    job = api.job_from_synth(c, sb, W)
    try:
        job.featurize()
        seen = set()
        for o, d in enumerate(arr["ow"]):
            if int(d["win"]) != cs["win"]:
                continue
            dQ, de = Wc.directory_words(d, arr["ops"], lim, nw)
            want = np.where((dQ < lim["DIR_Q"]) & (de < lim["DIR_EV"]), dQ | (de << 20), 0xffffffff).astype(np.uint32)
            got = job.directory_words(o, nw)
            n = (int(d["wlen"]) + 31) // 32
            assert np.array_equal(got[:n], want[:n]), (name, o, np.flatnonzero(got[:n] != want[:n])[:8])
            flagged = np.flatnonzero(got[:n] == 0xffffffff)
            if 1 <= int(d["qid"]) <= cs["carriers"]:
                seen.add(int(d["strand"]))
                if name == "kept_wide_slice_w2048":
                    assert len(flagged) == 0
                else:
                    assert flagged.tolist() == list(range(128, 256)) and n == 256, (name, o, flagged[:4])
                    assert (got[:128] >> 20).tolist() == [min(32 * w, cs["ins"][1]) for w in range(128)]     # 32 events in front of every further word
            else:
                assert len(flagged) == 0 and (got[:n] >> 20).max() == 0
        assert seen == {0, 1}
    finally:
        job.close()


@pytest.mark.parametrize("precision", [1, api.DEFAULT_PRECISION])
def test_model_forward_on_a_window_of_more_than_65535_rows(precision):
    """The model's kernels on rows and plane strides that do not fit 16 bits (the width cases above reach them through receptive-field records; herro_model_forward
    makes k_conv_m read the token planes themselves, with the batch length as the stride): informative rows at both ends of a 66 100-row window, around row
    65 536, next to the collate padding of a short window — against the fp32 twin on the same batch, at the contract's 1e-3."""
    import model_ref as MR
    rng = np.random.default_rng(66100)
    L, win_len = 66100, [66100, 300]
    bases = np.full((2, L, 31), 11, np.uint8)
    quals = np.full((2, L, 31), 126, np.uint8)
    for k, n in enumerate(win_len):
        bases[k, :n] = rng.integers(0, 11, (n, 31))
        quals[k, :n] = rng.integers(33, 90, (n, 31))
    rows = [np.array([0, 1, 2, 300, 16383, 16384, 65533, 65534, 65535, 65536, 65537, 65538, 66000, 66097, 66098, 66099]), np.array([0, 150, 297, 298, 299])]
    lens = np.array([len(r) for r in rows], np.int32)
    c = G.ctx()
    c.set_precision(precision)
    info, base = c.model_forward(bases, quals, lens, np.concatenate(rows).astype(np.int32))
    cb, cq, cl, cidx, cpos = Wc.compact_twin_inputs([(bases[k, :n], quals[k, :n], rows[k]) for k, n in enumerate(win_len)], 2 * (model_io.Hyper().kw // 2))
    ti, tb = MR.run_batch(Cap._twin(), cb, cq, cl, cidx, gemm=True, positions_flat=cpos)
    assert info.shape == ti.shape and base.shape == tb.shape
    e_info, e_base = float(np.abs(info - ti).max()), float(np.abs(base - tb).max())
    print(f"precision {precision}: twin error info {e_info:.2e} base {e_base:.2e}")
    assert max(e_info, e_base) <= TOL, (precision, e_info, e_base)
