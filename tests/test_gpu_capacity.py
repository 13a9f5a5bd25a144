"""-m gpu: the pileup and consensus kernels past their LDS capacities (capacity_cases.py), against the oracle.

Every case crosses k_rows' insertion-row cap (several passes, informative flags read back from global memory) or k_quals' event cap;
A and B also leave k_consensus_p's votes in global memory, B and C make it write the corrected bases as byte stores, A and B have
windows above the fused f16 stack's informative rows.  On each case: features bit-exact on the planes path; the lean path equal to
the planes path (informative rows, logits bit for bit, FASTA; on its own and with a job pending); the consensus of k_consensus,
k_consensus_p and the host decoder equal to the oracle decoding the job's own logits; logits within 1e-3 of the fp32 twin.  Then a
seeded sweep at ONT-like error rates, and the argmax rule (last maximum wins, NaN is greatest) on planted ties, infinities and NaNs
through all three decoders."""
import numpy as np
import pytest

import capacity_cases as K
import gpu_common as G
import oracle_lib as O
from herro_amd import api, synth

pytestmark = pytest.mark.gpu
TOL = 1e-3
TOKMAP = np.full(256, 255, np.uint8)
for _i, _ch in enumerate("ACGT*acgt#."):
    TOKMAP[ord(_ch)] = _i


def _oracle(sb, W):
    """per target: (rid, FeatResult, [OracleWindow])"""
    store = O.store_from_synth(sb)
    out = []
    for t in range(sb.n_targets):
        rid, rows, cigs = O.target_alignments(sb, t)
        res = store.extract_features(rid, rows, cigs, W)
        out.append((rid, res, [res.window(wi) for wi in range(len(res))]))
    return store, out


def _logits(job):
    return [job.logits(w) for w in range(job.n_windows)]


def _oracle_fasta(orc, base_of_window):
    """per target: the oracle's consensus.rs + lib.rs decoding base_of_window(job window) -> [n_supported, 5]"""
    out, w = [], 0
    for rid, res, wins in orc:
        lg = [base_of_window(w + i) for i in range(len(wins)) if len(wins[i].sup_pos)]
        out.append(res.consensus_fasta(np.concatenate(lg) if lg else np.zeros((0, 5), np.float32)))
        w += len(wins)
    return out


def _check_decoders(job, sb, orc, base_of_window, tag):
    """The host decoder (before herro_job_consensus), then the device decoder of the job's path (k_consensus or k_consensus_p): FASTA of every
    target, one by one and all together, == the oracle decoding the same base logits."""
    want = _oracle_fasta(orc, base_of_window)
    names = [sb.read_name(rid) for rid, _, _ in orc]
    for t, nm in enumerate(names):
        assert job.consensus_fasta(t, nm) == want[t], (tag, "host decoder", t)
    job.consensus()
    for t, nm in enumerate(names):
        assert job.consensus_fasta(t, nm) == want[t], (tag, "device decoder", t)
    assert job.fasta(names).decode() == "".join(want), (tag, "herro_job_fasta")
    assert sum(bool(x) for x in want) > 0, tag
    return want


def _results(job):
    """the per-window results of a job behind herro_job_infer that the two paths must agree on (asks for no token plane)"""
    wins = []
    for w in range(job.n_windows):
        wi = job.info(w)
        sp = np.zeros(wi.n_supported, np.uint16)
        si = np.zeros(wi.n_supported, np.uint8)
        job.ctx._chk(job._l.herro_job_window_copy(job.h, w, 1, None, None, sp.ctypes.data, si.ctypes.data, None))
        info, base = job.logits(w)
        wins.append((wi.length, wi.n_supported, wi.n_alns, sp.tolist(), si.tolist(), info, base))
    return wins


def _run_lean(job):
    """featurize + infer + the per-window results"""
    job.featurize()
    job.infer(64, 1)
    return _results(job)


_TWIN = {}


def _twin():
    """the fp32 twin on the GPU (windows of 17 k rows x 31 columns through its dense convolutions)"""
    if "m" not in _TWIN:
        import torch
        import model_ref as MR
        from herro_amd import model_io
        _TWIN["m"] = MR.build(G.raw_params(), model_io.Hyper()).to(torch.device("cuda", 0))
    return _TWIN["m"]


def _twin_errors(orc, logits):
    """base / info logits of the job against the fp32 twin on the ORACLE's features (all informative windows in one batch, as
    herro_job_infer(64, 1) groups a job of <= 64 windows: the collate padding of the shorter windows reaches their last rows)"""
    import model_ref as MR
    wins, w = [], 0
    for _, _, ows in orc:
        for ow in ows:
            if len(ow.sup_pos):
                wins.append((w, ow))
            w += 1
    assert 0 < len(wins) <= 64
    lmax = max(ow.bases.shape[0] for _, ow in wins)
    bases = np.full((len(wins), lmax, 31), 11, np.uint8)   # collate padding, inference.rs:86-97
    quals = np.full((len(wins), lmax, 31), 126, np.uint8)
    lens, flat = [], []
    for k, (_, ow) in enumerate(wins):
        enc = TOKMAP[ow.bases]
        bases[k, :enc.shape[0]] = enc
        quals[k, :enc.shape[0]] = ow.quals
        tidx = np.flatnonzero(enc[:, 0] != 4)
        lens.append(len(ow.sup_pos))
        flat.extend((tidx[ow.sup_pos.astype(np.int64)] + ow.sup_ins).tolist())
    ti, tb = MR.run_batch(_twin(), bases, quals, np.array(lens, np.int32), np.array(flat, np.int32), gemm=True)
    e_info = e_base = 0.0
    o = 0
    for k, (w, _) in enumerate(wins):
        gi, gb = logits[w]
        e_info = max(e_info, float(np.abs(gi - ti[o:o + lens[k]]).max()))
        e_base = max(e_base, float(np.abs(gb - tb[o:o + lens[k]]).max()))
        o += lens[k]
    return e_info, e_base


@pytest.mark.parametrize("name", list(K.CASES))
def test_capacity_case_against_the_oracle(name):
    cs = K.CASES[name]
    W = cs["W"]
    cap = K.caps()
    sb = K.generate(name)
    c = G.ctx()
    G.load_synth(c, sb)
    store, orc = _oracle(sb, W)
    ids = [sb.read_name(rid) for rid, _, _ in orc]
    job = api.job_from_synth(c, sb, W)
    other = None
    try:
        # ---- planes path: features bit-exact (k_tokens, k_quals<true> past its event cap), k_consensus
        c.featurize_planes(True)
        job.featurize()
        assert G.compare_features(job, sb, store, W) == job.n_windows
        job.infer(64, 1)
        planes = _logits(job)
        want = _check_decoders(job, sb, orc, lambda w: planes[w][1], (name, "planes"))
        fa_planes = job.fasta(ids)
        plan_rows = [(job.info(w).length, job.info(w).n_supported) for w in range(job.n_windows)]
        # ---- lean path (k_rows, k_consensus_p): on its own (k_rfq) and with another job pending (fused gather)
        c.featurize_planes(False)
        lean = _run_lean(job)
        assert not job.rf_fused()
        _check_decoders(job, sb, orc, lambda w: lean[w][6], (name, "lean"))
        fa_lean = job.fasta(ids)
        other = api.job_from_synth(c, sb, W, targets=[0])
        other.featurize()
        lean2 = _run_lean(job)
        fused = job.rf_fused()
        other.close(); other = None
        job.consensus()
        fa_lean2 = job.fasta(ids)
    finally:
        c.featurize_planes(False)
        if other is not None:
            other.close()
    assert fused
    assert fa_lean == fa_lean2 == fa_planes == "".join(want).encode()
    for w, (a, a2) in enumerate(zip(lean, lean2)):
        assert a[:5] == a2[:5], (name, w)
        assert np.array_equal(a[5], a2[5]) and np.array_equal(a[6], a2[6]), (name, w, "logits differ between the two gathers")
        assert (a[0], a[1]) == plan_rows[w], (name, w, "informative rows differ from the planes path")
        assert np.array_equal(a[5], planes[w][0]) and np.array_equal(a[6], planes[w][1]), (name, w, "logits differ from the planes path")
    ows = [ow for _, _, wins in orc for ow in wins]
    for w, (a, ow) in enumerate(zip(lean, ows)):
        assert a[3] == ow.sup_pos.tolist() and a[4] == ow.sup_ins.tolist(), (name, w)
    # ---- logits against the fp32 twin on the oracle's features
    e_info, e_base = _twin_errors(orc, planes)
    assert max(e_info, e_base) <= TOL, (name, e_info, e_base)
    # ---- what the case crossed, on the device's own counts
    irows = max(a[0] - int((ow.bases[:, 0] != ord("*")).sum()) for a, ow in zip(lean, ows))   # L' on the device - window length
    out_len = max(len(K.corrected_window(ow, a[6])) for a, ow in zip(lean, ows))
    seen = {"RW_ICAP": int(irows), "CP_ICAP": int(irows), "CP_OCAP": out_len, "QEVCAP": int(K.insertion_events(sb, W).max()),
            "FUSED_ROWS": max(a[1] for a in lean)}
    crossed = {k: (seen[k], cap[k]) for k in seen if seen[k] > cap[k]}
    print(f"{name}: crossed {crossed}; largest {seen}; twin error info {e_info:.2e} base {e_base:.2e}")
    for k in cs["crosses"]:
        assert seen[k] > cap[k], (name, k, seen[k], cap[k])
    if "CP_ICAP" in cs["crosses"] and "CP_OCAP" in cs["crosses"]:   # votes in global memory AND byte stores, in one window
        assert any(a[0] - int((ow.bases[:, 0] != ord("*")).sum()) > cap["CP_ICAP"] and len(K.corrected_window(ow, a[6])) > cap["CP_OCAP"]
                   for a, ow in zip(lean, ows)), name
    job.close()


@pytest.mark.parametrize("trial", G.sweep_trials(8))
def test_high_error_sweep_against_the_oracle(trial):
    """Seeded sweep at ONT-like insertion / deletion rates: features (planes path) bit-exact, and the device consensus of both paths
    equal to the oracle decoding the job's own logits."""
    g = np.random.default_rng(0x3c6ef372 + trial)
    W = int(g.choice([1000, 2048, 4096, 8192]))
    tl = int(g.integers(1, 3)) * W + int(g.integers(0, W))
    ov = int(g.integers(20, 41))
    kw = dict(p_sub=float(g.choice([0.006, 0.02, 0.03])), p_ins=float(g.choice([0.02, 0.05, 0.08])), p_del=float(g.choice([0.02, 0.05, 0.08])),
              p_partial=float(g.choice([0.0, 0.3])))
    sb = synth.generate(int(g.integers(1, 4)), tl, ov, seed=int(g.integers(1, 1 << 30)), **kw)
    c = G.ctx()
    G.load_synth(c, sb)
    store, orc = _oracle(sb, W)
    job = api.job_from_synth(c, sb, W)
    try:
        c.featurize_planes(True)
        job.featurize()
        assert G.compare_features(job, sb, store, W) == job.n_windows
        job.infer(64, 1)
        planes = _logits(job)
        fa = _check_decoders(job, sb, orc, lambda w: planes[w][1], (trial, W, ov, kw, "planes"))
        c.featurize_planes(False)
        job.featurize()
        job.infer(64, 1)
        lean = _logits(job)
        assert _check_decoders(job, sb, orc, lambda w: lean[w][1], (trial, W, ov, kw, "lean")) == fa
    finally:
        c.featurize_planes(False)
    ows = [ow for _, _, ws in orc for ow in ws]
    irows = max(job.info(w).length - int((ow.bases[:, 0] != ord("*")).sum()) for w, ow in enumerate(ows))
    cap = K.caps()
    seen = {"RW_ICAP": int(irows), "CP_ICAP": int(irows), "FUSED_ROWS": max(len(x[0]) for x in lean)}
    print(f"trial {trial}: W {W} depth {ov} {kw}: crossed {[k for k in seen if seen[k] > cap[k]]}; largest {seen}")
    job.close()


_NAN, _INF = np.float32("nan"), np.float32("inf")
_PLANTED = [   # (row, the decoder's answer: the LAST maximum, NaN the greatest, -0.0 == +0.0)
    ([1, 1, 1, 1, 1], 4), ([2, 2, 0, 0, 0], 1), ([0, 3, 0, 3, -1], 3), ([3, 0, 3, 0, 1], 2), ([5, 5, 5, 0, 0], 2), ([0, 5, 5, 5, 1], 3),
    ([1, 1, 1, 1, 0], 3), ([0, 2, 0, 0, 2], 4), ([2, 0, 0, 2, 2], 4), ([-0.0, 0.0, -1, -1, -1], 1), ([0.0, -0.0, -1, -1, -1], 1),
    ([-1, -1, -1, 0.0, -0.0], 4), ([-1, -0.0, -1, 0.0, -2], 3), ([_INF, 0, _INF, 0, 0], 2), ([_INF] * 5, 4), ([0, _INF, 0, 0, _INF], 4),
    ([-_INF, -_INF, 3, -_INF, -_INF], 2), ([-_INF, -_INF, -_INF, -_INF, 0], 4), ([0, -_INF, -_INF, -_INF, -_INF], 0), ([-_INF] * 5, 4),
    ([_NAN, 0, 9, 0, 0], 0), ([0, _NAN, 9, 0, 0], 1), ([9, 0, _NAN, 0, 0], 2), ([0, 9, 0, _NAN, 0], 3), ([0, 9, 0, 0, _NAN], 4),
    ([_NAN, 0, _NAN, 0, 0], 2), ([_NAN, _NAN, 0, 0, 0], 1), ([_NAN] * 5, 4), ([0, _NAN, _NAN, _NAN, 0], 3), ([-_NAN, 0, 0, 0, 0], 0),
    ([0, _NAN, _INF, 0, 0], 1), ([0, _INF, _NAN, 0, 0], 2), ([_NAN, _INF, _INF, _INF, _INF], 0), ([_INF, _INF, _NAN, -_INF, 0], 2),
]


@pytest.mark.parametrize("W", [4096, 8192])
def test_argmax_rule_on_planted_logits(W):
    """consensus.rs:136-141, max_by_key(OrderedFloat): planted rows (ties of two to five classes, -0.0 against +0.0, infinities, NaN at
    every index, several NaNs, NaN next to +inf) among random logits; the host decoder, k_consensus (planes path) and k_consensus_p
    (lean path) against the oracle decoding the same array."""
    sb = synth.generate(2, 2 * W + 333, 30, seed=synth.SEED + 131 + W, p_sub=0.01, p_ins=0.01, p_del=0.01)
    c = G.ctx()
    G.load_synth(c, sb)
    _, orc = _oracle(sb, W)
    job = api.job_from_synth(c, sb, W)
    ows = [ow for _, _, wins in orc for ow in wins]
    corrected = np.concatenate([np.full(len(ow.sup_pos), min(ow.n_alns, 30) >= 2) for ow in ows])
    rows = np.flatnonzero(corrected)
    assert len(rows) >= 4 * len(_PLANTED), len(rows)
    g = np.random.default_rng(W)
    base = g.standard_normal((len(corrected), 5)).astype(np.float32)
    at = np.sort(g.choice(rows, 3 * len(_PLANTED), replace=False))   # every pattern three times, at rows spread over the job
    for k, r in enumerate(at):
        base[r] = np.array(_PLANTED[k % len(_PLANTED)][0], np.float32)
    off = np.concatenate([[0], np.cumsum([len(ow.sup_pos) for ow in ows])])
    try:
        for planes in (True, False):
            c.featurize_planes(planes)
            job.featurize()
            job.infer(64, 1)
            assert [job.info(w).n_supported for w in range(job.n_windows)] == [len(ow.sup_pos) for ow in ows]
            job.set_base_logits(base)
            got = np.concatenate([job.logits(w)[1] for w in range(job.n_windows)])
            assert np.array_equal(got.view(np.uint32), base.view(np.uint32))   # the host copy is the planted array, bit for bit
            _check_decoders(job, sb, orc, lambda w: base[off[w]:off[w + 1]], (W, "planes" if planes else "lean"))
    finally:
        c.featurize_planes(False)
    cap = K.caps()
    irows = max(job.info(w).length - int((ow.bases[:, 0] != ord("*")).sum()) for w, ow in enumerate(ows))
    print(f"argmax W {W}: {len(at)} planted rows of {len(base)}; crossed {[k for k in ('RW_ICAP', 'CP_ICAP') if irows > cap[k]]}; largest insertion rows {irows}")
    for row, arg in _PLANTED:   # the rule itself, as the oracle states it, on the bare rows
        v = np.array(row, np.float32)
        a = 0
        for k in range(1, 5):
            if np.isnan(v[k]) or (not np.isnan(v[a]) and v[k] >= v[a]):
                a = k
        assert a == arg, (row, a, arg)
    job.close()
