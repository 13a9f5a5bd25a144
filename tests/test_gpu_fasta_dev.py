"""-m gpu: the corrected reads as FASTA formed on the device (csrc/fasta_dev.hip, herro_job_fasta_dev) against the host path and the
specification.  herro_job_fasta — the parent's code, unchanged — is the oracle: with all-zero parameters the device text, its target ends and
its statistics are the host path's, byte for byte; with parameters the text is tests/chop_ref.py applied to the host path's text.  The jobs
are those of tests/chop_cases.py (tests/test_chop_host.py proves what they cover) and one family with informative rows that runs the model."""
import ctypes as C

import numpy as np
import pytest

import chop_cases as CC
import chop_ref as R
import gpu_common as G
from herro_amd import api, synth

pytestmark = pytest.mark.gpu


def _codes():
    """the two codes by name, read from the header the library was built from"""
    import os
    import re
    hdr = open(os.path.join(G.ROOT, "include", "herro_amd.h")).read()
    return {k: int(v) for k, v in re.findall(r"#define\s+(HERRO_E_[A-Z_]+)\s+\(?(-?\d+)\)?", hdr)}


def host_fasta(job, ids, descs=None):
    """herro_job_fasta with descriptions and missing ids (Job.fasta passes neither): (text, rec_end)"""
    n = len(ids)
    a = (C.c_char_p * max(n, 1))(*ids)
    d = None if descs is None else (C.c_char_p * max(n, 1))(*descs)
    ends = np.zeros(max(n, 1), np.uint64)
    need = job._l.herro_job_fasta(job.h, a, d, None, 0, ends.ctypes.data)
    assert need >= 0, need
    out = np.empty(max(int(need), 1), np.uint8)
    got = job._l.herro_job_fasta(job.h, a, d, out.ctypes.data, int(need), None)
    assert got == need
    return out[:got].tobytes(), [int(e) for e in ends[:n]]


def _hand_job(c, case):
    c.set_reads(case.seq, case.qual, case.off)
    job = c.create_job(case.rids, case.rows, case.aln_off, case.cigars, case.W)
    job.featurize()
    if any(job.info(w).n_supported for w in range(job.n_windows)):
        job.infer(64, 1)
    job.consensus()
    return job


def _check_against_host(job, ids, descs, params, host=None):
    """every (chop_len, min_length, line_width) of params: text, target ends and statistics are chop_ref's of the host path's text"""
    text, ends = host if host is not None else host_fasta(job, ids, descs)
    for C_, M, L in params:
        want, wst, wends = R.chop(text, C_, M, L, ends)
        got, gends, gst = job.fasta_dev(ids, descs, chop_len=C_, min_length=M, line_width=L, with_ends=True, with_stats=True)
        assert got == want, ((C_, M, L), len(got), len(want), next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), None))
        assert gends.tolist() == wends, (C_, M, L)
        assert tuple(gst) == tuple(wst), ((C_, M, L), gst, wst)
    return text, ends


@pytest.mark.parametrize("W", [16, 40])
def test_hand_cases_equal_the_host_path_and_the_specification(W):
    case = CC.hand_case(W)
    c = G.ctx()
    job = _hand_job(c, case)
    try:
        text, ends = host_fasta(job, case.ids, case.descs)
        assert (text, ends) == CC.host_text(case)                 # what tests/test_chop_host.py proved the coverage from
        # all-zero parameters, and no parameters at all: the host path's bytes
        got, gends, gst = job.fasta_dev(case.ids, case.descs, with_ends=True, with_stats=True)
        assert got == text and gends.tolist() == ends
        n_rec = text.count(b">")
        assert tuple(gst) == (n_rec, sum(len(s) for _, _, s in R.parse(text)), 0, 0, n_rec, sum(b > a for a, b in zip([0] + ends[:-1], ends)))
        h = C.c_void_p()
        ids = (C.c_char_p * len(case.ids))(*case.ids)
        descs = (C.c_char_p * len(case.ids))(*case.descs)
        c._chk(job._l.herro_job_fasta_dev(job.h, ids, descs, None, C.byref(h)))
        try:
            assert C.string_at(job._l.herro_fasta_text_data(h), job._l.herro_fasta_text_len(h)) == text
        finally:
            job._l.herro_fasta_text_free(h)
        # without descriptions: Job.fasta's own text
        plain_ids = [i if i is not None else b"x" for i in case.ids]
        host_plain, plain_ends = job.fasta(plain_ids, with_ends=True)
        dev_plain, dev_ends = job.fasta_dev(plain_ids, with_ends=True)
        assert dev_plain == host_plain and dev_ends.tolist() == plain_ends.tolist()
        arr = job.fasta_dev(plain_ids, as_array=True)
        assert arr.dtype == np.uint8 and arr.tobytes() == host_plain
        # the parameter lists
        _check_against_host(job, case.ids, case.descs, CC.param_sets(text, W), host=(text, ends))
        # two consecutive calls, and the host path after the device call
        assert job.fasta_dev(case.ids, case.descs, chop_len=W + 1, min_length=2, line_width=7) == job.fasta_dev(case.ids, case.descs, chop_len=W + 1, min_length=2, line_width=7)
        assert host_fasta(job, case.ids, case.descs) == (text, ends)
    finally:
        job.close()


def test_chunk_sizes_give_the_same_bytes():
    case = CC.hand_case(16)
    c = G.ctx()
    job = _hand_job(c, case)
    try:
        text, ends = host_fasta(job, case.ids, case.descs)
        params = [(0, 0, 0), (17, 2, 7), (1, 0, 0), (15, 15, 60), (30000, 0, 1)]
        for chunk in (64, 4096, 0):
            c.fasta_chunk(chunk)
            _check_against_host(job, case.ids, case.descs, params, host=(text, ends))
        c.fasta_chunk(50)            # not a multiple of 16: rounded up inside, the same bytes
        _check_against_host(job, case.ids, case.descs, params[:2], host=(text, ends))
    finally:
        c.fasta_chunk(0)
        job.close()


def test_more_than_one_scan_tile_of_windows_and_pieces():
    case = CC.big_case()
    c = G.ctx()
    job = _hand_job(c, case)
    try:
        assert job.n_windows > CC.SCAN_TILE
        text, ends = host_fasta(job, case.ids, case.descs)
        assert (text, ends) == CC.host_text(case)
        _check_against_host(job, case.ids, case.descs, CC.BIG_PARAMS, host=(text, ends))
        c.fasta_chunk(4096)
        _check_against_host(job, case.ids, case.descs, CC.BIG_PARAMS[:3], host=(text, ends))
    finally:
        c.fasta_chunk(0)
        job.close()


def test_informative_rows_through_the_model():
    """Windows with informative rows: the consensus holds the model's calls, insertions and removed bases, so the windows' lengths are
    irregular.  Both sides read the same consensus; the model's values do not matter."""
    W = 256
    sb = synth.generate(4, 1500, 16, seed=synth.SEED + 151, flank_min=30, flank_max=60, p_snp=0.03, p_partial=0.4)
    c = G.ctx()
    G.load_synth(c, sb)
    ids = [b"read%d" % t for t in range(sb.n_targets)]
    descs = [b"t=%d" % t if t % 2 else None for t in range(sb.n_targets)]
    job = api.job_from_synth(c, sb, W)
    try:
        job.featurize(); job.infer(64, 1); job.consensus()
        assert sum(job.info(w).n_supported for w in range(job.n_windows)) > 0
        text, ends = host_fasta(job, ids, descs)
        assert len({len(s) % W for _, _, s in R.parse(text)}) > 1
        got, gends = job.fasta_dev(ids, descs, with_ends=True)
        assert got == text and gends.tolist() == ends
        _check_against_host(job, ids, descs, CC.param_sets(text, W), host=(text, ends))
        c.fasta_chunk(64)
        _check_against_host(job, ids, descs, [(0, 0, 0), (W + 1, 3, 60)], host=(text, ends))
        assert host_fasta(job, ids, descs) == (text, ends)
    finally:
        c.fasta_chunk(0)
        job.close()


def test_checks_and_their_order():
    codes = _codes()
    case = CC.hand_case(16)
    c = G.ctx()
    c.set_reads(case.seq, case.qual, case.off)
    job = c.create_job(case.rids, case.rows, case.aln_off, case.cigars, case.W)
    L = job._l
    ids = (C.c_char_p * len(case.ids))(*case.ids)
    h = C.c_void_p(1)
    try:
        job.featurize()
        assert L.herro_job_fasta_dev(None, ids, None, None, C.byref(h)) == codes["HERRO_E_INVALID"]
        assert L.herro_job_fasta_dev(job.h, ids, None, None, None) == codes["HERRO_E_INVALID"]
        assert L.herro_job_fasta_dev(job.h, None, None, None, C.byref(h)) == codes["HERRO_E_INVALID"] and not h
        bad = api.ChopParams(chop_len=1 << 31)
        assert L.herro_job_fasta_dev(job.h, ids, None, C.byref(bad), C.byref(h)) == codes["HERRO_E_INVALID"]     # before the state: the consensus has not run either
        assert "chop_len = 2147483648" in L.herro_last_error(c.h).decode()
        bad = api.ChopParams(flags=2)
        assert L.herro_job_fasta_dev(job.h, ids, None, C.byref(bad), C.byref(h)) == codes["HERRO_E_INVALID"]
        with pytest.raises(api.HerroError) as e:
            job.fasta_dev(case.ids)
        assert e.value.code == codes["HERRO_E_STATE"] and "herro_job_consensus has not run" in str(e.value)
        job.consensus()
        assert job.fasta_dev(case.ids, case.descs) == host_fasta(job, case.ids, case.descs)[0]
    finally:
        job.close()


def _close(a, b):
    if len(a) != len(b):
        return abs(len(a) - len(b)) <= 2
    return sum(x != y for x, y in zip(a, b)) <= max(1, len(a) // 1000)


def test_the_sibling_tile_repeat_runs_in_front_of_the_text():
    """The software hook of tests/test_gpu_sib_retry.py (a flag in host memory; no GPU fault): the device call finds the word, the job's model
    and consensus passes are repeated once without sibling tiles, and the text is formed from the repeated pass — the bytes the host path then
    gives for the same job."""
    sb = synth.generate(2, 2 * 4096, 32, seed=synth.SEED + 71, p_snp=0.03)
    c = G.ctx()
    G.load_synth(c, sb)
    c.set_precision(4)
    ids = [f"read{t}" for t in range(sb.n_targets)]
    job = api.job_from_synth(c, sb, 4096)
    try:
        job.featurize(); job.infer(64, 1); job.consensus()
        assert max(job.info(w).n_supported for w in range(job.n_windows)) > 64, "the case needs a window on sibling tiles"
        fa0 = job.fasta_dev(ids)
        assert fa0 == job.fasta(ids)
        r0 = c.sib_retries()
        job.featurize(); job.infer(64, 1); job.consensus()
        c.sib_fault()
        fa1 = job.fasta_dev(ids, chop_len=1000, line_width=60)
        assert c.sib_retries() == r0 + 1
        host1 = job.fasta(ids)                                   # the repeated pass, fetched by the host path: no second repeat
        assert c.sib_retries() == r0 + 1
        assert fa1 == R.chop(host1, 1000, 0, 60)[0]
        assert job.fasta_dev(ids) == host1
        a, b = fa0.splitlines(), host1.splitlines()              # the two model paths agree within their tolerance, as in test_gpu_sib_retry.py
        assert len(a) == len(b) and all(x == y for x, y in zip(a[::2], b[::2])) and all(_close(x, y) for x, y in zip(a[1::2], b[1::2]))
    finally:
        job.close()
        c.set_precision(api.DEFAULT_PRECISION)


def _records(rec):
    rids, ends, text = rec
    text, ends = bytes(text), np.concatenate([[0], np.asarray(ends).astype(np.int64)])
    return {int(r): text[ends[i]:ends[i + 1]] for i, r in enumerate(rids)}


def test_the_shard_pipeline_writes_assembler_ready_records():
    """shard.correct_reads_shard(postprocess=...): reads alone -> overlaps -> alignments -> consensus -> chopped FASTA; every target's records
    are the default path's put through the specification."""
    import pair_cases as PC
    from herro_amd import shard
    rs = PC.set_a()
    c = G.ctx()
    PC.load(c, rs)
    W, kw = 256, dict(max_occ=64, min_score=200)
    read_name = lambda r: f"read{r}"
    everything = np.ones(len(rs.off) - 1, np.uint8)
    plain = _records(shard.correct_reads_shard(c, everything, W, 64, 0, read_name, **kw))
    longest = max(len(s) for t in plain.values() for _, _, s in R.parse(t))
    assert len(plain) > 0 and longest > 8
    assert _records(shard.correct_reads_shard(c, everything, W, 64, 0, read_name, postprocess={}, **kw)) == plain
    post = dict(chop_len=longest // 2, min_length=longest // 4, line_width=60)
    got = _records(shard.correct_reads_shard(c, everything, W, 64, 0, read_name, group_targets=7, postprocess=post, **kw))
    assert got == {r: R.chop(t, **post)[0] for r, t in plain.items()}
    assert any(b"_sliding:%d-" % (longest // 2 + 1) in t for t in got.values())
