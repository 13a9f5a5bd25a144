"""gpu: a core set of targets on the device front end (herro_find_overlaps_core, herro_find_overlap_pairs_core; DESIGN.md §10, "A core
set of targets").  The yardstick is a filter of the unmasked result on the same context (tests/core_cases.py): every masked handle equals
filter_pairs(full handle) field for field, its alignments equal the full handle's at the kept indices, its job equals the job built from
the full handle restricted to the core targets, and the shards of shard.core_masks together correct every target once.  The `anchors`
figure of HERRO_OVL_STATS shows that the anchors were never created rather than dropped at the end.  Read sets: tests/pair_cases.py."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import core_cases as CC  # noqa: E402
import gpu_common as G  # noqa: E402
import pair_cases as PC  # noqa: E402
from herro_amd import api, shard  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(name, kw) for name, _, kws in PC.SETS for kw in kws]
_SETS = {}


def _set(name):
    if name not in _SETS:
        _SETS[name] = dict((n, m) for n, m, _ in PC.SETS)[name]()
    return _SETS[name]


def _ctx_with(name):
    c = G.ctx()
    PC.load(c, _set(name))
    return c, len(_set(name).off) - 1


def _find(c, ext, kw, core=None):
    return c.find_overlap_pairs(core=core, **dict(kw, **ext)) if ext is not None else c.find_overlap_pairs(extend=False, core=core, **kw)


# ---- 1. the masked handle is the filter of the full one -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw", CASES, ids=[f"{n}-{i}" for i, (n, _) in enumerate(CASES)])
def test_masked_pairs_equal_the_filtered_full_handle(name, kw):
    c, n = _ctx_with(name)
    M = CC.masks(n)
    some = 0
    for ext in PC.EXTENDS:
        full = _find(c, ext, kw)
        want_all, fields = PC.pairs_bytes(full), PC.pairs_fields(full)
        assert full.n_rows == 2 * full.n_pairs
        full.close()
        for mname, m in list(M.items()) + [("every3rd-2-255", CC.odd_bytes(M["every3rd"]))]:
            p = _find(c, ext, kw, core=m)
            want = CC.filter_pairs(fields, m)
            PC.assert_same_fields(PC.pairs_fields(p), want, (name, kw, ext, mname))
            assert p.n_pairs == len(want["primaries"]) and p.n_rows == len(want["rec_of_row"]) <= 2 * p.n_pairs
            if mname == "all":
                assert PC.pairs_bytes(p) == want_all                          # all ones: the bytes of herro_find_overlap_pairs
            if mname == "none" or name == "E":
                assert p.n_pairs == 0 and p.n_rows == 0 and p.aln_off.tolist() == [0]
            some += 0 < p.n_rows < 2 * full.n_pairs
            p.close()
        h = C.c_void_p()                                                      # a NULL mask through the new entry: the same bytes again
        pp, ee = c._overlap_params(dict(kw)), api.ExtendParams(**(ext or {}))
        c._chk(c._l.herro_find_overlap_pairs_core(c.h, C.byref(pp), C.byref(ee), 0 if ext is not None else api.PAIRS_NO_EXTEND, None, C.byref(h)))
        p = api.OverlapPairs(c, h)
        assert PC.pairs_bytes(p) == want_all
        p.close()
    assert some or name == "E", "no mask selected a proper part of the table"


# ---- 2. the stepwise finder -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw", [("B", PC.DEFAULTS), ("B", PC.SMALL_K), ("D", PC.DEFAULTS), ("D", PC.SMALL_K)])
def test_find_overlaps_with_a_mask_is_the_filtered_unmasked_call(name, kw):
    c, n = _ctx_with(name)
    full = c.find_overlaps(**kw)
    assert len(full[1]) > 0
    for mname, m in CC.masks(n).items():
        got = c.find_overlaps(core=m, **kw)
        want = CC.filter_rows(*full, m)
        for g, w, f in zip(got, want, ("rids", "rows", "aln_off", "scores")):
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (name, mname, f)
    got = c.find_overlaps(core=CC.odd_bytes(CC.masks(n)["first_half"]), **kw)
    for g, w in zip(got, CC.filter_rows(*full, CC.masks(n)["first_half"])):
        assert np.array_equal(g, w)


# ---- 3. the anchors that were never created, and the scratch budget ----------------------------------------------------------------------
_CHILD = r"""
import json, os, sys
sys.path.insert(0, os.path.join(sys.argv[1], "tests")); sys.path.insert(0, sys.argv[1])
from herro_amd import api
import core_cases as CC
import pair_cases as PC
c = api.Context(0)
rs = PC.set_b()
PC.load(c, rs)
M = CC.masks(len(rs.off) - 1)
out = []
for ext in PC.EXTENDS:
    p = c.find_overlap_pairs(core=M["every3rd"], **dict(PC.SMALL_K, **ext)) if ext is not None else c.find_overlap_pairs(extend=False, core=M["every3rd"], **PC.SMALL_K)
    out.append(PC.pairs_bytes(p).hex())
sys.stderr.write("SECOND\n")
c.find_overlap_pairs(core=M["first_half"], **PC.DEFAULTS).close()
c.find_overlaps(core=M["first_half"], **PC.DEFAULTS)
print(json.dumps(out))
"""


def test_the_anchor_count_is_the_masked_one_under_a_small_scratch_budget():
    """set B, k = 15, w = 5, every third read core: 20 615 of the 35 654 anchors exist, in several chunks at 1 MiB, and the bytes are those of
    the in-process call with the default budget; at the defaults with the first half core: 4 216 of 6 838"""
    assert CC.EXPECTED[("B", "SMALL_K")][1]["every3rd"][0] == 20615 and CC.EXPECTED[("B", "DEFAULTS")][1]["first_half"][0] == 4216
    c, n = _ctx_with("B")
    env = dict(os.environ, HERRO_OVL_SCRATCH_MB="1", HERRO_OVL_STATS="1")
    p = subprocess.run([sys.executable, "-c", _CHILD, G.ROOT], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    first, second = p.stderr.split("SECOND\n")
    lines = re.findall(r"OVL .*", first)
    chunks = [int(x) for x in re.findall(r"anchors=20615 .*chunks=(\d+)", first)]
    assert len(lines) == 3 and len(chunks) == 3 and min(chunks) >= 2, first[-500:]
    assert re.findall(r"anchors=(\d+)", second) == ["4216", "4216"], second[-500:]
    child = json.loads(p.stdout.strip().splitlines()[-1])
    m = CC.masks(n)["every3rd"]
    for got, ext in zip(child, PC.EXTENDS):
        want = _find(c, ext, PC.SMALL_K, core=m)
        assert want.n_pairs == 44 and want.n_rows == 50
        assert got == PC.pairs_bytes(want).hex(), ext
        want.close()


# ---- 4. align and the job -------------------------------------------------------------------------------------------------------------------
def _restricted_job_args(full, m_full, mask):
    """create_job_aligned's arguments for the full handle's rows whose target is core: the same targets in the same order"""
    rids, off, rec = api.paired_job_args(full.rids, full.aln_off, full.rec_of_row, m_full.ok)
    keep_t = np.asarray(mask)[rids] != 0
    off = off.astype(np.int64)
    parts = [rec[off[t]:off[t + 1]] for t in np.flatnonzero(keep_t)]
    new_off = np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.uint64)
    return rids[keep_t], new_off, np.concatenate(parts).astype(np.uint32) if parts else np.zeros(0, np.uint32)


def _run(job, batch=64):
    job.featurize(); job.infer(batch, 0); job.consensus()


def _same_jobs(c, jp, ja, tag):
    a, b = c.job_arrays(jp), c.job_arrays(ja)
    assert set(a) == set(b) and jp.n_targets == ja.n_targets and jp.n_windows == ja.n_windows > 0 and jp.skipped() == ja.skipped(), tag
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (tag, k)
    _run(jp); _run(ja)
    rows = 0
    for w in range(jp.n_windows):
        wa, wb = jp.window(w), ja.window(w)
        assert (wa.info.length, wa.info.n_supported) == (wb.info.length, wb.info.n_supported), (tag, w)
        assert np.array_equal(wa.sup_pos, wb.sup_pos) and np.array_equal(wa.sup_ins, wb.sup_ins), (tag, w)       # informative rows
        (ia, ba), (ib, bb) = jp.logits(w), ja.logits(w)
        assert ia.tobytes() == ib.tobytes() and ba.tobytes() == bb.tobytes(), (tag, w)                           # bit for bit
        rows += wa.info.n_supported
    assert rows > 0, tag
    ids = [f"read{t}" for t in range(jp.n_targets)]
    assert jp.fasta(ids) == ja.fasta(ids), tag


@pytest.mark.parametrize("name,kw,W", [("A", dict(max_occ=64, min_score=200), 256), ("B", PC.DEFAULTS, 256)])
def test_align_and_job_of_a_masked_handle_equal_the_full_handle_restricted(name, kw, W):
    c, n = _ctx_with(name)
    full = c.find_overlap_pairs(**kw)
    m_full = full.align()
    P = full.n_pairs
    for mname in ("every3rd", "first_half"):
        mask = CC.masks(n)[mname]
        p = c.find_overlap_pairs(core=mask, **kw)
        m = p.align()
        kept = np.flatnonzero((mask[full.primaries[:, 5]] | mask[full.primaries[:, 0]]) != 0)
        assert 0 < p.n_pairs == len(kept) < P and p.n_rows <= 2 * p.n_pairs and m.n == 2 * p.n_pairs
        sel = np.concatenate([kept, P + kept])                                 # primaries, then mirrors
        assert np.array_equal(m.rows, m_full.rows[sel]) and np.array_equal(m.scores, m_full.scores[sel]) and np.array_equal(m.n_ops, m_full.n_ops[sel])
        for r, rf in enumerate(sel):
            assert m.cigar(r) == m_full.cigar(int(rf)), (name, mname, r)
        jp = c.create_job_paired(p, m, W)
        rids, off, rec = _restricted_job_args(full, m_full, mask)
        assert np.array_equal(rids, p.rids)
        ja = c.create_job_aligned(rids, off, rec, m_full, W)
        _same_jobs(c, jp, ja, (name, mname))
        for x in (jp, ja, p, m):
            x.close()
    full.close()
    m_full.close()


# ---- 5. the shards together -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw,W", [("A", dict(max_occ=64, min_score=200), 256), ("B", PC.DEFAULTS, 256)])
def test_the_shards_of_core_masks_correct_every_target_once(name, kw, W):
    c, n = _ctx_with(name)
    lens = np.diff(np.asarray(_set(name).off).astype(np.int64))
    full = c.find_overlap_pairs(**kw)
    m_full = full.align()
    masks = shard.core_masks(lens, W, 3)
    parts = []
    for mask in masks:
        rec = shard.correct_reads_shard(c, mask, W, 64, 0, lambda r: f"read{r}", **kw)         # (one job: the yardstick's batches)
        rids, off, recs = _restricted_job_args(full, m_full, mask)
        assert len(rids) > 0 and np.array_equal(rec[0], rids) and (np.diff(rids.astype(np.int64)) > 0).all()
        ja = c.create_job_aligned(rids, off, recs, m_full, W)
        _run(ja)
        text, ends = ja.fasta([f"read{int(r)}" for r in rids], with_ends=True)
        ja.close()
        assert bytes(rec[2]) == text and np.array_equal(rec[1], ends), name
        parts.append(rec)
    rids, ends, text = shard.merge_records(parts)
    assert np.array_equal(np.sort(rids), full.rids) and len(np.unique(rids)) == len(rids)   # every target of the full table, once
    assert int(ends[-1]) == len(text) and bytes(text).count(b">") > 0
    by_id = shard.sorted_fasta(rids, ends, text)
    assert re.findall(rb">read(\d+)", by_id) == sorted(re.findall(rb">read(\d+)", by_id), key=int)
    full.close()
    m_full.close()


# ---- 6. errors ------------------------------------------------------------------------------------------------------------------------------
def _raises(code, text, fn, *args, **kw):
    with pytest.raises(api.HerroError) as e:
        fn(*args, **kw)
    assert e.value.code == code and text in str(e.value), str(e.value)


def test_errors():
    c, n = _ctx_with("D")
    mask = CC.masks(n)["first_half"]
    other = api.Context(0)
    try:
        _raises(-1, "max_ext must be at most 2^20", other.find_overlap_pairs, max_ext=(1 << 20) + 1, core=mask)   # parameters first
        _raises(-6, "herro_set_reads must be called first", other.find_overlap_pairs, core=mask)                  # then: no reads
        _raises(-6, "herro_set_reads must be called first", other.find_overlaps, core=mask)
        p = c.find_overlap_pairs(core=mask, **PC.DEFAULTS)
        m = p.align()
        assert (p.n_pairs, p.n_rows, m.n) == (3, 5, 6)
        PC.load(other, _set("D"))
        h = C.c_void_p()
        assert other._l.herro_pairs_align(other.h, p.h, C.byref(h)) == -1 and "herro_pairs_align: the handle belongs to another context" in other.last_error()
        p_other = other.find_overlap_pairs(core=mask, **PC.DEFAULTS)
        _raises(-1, "herro_job_create_paired: the handle belongs to another context", c.create_job_paired, p_other, m, 256)
        rows_only = c.align_dev(p.primaries)                                   # P' records: the mirrors are missing
        _raises(-1, "herro_job_create_paired: the aligned handle has 3 records, the pairs need 6", c.create_job_paired, p, rows_only, 256)
        assert c._l.herro_job_create_status(c.h) == -1
        c.create_job_paired(p, m, 256).close()
        assert c._l.herro_job_create_status(c.h) == 0
        with pytest.raises(ValueError):
            c.find_overlap_pairs(core=mask[:-1], **PC.DEFAULTS)
        for x in (p, m, p_other, rows_only):
            x.close()
    finally:
        other.close()


# ---- 7. correct_reads_sharded on a one-rank RCCL group ---------------------------------------------------------------------------------------
def test_correct_reads_sharded_on_rccl_with_one_rank():
    """LOOPBACK: the gather of the records goes through the transport; the records are those of correct_reads_shard with every read core"""
    import textwrap
    code = textwrap.dedent("""
        import json, os, sys
        import numpy as np
        sys.path.insert(0, 'tests')
        import torch, torch.distributed as dist
        torch.cuda.set_device(0)
        dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda', 0))
        import gpu_common as G
        import pair_cases as PC
        from herro_amd import shard
        assert shard.LOOPBACK and dist.get_backend() == 'nccl'
        W, kw = 256, dict(max_occ=64, min_score=200)
        rs = PC.set_a(W)
        c = G.ctx()
        PC.load(c, rs)
        lens = np.diff(np.asarray(rs.off).astype(np.int64))
        name = lambda r: f"read{r}"
        got, n_mine = shard.correct_reads_sharded(c, lens, W, 64, 0, name, group_targets=5, **kw)
        want = shard.correct_reads_shard(c, np.ones(len(lens), np.uint8), W, 64, 0, name, group_targets=5, **kw)
        out = {"n_mine": n_mine, "reads": len(lens), "records": bytes(want[2]).count(b">"),
               "same": all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(got, want))}
        dist.barrier()
        dist.destroy_process_group()
        print("RESULT " + json.dumps(out))
    """)
    env = dict(os.environ, HERRO_SHARD_LOOPBACK="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29519", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-c", code], cwd=G.ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert r.returncode == 0 and lines, r.stdout[-3000:]
    d = json.loads(lines[-1][7:])
    assert d["same"] and d["n_mine"] == d["reads"] == 12 and d["records"] >= 1, d
