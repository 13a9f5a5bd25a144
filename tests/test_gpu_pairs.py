"""gpu: pair overlaps (herro_find_overlap_pairs, herro_pairs_align, herro_job_create_paired; DESIGN.md §10, "Pairs on the device") —
the strand choice, the compaction, the row table and the extension of the primaries on the device — against the stepwise chain on the
same context: find_overlaps -> pair_rows -> extend_overlaps(rows[prim]) -> align_dev -> mirror -> paired_job_args -> create_job_aligned.
Every result is compared exactly; the read sets are tests/pair_cases.py's."""
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
import aligned_dev_cases as AC  # noqa: E402
import gpu_common as G  # noqa: E402
import pair_cases as PC  # noqa: E402
from herro_amd import api  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(name, make, kw) for name, make, kws in PC.SETS for kw in kws]
_SETS = {}


def _set(name):
    if name not in _SETS:
        _SETS[name] = dict((n, m) for n, m, _ in PC.SETS)[name]()
    return _SETS[name]


def _ctx_with(name):
    c = G.ctx()
    PC.load(c, _set(name))
    return c


def _find(c, ext, **kw):
    return c.find_overlap_pairs(**kw) if ext is not None else c.find_overlap_pairs(extend=False, **kw)


# ---- 1. the handle against the stepwise chain ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,make,kw", CASES, ids=[f"{n}-{i}" for i, (n, _, _) in enumerate(CASES)])
def test_pairs_equal_the_stepwise_chain(name, make, kw):
    c = _ctx_with(name)
    n_pairs = None
    for ext in PC.EXTENDS:
        want = PC.stepwise(c, ext, **kw)
        p = _find(c, ext, **(dict(kw, **ext) if ext else kw))
        PC.assert_same_fields(PC.pairs_fields(p), want, (name, kw, ext))
        again = _find(c, ext, **(dict(kw, **ext) if ext else kw))
        assert PC.pairs_bytes(again) == PC.pairs_bytes(p)                      # a second call: the same bytes
        n_pairs = p.n_pairs
        if ext is None:
            assert not p.ext.any() and not p.ext_scores.any()
        elif name in "AB" and ext == {}:
            assert p.ext.any()                                               # the extension did move something
        p.close()
        again.close()
    pr = want["primaries"]
    if name == "A":
        assert n_pairs >= 20
    elif name == "B":
        assert n_pairs >= 40 and (pr[:, 4] == 0).any() and (pr[:, 4] == 1).any()
    elif name == "C":
        assert n_pairs == 1 and pr[0, 4] == 0                                 # an exact tie: the forward strand
    elif name == "D":
        assert pr[:, [5, 0, 4]].tolist() == [[0, 1, 0], [2, 3, 1], [4, 5, 0], [6, 7, 1]]
        if kw is PC.DEFAULTS:
            assert want["chain_scores"].tolist() == [1477, 1487, 1890, 1889]
        elif kw is PC.SMALL_K:
            assert want["chain_scores"].tolist()[:2] == [1499, 1497]
        assert want["rids"].tolist() == list(range(8)) and want["rec_of_row"].tolist() == [0, 4, 1, 5, 2, 6, 3, 7]
    else:
        assert n_pairs == 0 and want["aln_off"].tolist() == [0]
        for f in PC.FIELDS:
            assert np.asarray(want[f]).size == (1 if f == "aln_off" else 0)


# ---- 2. the scratch budget ----------------------------------------------------------------------------------------------------------------
_CHILD = r"""
import json, os, sys
sys.path.insert(0, os.path.join(sys.argv[1], "tests")); sys.path.insert(0, sys.argv[1])
from herro_amd import api
import pair_cases as PC
c = api.Context(0)
PC.load(c, PC.set_b())
out = []
for ext in PC.EXTENDS:
    p = c.find_overlap_pairs(**dict(PC.SMALL_K, **ext)) if ext is not None else c.find_overlap_pairs(extend=False, **PC.SMALL_K)
    out.append(PC.pairs_bytes(p).hex())
print(json.dumps(out))
"""


def test_a_small_scratch_budget_gives_the_same_bytes():
    """k = 15, w = 5: 35 654 anchors in chunks of ~8 000 — the primaries of a chunk land behind those of the chunks before it"""
    c = _ctx_with("B")
    env = dict(os.environ, HERRO_OVL_SCRATCH_MB="1", HERRO_OVL_STATS="1")
    p = subprocess.run([sys.executable, "-c", _CHILD, G.ROOT], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    chunks = [int(x) for x in re.findall(r"anchors=35654 .*chunks=(\d+)", p.stderr)]
    assert len(chunks) == 3 and min(chunks) >= 3, p.stderr[-500:]
    child = json.loads(p.stdout.strip().splitlines()[-1])
    for got, ext in zip(child, PC.EXTENDS):
        want = _find(c, ext, **(dict(PC.SMALL_K, **ext) if ext else PC.SMALL_K))
        assert want.n_pairs >= 40
        assert got == PC.pairs_bytes(want).hex(), ext
        want.close()


# ---- 3. OverlapPairs.align ----------------------------------------------------------------------------------------------------------------
def _same_handles(m, w, tag):
    assert m.n == w.n and m.failed == w.failed, tag
    assert np.array_equal(m.rows, w.rows) and np.array_equal(m.scores, w.scores) and np.array_equal(m.n_ops, w.n_ops), tag
    for r in range(m.n):
        assert m.cigar(r) == w.cigar(r), (tag, r)


@pytest.mark.parametrize("name,kw", [("A", dict(max_occ=64, min_score=200)), ("B", PC.DEFAULTS), ("D", PC.SMALL_K)])
def test_align_equals_align_dev_and_mirror(name, kw):
    c = _ctx_with(name)
    want = PC.stepwise(c, {}, **kw)
    h = c.align_dev(want["primaries"])
    w = h.mirror()
    h.close()
    p = c.find_overlap_pairs(**kw)
    m = p.align()
    assert m.n == 2 * p.n_pairs > 0 and (m.n_ops[:p.n_pairs] > 0).any()
    _same_handles(m, w, name)
    for x in (p, m, w):
        x.close()


# ---- 4. create_job_paired -----------------------------------------------------------------------------------------------------------------
def _same_jobs(c, jp, ja, tag, records=False):
    a, b = c.job_arrays(jp), c.job_arrays(ja)
    assert set(a) == set(b) and jp.n_windows == ja.n_windows > 0 and jp.skipped() == ja.skipped(), tag
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (tag, k)
    assert c._l.herro_debug_job_dev_built(jp.h) == c._l.herro_debug_job_dev_built(ja.h), tag
    ids = [f"read{t}" for t in range(jp.n_targets)]
    texts = []
    for j in (jp, ja):
        j.featurize(); j.infer(64, 1); j.consensus()
        texts.append(j.fasta(ids))
    assert texts[0] == texts[1] and (not records or texts[0].count(b">") > 0), tag


@pytest.mark.parametrize("name,kw,W", [("A", dict(max_occ=64, min_score=200), 256), ("A", dict(max_occ=64, min_score=200), 4096),
                                       ("D", PC.DEFAULTS, 256)])
def test_create_job_paired_equals_paired_job_args(name, kw, W):
    c = _ctx_with(name)
    p = c.find_overlap_pairs(**kw)
    m = p.align()
    assert m.failed == 0
    jp = c.create_job_paired(p, m, W)
    ja = c.create_job_aligned(*api.paired_job_args(p.rids, p.aln_off, p.rec_of_row, m.ok), m, W)
    assert jp.n_targets == ja.n_targets == len(p.rids)
    _same_jobs(c, jp, ja, (name, W), records=(name, W) == ("A", 256))   # (the other two: windows, but too few per read for a FASTA record)
    for x in (jp, ja, p, m):
        x.close()


# ---- 5. failed records --------------------------------------------------------------------------------------------------------------------
def test_create_job_paired_drops_failed_rows_and_keeps_the_targets():
    """set D: primaries 0 and 2 lose their ops, so their mirrors fail too — targets 0, 1, 4 and 5 have no row left and keep their place"""
    c = _ctx_with("D")
    p = c.find_overlap_pairs(**PC.DEFAULTS)
    assert p.n_pairs == 4
    h = c.align_dev(p.primaries)
    assert h.failed == 0
    off, ops = AC.cigars_to_ops([b"" if r in (0, 2) else h.cigar(r) for r in range(h.n)])
    h2 = c.aligned_dev_from_ops(h.rows, off, ops)
    m = h2.mirror()
    assert m.n == 8 and m.ok.tolist() == [False, True, False, True] * 2
    jp = c.create_job_paired(p, m, 256)
    rids, off2, rec = api.paired_job_args(p.rids, p.aln_off, p.rec_of_row, m.ok)
    assert rids.tolist() == list(range(8)) and np.diff(off2.astype(np.int64)).tolist() == [0, 0, 1, 1, 0, 0, 1, 1] and rec.tolist() == [1, 5, 3, 7]
    ja = c.create_job_aligned(rids, off2, rec, m, 256)
    assert jp.n_targets == 8
    _same_jobs(c, jp, ja, "failed")
    for x in (jp, ja, p, h, h2, m):
        x.close()


# ---- 6. errors ----------------------------------------------------------------------------------------------------------------------------
def _raises(code, text, fn, *args, **kw):
    with pytest.raises(api.HerroError) as e:
        fn(*args, **kw)
    assert e.value.code == code and text in str(e.value), str(e.value)


def test_errors():
    c = _ctx_with("D")
    h = C.c_void_p()
    k32 = api.OverlapParams(k=32)
    assert c._l.herro_find_overlap_pairs(c.h, C.byref(k32), None, 0, C.byref(h)) == -1 and "5 <= k <= 31" in c.last_error() and not h.value
    _raises(-1, "5 <= k <= 31", c.find_overlap_pairs, k=32)
    _raises(-1, "herro_find_overlap_pairs: max_ext must be at most 2^20", c.find_overlap_pairs, max_ext=(1 << 20) + 1)
    _raises(-1, "herro_find_overlap_pairs: max_ext must be at most 2^20", c.find_overlap_pairs, extend=False, max_ext=(1 << 20) + 1)
    other = api.Context(0)
    try:
        _raises(-6, "herro_set_reads must be called first", other.find_overlap_pairs)      # no reads
        _raises(-1, "max_ext must be at most 2^20", other.find_overlap_pairs, max_ext=(1 << 20) + 1)   # parameters first
        p = c.find_overlap_pairs(**PC.DEFAULTS)
        m = p.align()
        PC.load(other, _set("D"))
        p_other = other.find_overlap_pairs(**PC.DEFAULTS)
        m_other = p_other.align()
        assert other._l.herro_pairs_align(other.h, p.h, C.byref(h)) == -1 and "herro_pairs_align: the handle belongs to another context" in other.last_error()
        _raises(-1, "herro_job_create_paired: the handle belongs to another context", c.create_job_paired, p_other, m, 256)
        _raises(-1, "herro_job_create_paired: the handle belongs to another context", c.create_job_paired, p, m_other, 256)
        assert c._l.herro_job_create_status(c.h) == -1
        prim_only = c.align_dev(p.primaries)                                   # P records: the mirrors are missing
        _raises(-1, "herro_job_create_paired: the aligned handle has 4 records, the pairs need 8", c.create_job_paired, p, prim_only, 256)
        c.create_job_paired(p, m, 256).close()
        assert c._l.herro_job_create_status(c.h) == 0
        for x in (p, m, p_other, m_other, prim_only):
            x.close()
    finally:
        other.close()
