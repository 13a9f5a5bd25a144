"""gpu: the longer chain look-back (herro_set_chain_params, k_chain_far in csrc/overlap_dev.hip; DESIGN.md §10, "A longer look-back") against
tests/overlap_ref.py at the same look-back, bit for bit: the chain stage alone through herro_debug_chain — at 64 that is today's k_chain —
on slices around every block and round boundary and on whole tandem groups, then the finder, the pairs, a regular batch, a 1 MiB scratch
budget in a child process and the life of the setting."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gpu_common as G  # noqa: E402
import lookback_cases as L  # noqa: E402
import overlap_ref as R  # noqa: E402
from herro_amd import api, synth  # noqa: E402

pytestmark = pytest.mark.gpu

FKW = dict(k=15, w=5, max_occ=4096, min_score=100)     # the finder's parameters on the tandem sets
_CACHE = {}


def _ctx():
    c = G.ctx()
    c.set_chain_lookback(0)                             # every test starts from the default, whatever the previous one left
    return c


def _same(got, want):
    g_rids, g_rows, g_off, g_sc = got
    r_rids, r_rows, r_off, r_sc = want
    assert g_rids.tolist() == r_rids.tolist()
    assert g_off.tolist() == r_off.tolist()
    bad = [i for i in range(min(len(g_rows), len(r_rows))) if not np.array_equal(g_rows[i], r_rows[i]) or int(g_sc[i]) != int(r_sc[i])]
    assert not bad and len(g_rows) == len(r_rows), (len(g_rows), len(r_rows), [(i, g_rows[i].tolist(), int(g_sc[i]), r_rows[i].tolist(), int(r_sc[i])) for i in bad[:5]])
    assert g_rows.dtype == np.uint32 and g_rows.shape[1] == 10 and (g_rows[:, 9] == 0).all()


def _load(c, names):
    seq, qual, off, codes = L.store(names)
    c.set_reads(seq, qual, off)
    return codes


def _ref_find(names, H):
    """R.find_overlaps of a store of tandem sets at a look-back, once per process"""
    key = (tuple(names), H)
    if key not in _CACHE:
        _CACHE[key] = R.find_overlaps(L.store(names)[3], lookback=H, **FKW)
    return _CACHE[key]


# ---- 1, 2: the chain stage alone ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_gap", L.GAPS)
@pytest.mark.parametrize("H", (64, 128, 192, 256, 512, 1024))
def test_the_chain_stage_on_the_slices(H, max_gap):
    """every slice in one call — groups of 1 to 3000 anchors share a launch; at 64 the default context drives k_chain itself"""
    c = _ctx()
    kw = dict(k=L.KW["k"], bandwidth=L.KW["bandwidth"], max_gap=max_gap)
    got = c.chain(list(L.slices()), **kw) if H == 64 else c.chain(list(L.slices()), lookback=H, **kw)
    want = L.ref_slices(H, max_gap)
    bad = [(n, g.tolist(), w) for n, g, w in zip(L.SLICE_LENGTHS, got, want) if tuple(g.tolist()) != w]
    assert not bad, bad[:5]
    assert c.chain_lookback == 64


WHOLE = [(name, H) for name, (_, _, scores) in L.SETS.items() for H in scores if H <= 1024 and (name != "T4" or H in L.T4_USED)]


@pytest.mark.parametrize("name,H", WHOLE, ids=[f"{n}-{h}" for n, h in WHOLE])
def test_the_chain_stage_on_the_whole_groups(name, H):
    c = _ctx()
    got = c.chain([L.group(name)], lookback=H, k=L.KW["k"], bandwidth=L.KW["bandwidth"], max_gap=L.KW["max_gap"])
    assert tuple(got[0].tolist()) == L.ref_group(name, H)
    assert int(got[0, 0]) == L.SETS[name][2][H]


# ---- 3: the finder ---------------------------------------------------------------------------------------------------------------------------
def _span(rows):
    return [(int(r[8]) - int(r[7])) / int(r[6]) for r in rows]


@pytest.mark.parametrize("names", (("T1",), ("T0", "T2")), ids=("T1", "T0+T2"))
@pytest.mark.parametrize("H", (128, 192, 256, 1024))
def test_the_finder_equals_the_reference_at_the_lookback(names, H):
    c = _ctx()
    _load(c, names)
    got = c.find_overlaps(lookback=H, **FKW)
    want = _ref_find(names, H)
    assert len(want[1]) == 2 * len(names)
    _same(got, want)
    again = c.find_overlaps(lookback=H, **FKW)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    if names == ("T1",) and H == 256:
        assert min(_span(got[1])) >= 0.99
        at64 = c.find_overlaps(**FKW)
        _same(at64, _ref_find(names, 64))
        assert int(at64[0][0]) == 0 and round(_span(at64[1])[0], 2) == 0.57 and max(_span(at64[1])) < 0.61      # 3 437 of target 0's 6 000 bases


# ---- 4: a regular batch ------------------------------------------------------------------------------------------------------------------------
def test_a_regular_batch_without_repeats_at_256():
    sb = synth.merge([
        synth.generate(4, 4096, 12, seed=51, p_partial=0.3, min_partial_len=1024),
        synth.generate(1, 30000, 8, seed=56, flank_min=200, flank_max=400),                     # >= 30 kb: several hundred anchors per wave
    ])
    codes = [R.store_codes(sb.read_seq(i)) for i in range(sb.n_reads)]
    c = _ctx()
    G.load_synth(c, sb)
    want = R.find_overlaps(codes, lookback=256, max_occ=64, min_score=100)
    assert len(want[1]) >= 2 * 300 and (want[1][:, 8] - want[1][:, 7]).max() >= 25000
    _same(c.find_overlaps(lookback=256, max_occ=64, min_score=100), want)


# ---- 5: pairs -----------------------------------------------------------------------------------------------------------------------------------
def test_pairs_at_256_on_the_tandem_pair():
    c = _ctx()
    _load(c, ("T1",))
    rids, rows, off, sc = _ref_find(("T1",), 256)
    prim = rows[rows[:, 5] < rows[:, 0]]                     # tid < qid: the pair's record, query 1 on target 0
    assert len(prim) == 1
    for core in (None, np.array([1, 0], np.uint8)):
        pairs = c.find_overlap_pairs(extend=False, lookback=256, core=core, **FKW)
        try:
            assert pairs.n_pairs == 1 and pairs.n_rows == (2 if core is None else 1)
            assert pairs.primaries[0, :9].tolist() == prim[0, :9].tolist()
            assert int(pairs.chain_scores[0]) == int(sc[0]) == L.SETS["T1"][2][256]
            if core is None:
                m = pairs.align()
                try:
                    assert m.n == 2 and int(m.failed) == 0 and m.ok.all()
                finally:
                    m.close()
        finally:
            pairs.close()
    assert c.chain_lookback == 64


# ---- 6: the scratch budget ------------------------------------------------------------------------------------------------------------------------
_CHILD = r"""
import json, os, sys
sys.path.insert(0, os.path.join(sys.argv[1], "tests")); sys.path.insert(0, sys.argv[1])
from herro_amd import api
import lookback_cases as L
import test_gpu_lookback as T
seq, qual, off, _ = L.store(("T0", "T2"))
c = api.Context(0)
c.set_reads(seq, qual, off)
rids, rows, aoff, sc = c.find_overlaps(lookback=256, **T.FKW)
print(json.dumps({"rids": rids.tolist(), "rows": rows.tolist(), "off": aoff.tolist(), "sc": sc.tolist()}))
"""


def test_a_scratch_budget_of_1_mib_gives_the_same_bytes_at_256():
    c = _ctx()
    _load(c, ("T0", "T2"))
    rids, rows, off, sc = c.find_overlaps(lookback=256, **FKW)
    _same((rids, rows, off, sc), _ref_find(("T0", "T2"), 256))
    env = dict(os.environ, HERRO_OVL_SCRATCH_MB="1", HERRO_OVL_STATS="1")      # ~8 000 anchors a chunk: T2's 50 000 run alone, over the budget
    p = subprocess.run([sys.executable, "-c", _CHILD, G.ROOT], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    child = json.loads(p.stdout.strip().splitlines()[-1])
    assert child["rids"] == rids.tolist() and child["off"] == off.tolist() and child["sc"] == sc.tolist()
    assert child["rows"] == rows.tolist()
    ovl = [ln for ln in p.stderr.splitlines() if ln.startswith("OVL ")]
    assert ovl and int(ovl[-1].split("chunks=")[1]) >= 2, p.stderr[-500:]
    assert any(ln.startswith("OVLCHAIN lookback=256 ") for ln in p.stderr.splitlines()), p.stderr[-500:]


# ---- 7: the life of the setting ---------------------------------------------------------------------------------------------------------------
def test_the_setting_holds_until_it_is_changed_and_a_keyword_for_one_call():
    c = _ctx()
    _load(c, ("T1",))
    w64, w256 = _ref_find(("T1",), 64), _ref_find(("T1",), 256)
    assert w64[3].tolist() != w256[3].tolist()
    c.set_chain_lookback(256)
    try:
        _same(c.find_overlaps(**FKW), w256)                  # the context's setting
        _same(c.find_overlaps(lookback=64, **FKW), w64)      # a keyword for one call ...
        assert c.chain_lookback == 256
        _same(c.find_overlaps(**FKW), w256)                  # ... leaves the setting as it was
        _same(c.find_overlaps(lookback=None, **FKW), w256)
        for bad in (63, 65, 1088, 1 << 31):                  # a refused value changes nothing
            with pytest.raises(api.HerroError) as e:
                c.set_chain_lookback(bad)
            assert e.value.code == -1
            with pytest.raises(api.HerroError):
                c.find_overlaps(lookback=bad, **FKW)
        assert c.chain_lookback == 256
        _same(c.find_overlaps(**FKW), w256)
        got = c.chain([L.group("T0")], k=L.KW["k"])          # the hook runs under the setting too
        assert tuple(got[0].tolist()) == L.ref_group("T0", 256)
        c.set_chain_lookback(0)
        assert c.chain_lookback == 64
        _same(c.find_overlaps(**FKW), w64)                   # the 64 one again
        _same(c.find_overlaps(lookback=256, **FKW), w256)
        _same(c.find_overlaps(**FKW), w64)
    finally:
        c.set_chain_lookback(0)
