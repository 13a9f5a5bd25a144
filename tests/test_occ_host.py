"""not-gpu: the frequency cut taken from the index (occ_frac_ppm; tests/occ_ref.py) without a device — the pick against the sorted-array
definition, what the cut does on the deep and the 33-deep read sets of tests/occ_cases.py under the numpy reference, two mutants of the
specification, and the parameter on a device-free context."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occ_cases as OC  # noqa: E402
import occ_ref as OR  # noqa: E402
import overlap_ref as R  # noqa: E402
from herro_amd import api  # noqa: E402


def _q_by_sorting(counts, ppm):
    """the (D - drop)-th smallest clamped count"""
    c = sorted(min(int(x), 65535) for x in counts)
    D = len(c)
    return c[D - D * ppm // 10**6 - 1] if D else 0


def _by_sorting(counts, ppm, max_occ=0):
    """the definition: q, the floor, the ceiling, the clamp"""
    cut = max(_q_by_sorting(counts, ppm), 10)
    if max_occ:
        cut = min(cut, max_occ)
    return min(cut, 65534)


# ---- the pick ---------------------------------------------------------------------------------------------------------------------------------
def test_the_pick_equals_the_sorted_array_definition_on_random_multisets():
    rng = np.random.default_rng(3)
    seen = dict(ties=0, floor=0, ceiling=0, clamp=0, drop0=0)
    for trial in range(300):
        D = int(rng.integers(1, 400))
        hi = int(rng.choice([3, 12, 40, 300, 70000, 200000]))
        c = rng.integers(1, hi + 1, D)
        if trial % 3 == 0:
            c[rng.integers(0, D, D // 2 + 1)] = int(rng.integers(1, hi + 1))              # many runs of one length: ties at q
        ppm = int(rng.choice([1, 500, 5000, 20000, 300000, 999999]))
        max_occ = int(rng.choice([0, 0, 5, 50, 100000]))
        got, want = OR.occ_cut(c, ppm, max_occ), _by_sorting(c, ppm, max_occ)
        assert got == want, (trial, D, ppm, max_occ)
        q = _q_by_sorting(c, ppm)
        drop = D * ppm // 10**6
        seen["ties"] += int((np.minimum(c, 65535) == q).sum() > 1 and q > 10)
        seen["floor"] += int(want == 10 and max(c) > 10 and not (max_occ and max_occ <= 10))
        seen["ceiling"] += int(max_occ and want == max_occ)
        seen["clamp"] += int(want == 65534)
        seen["drop0"] += int(drop == 0)
        f = OR.figures(c, ppm, max_occ)
        assert f["cut_runs"] == sum(1 for x in c if x > want) and f["cut_minimizers"] == sum(int(x) for x in c if x > want) and f["distinct"] == D
        assert (np.minimum(c, 65535) > q).sum() <= drop                                     # no more than the fraction lies above q
    assert min(seen.values()) >= 5, seen


def test_the_edges_of_the_pick():
    assert OR.occ_cut([37], 5000) == 37                                   # D = 1: nothing may be dropped
    assert OR.occ_cut([3], 5000) == 10 and OR.occ_cut([], 5000) == 10     # the floor
    assert OR.occ_cut([20] * 999 + [50], 999) == 50                       # drop = floor(0.999) = 0
    assert OR.occ_cut([20] * 1000 + [50], 1000) == 20                     # drop = 1
    assert OR.occ_cut([20] * 1000 + [50, 50], 1000) == 50                 # two runs tie above a drop of one: both are kept
    assert OR.occ_cut([200] * 10, 5000, max_occ=64) == 64                 # the ceiling
    assert OR.occ_cut([200] * 10, 5000, max_occ=0) == 200                 # 0: no ceiling, not 128
    assert OR.occ_cut([70000, 140000], 5000) == 65534                     # the last bin is never usable
    assert OR.occ_cut([65534, 140000], 600000) == 65534 and OR.occ_cut([65535] * 3, 1) == 65534
    h = OR.histogram([1, 1, 2, 65534, 65535, 65536, 10**6])
    assert h.dtype == np.uint32 and len(h) == 65536 and (h[1], h[2], h[65534], h[65535]) == (2, 1, 1, 3) and h.sum() == 7
    for bad in (0, 10**6, -1):
        with pytest.raises(ValueError):
            OR.occ_cut([5, 5], bad)


# ---- the deep set: a fixed cut below the depth finds nothing ---------------------------------------------------------------------------------
# (k, w): runs above 128, (cut, distinct, runs above it, their minimizers), anchors at the fixed cut and at the index's
DEEP = {(15, 5): (127, dict(cut=190, distinct=1826, cut_runs=8, cut_minimizers=1545), 458, 2008237),
        (25, 17): (41, dict(cut=180, distinct=915, cut_runs=3, cut_minimizers=556), 332, 560466)}


@pytest.mark.parametrize("kw", OC.DEEP_KW, ids=["k15w5", "k25w17"])
def test_the_deep_set_needs_the_cut_from_the_index(kw):
    rs, codes = OC.get("deep")
    assert len(codes) == 200 and set(len(c) for c in codes) == {400}
    over128, fig, anchors_fixed, anchors_frac = DEEP[(kw["k"], kw["w"])]
    st = {}
    fixed = R.find_overlaps(codes, stats=st, **kw)
    h, _, _, _ = R.sketch_store(codes, kw["k"], kw["w"])
    print(dict(kw=kw, over128=int((OR.run_counts(h) > 128).sum()), anchors_fixed=st["anchors"], pairs_fixed=len(fixed[1]) // 2))
    assert int((OR.run_counts(h) > 128).sum()) == over128
    assert len(fixed[1]) == 0 and st["anchors"] == anchors_fixed                        # max_occ = 128: 0 of 19 900 pairs
    (rids, rows, aln_off, scores), cut, st = OC.reference("deep", OC.PPM, **kw)
    print(dict(cut=cut, occ=st["occ"], anchors=st["anchors"], pairs=len(rows) // 2))
    assert cut > 128 and st["occ"] == fig and st["anchors"] == anchors_frac
    assert len(rows) == 2 * OC.DEEP_PAIRS and len(st["pairs"]) == OC.DEEP_PAIRS == 19900  # every pair
    assert len(rids) == 200 and (np.diff(aln_off.astype(np.int64)) == 199).all()


# ---- the 33-deep set: the index's cut is far below 128 ---------------------------------------------------------------------------------------
D33 = {(25, 17): (dict(cut=25, distinct=4836, cut_runs=12, cut_minimizers=314), 71665),
       (15, 5): (dict(cut=29, distinct=9563, cut_runs=29, cut_minimizers=881), 339383)}


@pytest.mark.parametrize("kw", [dict(k=25, w=17, min_score=100), dict(k=15, w=5, min_score=60)], ids=["k25w17", "k15w5"])
def test_the_33_deep_set_is_cut_below_128_and_keeps_every_pair(kw):
    rs, codes = OC.get("depth33")
    fig, anchors = D33[(kw["k"], kw["w"])]
    (rids, rows, aln_off, scores), cut, st = OC.reference("depth33", OC.PPM, **kw)
    h, _, _, _ = R.sketch_store(codes, kw["k"], kw["w"])
    c = OR.run_counts(h)
    print(dict(kw=kw, occ=st["occ"], anchors=st["anchors"], pairs=len(rows) // 2, longest=int(c.max())))
    assert st["occ"] == fig and cut < 128 and st["anchors"] == anchors
    assert int(((c > cut) & (c <= 128)).sum()) == fig["cut_runs"] >= 1                  # runs the fixed cut would have used
    assert len(rows) == 2 * 528 and len(st["pairs"]) == 33 * 32 // 2
    hist, fig2 = OR.census(codes, OC.PPM, **kw)
    assert fig2 == fig and hist.sum() == fig["distinct"] and int((hist * np.arange(65536)).sum()) == len(h)


def test_a_ceiling_below_the_indexs_cut_is_the_cut():
    kw = dict(k=15, w=5, min_score=60)
    (_, rows, _, _), cut, st = OC.reference("depth33", OC.PPM, max_occ=20, **kw)
    assert cut == 20 and st["anchors"] == 24450 and len(rows) == 2 * 521
    assert OC.reference("depth33", OC.PPM, max_occ=128, **kw)[1] == 29                  # a ceiling above it changes nothing


# ---- two mutants of the specification ---------------------------------------------------------------------------------------------------------
def _differs(a, b):
    return any(x.shape != y.shape or not np.array_equal(x, y) for x, y in zip(a, b))


def test_the_pick_one_rank_higher_changes_the_output():
    """33-deep, (25, 17), 500 ppm: 2 of 4836 runs may be dropped and exactly two runs of 27 lie above the 26 of the third — one rank higher
    they are kept"""
    kw = dict(k=25, w=17, min_score=100)
    rs, codes = OC.get("depth33")
    h, _, _, _ = R.sketch_store(codes, 25, 17)
    c = OR.run_counts(h)
    assert (OR.occ_cut(c, 500), OR.occ_cut(c, 500, _rank=1)) == (26, 27)
    good, cut, st = OC.reference("depth33", 500, **kw)
    st2 = {}
    bad = R.find_overlaps(codes, stats=st2, **dict(kw, max_occ=27))
    assert cut == 26 and st["anchors"] != st2["anchors"] and _differs(good, bad)


def test_the_pick_without_the_floor_changes_the_output():
    """four reads of one genome, half of the distinct hashes to be dropped: q = 1, and only the floor keeps the runs of 2 .. 4"""
    kw = dict(k=15, w=5, min_score=60)
    rs, codes = OC.get("four")
    h, _, _, _ = R.sketch_store(codes, 15, 5)
    c = OR.run_counts(h)
    assert (OR.occ_cut(c, 500000), OR.occ_cut(c, 500000, _floor=0)) == (10, 1) and c.max() == 4
    (_, rows, _, _), cut, st = OC.reference("four", 500000, **kw)
    assert cut == 10 and len(rows) == 12 and st["anchors"] == 1901
    st2 = {}
    bad = R.find_overlaps(codes, stats=st2, **dict(kw, max_occ=1))
    assert len(bad[1]) == 0 and st2["anchors"] == 0


# ---- the parameter on a device-free context ---------------------------------------------------------------------------------------------------
def test_the_struct_and_the_parameter_check_on_a_host_context():
    assert C.sizeof(api.OverlapParams) == 32 and api.OverlapParams.occ_frac_ppm.offset == 28
    c = api.HostContext(np.array([100, 200], np.uint32))
    h = C.c_void_p()
    out = (C.c_uint64 * 4)()
    for ppm in (10**6, 10**6 + 1, 0xFFFFFFFF):
        p = api.OverlapParams(occ_frac_ppm=ppm)
        assert c._l.herro_find_overlaps(c.h, C.byref(p), C.byref(h)) == -1 and "occ_frac_ppm" in c.last_error()
        assert c._l.herro_find_overlaps_core(c.h, C.byref(p), None, C.byref(h)) == -1
        assert c._l.herro_find_overlap_pairs(c.h, C.byref(p), None, 0, C.byref(h)) == -1
        assert c._l.herro_find_overlap_pairs_core(c.h, C.byref(p), None, 0, None, C.byref(h)) == -1 and "occ_frac_ppm" in c.last_error()
        assert c._l.herro_debug_occ_census(c.h, C.byref(p), None, out) == -1 and not h.value
    with pytest.raises(api.HerroError) as e:
        c.find_overlaps(occ_frac_ppm=10**6)
    assert e.value.code == -1 and "occ_frac_ppm" in str(e.value)
    for ppm in (1, 5000, 999999):                                             # legal: the call gets as far as asking for a device
        p = api.OverlapParams(occ_frac_ppm=ppm)
        assert c._l.herro_find_overlaps(c.h, C.byref(p), C.byref(h)) == -2 and "the context has no device" in c.last_error()
        assert c._l.herro_debug_occ_census(c.h, C.byref(p), None, out) == -2
    k32 = api.OverlapParams(k=32, occ_frac_ppm=5000)
    assert c._l.herro_find_overlaps(c.h, C.byref(k32), C.byref(h)) == -1 and "5 <= k <= 31" in c.last_error()
    assert c._l.herro_debug_occ_census(c.h, None, None, out) == -1 and "occ_frac_ppm is 0" in c.last_error()
    with pytest.raises(TypeError):
        c.find_overlaps(occ_frac=5000)
    assert c._l.herro_overlaps_occ_cut(None) == 0 and c._l.herro_pairs_occ_cut(None) == 0
    assert "herro_overlaps_occ_cut" in api.EXPORTS and "herro_pairs_occ_cut" in api.EXPORTS and "herro_debug_occ_census" in api.EXPORTS
