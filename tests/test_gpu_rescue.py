"""gpu: the rescue of high-frequency minimizers (herro_set_seed_rescue; k_occ_place, k_rescue, k_resc_kind and the RESCUE side of k_runs / k_expand in
csrc/overlap_dev.hip; DESIGN.md §10, "Rescue of high-frequency minimizers").  The yardstick is tests/rescue_ref.py over tests/overlap_ref.py:
the flags minimizer for minimizer, find_overlaps and find_overlap_pairs record for record, a core mask as a selection of the unmasked result,
one scratch budget against another byte for byte, the setting off against a context that never had it, and reads to windows on a set that
has no overlap without it.  Read sets: tests/rescue_cases.py."""
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
import rescue_cases as RC  # noqa: E402
import rescue_ref as RR  # noqa: E402
from herro_amd import api  # noqa: E402

pytestmark = pytest.mark.gpu

_OWN = {}


def _ctx_with(name):
    """a context of this module's own (the setting must not reach the other modules' shared one), one per read set"""
    if name not in _OWN:
        c = api.Context(0)
        PC.load(c, RC.get(name)[0])
        _OWN[name] = c
    c = _OWN[name]
    c.set_seed_rescue(None)
    return c, RC.get(name)[1]


def teardown_module(module):
    for c in _OWN.values():
        c.close()
    _OWN.clear()


def _ref_flags(name, kw, d, rmax, ppm=0):
    h, rid, pos, st, lens = RC.sketch(name, kw["k"], kw["w"])
    cut = kw["max_occ"]
    if ppm:
        import occ_ref as OR
        cut = OR.occ_cut(OR.run_counts(h), ppm, 0)
    return RR.rescue_flags(h, rid, pos, lens, cut, d, rmax), cut


# ---- 1. the flags -----------------------------------------------------------------------------------------------------------------------------
FLAGS = [("streaks", RC.KW, case, ppm) for case in RC.CASES for ppm in (0, RC.PPM)] + [("set_a", RC.A_KW, RC.A_RESCUE, 0), ("set_b", RC.B_KW, RC.B_RESCUE, 0)]


@pytest.mark.parametrize("name,kw,case,ppm", FLAGS, ids=[f"{n}-{c if isinstance(c, str) else 'own'}-{'frac' if p else 'fixed'}" for n, _, c, p in FLAGS])
def test_the_flags_equal_the_reference(name, kw, case, ppm):
    d, rmax = RC.CASES[case] if isinstance(case, str) else case
    c, codes = _ctx_with(name)
    (want_occ, want), cut = _ref_flags(name, kw, d, rmax, ppm)
    fkw = dict({k: v for k, v in kw.items() if k in ("k", "w")}, **(dict(occ_frac_ppm=ppm) if ppm else dict(max_occ=kw["max_occ"])))
    occ, got = c.seed_rescue(occ_dist=d, rescue_max_occ=rmax, **fkw)
    print(dict(name=name, case=case, cut=cut, minimizers=len(occ), rescued=int(got.sum()), want=int(want.sum())))
    assert occ.dtype == np.uint32 and got.dtype == np.uint8 and len(occ) == len(want_occ)
    assert np.array_equal(occ, np.minimum(want_occ, RR.OCC_CAP)) and np.array_equal(got, want)
    occ2, got2 = c.seed_rescue(occ_dist=d, rescue_max_occ=rmax, **fkw)
    assert occ2.tobytes() == occ.tobytes() and got2.tobytes() == got.tobytes()
    o3, f3 = c.seed_rescue(**fkw)                                          # the keywords restored the setting: off, no flag, the same occ
    assert not f3.any() and o3.tobytes() == occ.tobytes()


# ---- 2. find_overlaps and find_overlap_pairs --------------------------------------------------------------------------------------------------
FIND = [("streaks", RC.KW, RC.CASES[case], ppm) for case, ppm in (("d100", 0), ("d200", 0), ("d1", 0), ("d_big", 0), ("r_below", 0), ("r_equal", 0),
                                                                   ("r_above", 0), ("d100", RC.PPM), ("d1", RC.PPM))]
FIND += [("set_a", RC.A_KW, RC.A_RESCUE, 0), ("set_b", RC.B_KW, RC.B_RESCUE, 0)]


def _finder_kw(kw, ppm):
    return dict({k: v for k, v in kw.items() if k != "max_occ"}, occ_frac_ppm=ppm) if ppm else dict(kw)


@pytest.mark.parametrize("name,kw,resc,ppm", FIND, ids=[f"{c[0]}-{i}" for i, c in enumerate(FIND)])
def test_find_overlaps_and_pairs_equal_the_reference_record_for_record(name, kw, resc, ppm):
    c, codes = _ctx_with(name)
    want, st = RC.reference(name, resc[0], resc[1], ppm, **{k: v for k, v in kw.items() if not (ppm and k == "max_occ")})
    fkw = _finder_kw(kw, ppm)
    c.set_seed_rescue(*resc)
    got = c.find_overlaps(**fkw)
    print(dict(name=name, resc=resc, ppm=ppm, cut=c.last_occ_cut, records=len(got[1]), want=len(want[1]), rescued=c.last_rescued))
    assert c.last_occ_cut == st["cut"] and c.last_rescued == int(st["rescued"].sum())
    for g, w, f in zip(got, want, ("rids", "rows", "aln_off", "scores")):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (name, f)
    assert [x.tobytes() for x in c.find_overlaps(**fkw)] == [x.tobytes() for x in got]
    # the pairs: the reference's records through pair_rows
    rids, rows, aln_off, scores = want
    prim, rec_of_row = api.pair_rows(rows, exact_ids=True)
    n = len(prim)
    fields = dict(primaries=rows[prim].reshape(n, 10), chain_scores=scores[prim], ext=np.zeros((n, 4), np.uint32), ext_scores=np.zeros((n, 2), np.int32),
                  rids=rids, aln_off=aln_off, rec_of_row=rec_of_row)
    p = c.find_overlap_pairs(extend=False, **fkw)
    PC.assert_same_fields(PC.pairs_fields(p), fields, (name, resc, ppm))
    assert p.rescued == int(st["rescued"].sum()) and p.occ_cut == st["cut"]
    p2 = c.find_overlap_pairs(extend=False, **fkw)
    assert PC.pairs_bytes(p2) == PC.pairs_bytes(p)
    t = c.pairs_from_table(p.primaries, p.chain_scores, p.rids, p.aln_off, p.rec_of_row)
    assert t.rescued == 0                                                  # a handle over the caller's table rescued nothing
    for x in (p, p2, t):
        x.close()
    if n:                                                                  # extended: the stepwise chain under the same setting
        pe = c.find_overlap_pairs(**fkw)
        PC.assert_same_fields(PC.pairs_fields(pe), PC.stepwise(c, dict(), **fkw), (name, "extended"))
        pe.close()


def test_sets_a_and_b_show_what_the_reference_shows():
    c, _ = _ctx_with("set_a")
    assert len(c.find_overlaps(**RC.A_KW)[1]) == 0 and c.last_rescued == 0
    got = c.find_overlaps(occ_dist=RC.A_RESCUE[0], rescue_max_occ=RC.A_RESCUE[1], **RC.A_KW)
    assert len(got[1]) == 2 * 780 and c.last_rescued == 790
    c, _ = _ctx_with("set_b")
    ro = RC.b_repeat_only()
    n = []
    for kw in (dict(), dict(occ_dist=RC.B_RESCUE[0], rescue_max_occ=RC.B_RESCUE[1])):
        p = c.find_overlap_pairs(extend=False, **kw, **RC.B_KW)
        n.append((p.n_pairs, int((np.isin(p.primaries[:, 0], ro) | np.isin(p.primaries[:, 5], ro)).sum())))
        p.close()
    assert n == [(12, 0), (28, 15)]


def test_the_stats_line():
    c, _ = _ctx_with("set_a")
    code = ("import os, sys; sys.path.insert(0, os.path.join(sys.argv[1], 'tests')); sys.path.insert(0, sys.argv[1])\n"
            "from herro_amd import api; import pair_cases as PC, rescue_cases as RC\n"
            "c = api.Context(0); PC.load(c, RC.get('set_a')[0])\n"
            "c.find_overlaps(**RC.A_KW); sys.stderr.write('SECOND\\n'); c.set_seed_rescue(*RC.A_RESCUE); c.find_overlaps(**RC.A_KW)\n")
    r = subprocess.run([sys.executable, "-c", code, G.ROOT], env=dict(os.environ, HERRO_OVL_STATS="1"), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    first, second = r.stderr.split("SECOND\n")
    assert "OVLRESC" not in first and re.findall(r"anchors=(\d+)", first)[0] == "263"
    assert re.findall(r"^OVLRESC high=(\d+) rescued=(\d+) anchors=(\d+)$", second, re.M) == [("23499", "790", str(15622 - 263))]
    assert re.findall(r"^OVL kmers=\d+ minimizers=(\d+) anchors=(\d+) ", second, re.M) == [("27625", "15622")]


# ---- 3. a core mask ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw,resc,ppm", [("streaks", RC.KW, RC.CASES["d100"], 0), ("streaks", RC.KW, RC.CASES["r_equal"], RC.PPM),
                                              ("set_b", RC.B_KW, RC.B_RESCUE, 0)], ids=["streaks", "streaks-frac", "set_b"])
def test_a_mask_selects_from_the_unmasked_result(name, kw, resc, ppm):
    c, codes = _ctx_with(name)
    n = len(codes)
    fkw = _finder_kw(kw, ppm)
    c.set_seed_rescue(*resc)
    full = c.find_overlap_pairs(**fkw)
    fields, rescued = PC.pairs_fields(full), full.rescued
    full.close()
    rows_full = c.find_overlaps(**fkw)
    assert rescued > 0 and len(fields["rec_of_row"]) > 0
    for mname in ("every3rd", "one"):
        m = CC.masks(n)[mname]
        p = c.find_overlap_pairs(core=m, **fkw)
        PC.assert_same_fields(PC.pairs_fields(p), CC.filter_pairs(fields, m), (name, mname))
        assert p.rescued == rescued and p.n_rows < len(fields["rec_of_row"])          # the selection saw no mask
        p.close()
        got = c.find_overlaps(core=m, **fkw)
        for g, w in zip(got, CC.filter_rows(*rows_full, m)):
            assert g.dtype == w.dtype and np.array_equal(g, w)


# ---- 4. the scratch budget --------------------------------------------------------------------------------------------------------------------
_CHILD = r"""
import json, os, sys
sys.path.insert(0, os.path.join(sys.argv[1], "tests")); sys.path.insert(0, sys.argv[1])
from herro_amd import api
import core_cases as CC
import pair_cases as PC
import rescue_cases as RC
c = api.Context(0)
PC.load(c, RC.get("set_a")[0])
c.set_seed_rescue(*RC.A_RESCUE)
p = c.find_overlap_pairs(**RC.A_KW)
out = dict(pairs=PC.pairs_bytes(p).hex(), rescued=p.rescued)
p2 = c.find_overlap_pairs(core=CC.masks(40)["every3rd"], **RC.A_KW)
out["core"], out["core_rescued"] = PC.pairs_bytes(p2).hex(), p2.rescued
print(json.dumps(out))
"""


def test_a_small_scratch_budget_gives_the_same_bytes():
    """set A with the rescue: 15 622 anchors, 2 MB of scratch, several chunks at 1 MiB"""
    c, codes = _ctx_with("set_a")
    env = dict(os.environ, HERRO_OVL_SCRATCH_MB="1", HERRO_OVL_STATS="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, G.ROOT], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    child = json.loads(r.stdout.strip().splitlines()[-1])
    chunks = [int(x) for x in re.findall(r"^OVL .* chunks=(\d+)$", r.stderr, re.M)]
    assert len(chunks) == 2 and chunks[0] >= 2, r.stderr[-500:]
    c.set_seed_rescue(*RC.A_RESCUE)
    p = c.find_overlap_pairs(**RC.A_KW)
    assert p.n_pairs == 780 and child["rescued"] == p.rescued == 790 and child["pairs"] == PC.pairs_bytes(p).hex()
    p.close()
    p = c.find_overlap_pairs(core=CC.masks(40)["every3rd"], **RC.A_KW)
    assert 0 < p.n_pairs < 780 and child["core_rescued"] == p.rescued == 790 and child["core"] == PC.pairs_bytes(p).hex()
    p.close()


# ---- 5. off ------------------------------------------------------------------------------------------------------------------------------------
def test_off_null_and_zero_are_a_context_that_never_had_the_setting():
    fresh = api.Context(0)
    for name, kws in (("set_b", (RC.B_KW,)), ("streaks", (RC.KW, _finder_kw(RC.KW, RC.PPM)))):
        rs = RC.get(name)[0]
        PC.load(fresh, rs)
        c, _ = _ctx_with(name)
        for kw in kws:
            want = [x.tobytes() for x in fresh.find_overlaps(**kw)]
            pw = fresh.find_overlap_pairs(**kw)
            want_p = PC.pairs_bytes(pw)
            pw.close()
            assert len(want[1]) > 0
            c.set_seed_rescue(200, 64)
            c.find_overlaps(**kw)
            assert c.last_rescued > 0                                                     # (the setting does something here)
            for off in (lambda: c.set_seed_rescue(None), lambda: c.set_seed_rescue(0), lambda: c.set_seed_rescue(0, 64),
                        lambda: c._chk(c._l.herro_set_seed_rescue(c.h, None))):
                c.set_seed_rescue(200, 64)
                off()
                assert [x.tobytes() for x in c.find_overlaps(**kw)] == want and c.last_rescued == 0
                p = c.find_overlap_pairs(**kw)
                assert PC.pairs_bytes(p) == want_p and p.rescued == 0
                p.close()
            got = c.find_overlaps(occ_dist=0, **kw)                                       # ... and the keyword at 0
            assert [x.tobytes() for x in got] == want
    fresh.close()
    with pytest.raises(api.HerroError) as e:
        c.find_overlaps(occ_dist=200, rescue_max_occ=65535, **RC.KW)
    assert e.value.code == -1 and "herro_set_seed_rescue" in str(e.value)


# ---- 6. reads to windows where there is no overlap without the rescue -------------------------------------------------------------------------
def test_set_a_reaches_the_windows_only_with_the_rescue():
    W = 256
    c = G.ctx()
    PC.load(c, RC.get("set_a")[0])
    p0 = c.find_overlap_pairs(**RC.A_KW)
    assert p0.n_pairs == 0 and p0.n_rows == 0 and p0.rescued == 0            # nothing to align, no window to build
    p0.close()
    p = c.find_overlap_pairs(occ_dist=RC.A_RESCUE[0], rescue_max_occ=RC.A_RESCUE[1], **RC.A_KW)
    m = p.align()
    assert p.n_pairs == 780 and p.rescued == 790 and m.failed == 0
    job = c.create_job_paired(p, m, W)
    job.featurize()
    n_alns = [job.info(w).n_alns for w in range(job.n_windows)]
    print(dict(windows=job.n_windows, alignments=sum(n_alns)))
    assert len(p.rids) == 40 and job.n_windows >= 40 and sum(1 for a in n_alns if a > 0) >= 40     # every read is a target with aligned windows
    for x in (job, m, p):
        x.close()
    p1 = c.find_overlap_pairs(**RC.A_KW)                                     # the keywords restored the shared context's setting: off
    assert p1.n_pairs == 0
    p1.close()
