"""gpu: the frequency cut taken from the index (occ_frac_ppm of herro_overlap_params; k_occ_census, k_occ_pick, k_runs_occ in
csrc/overlap_dev.hip; DESIGN.md §10, "The cut as a fraction").  The yardstick is tests/occ_ref.py over tests/overlap_ref.py: the census and
its four figures bin for bin, find_overlaps record for record, the pair and core entries against the stepwise chain with the same
parameter, one scratch budget against another byte for byte, and reads to FASTA on a set the fixed cut finds nothing in.
Read sets: tests/occ_cases.py."""
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
import occ_cases as OC  # noqa: E402
import occ_ref as OR  # noqa: E402
import pair_cases as PC  # noqa: E402
from herro_amd import api, shard, synth  # noqa: E402

pytestmark = pytest.mark.gpu

K25 = dict(k=25, w=17, min_score=100)
K15 = dict(k=15, w=5, min_score=60)
DEEP25 = OC.DEEP_KW[1]


def _ctx_with(name):
    c = G.ctx()
    PC.load(c, OC.get(name)[0])
    return c, OC.get(name)[1]


# ---- 1. the census and the pick ---------------------------------------------------------------------------------------------------------------
CENSUS = [
    ("depth33", K25, 5000, dict(cut=25)),
    ("depth33", K15, 5000, dict(cut=29)),
    ("depth33", K25, 500, dict(cut=26, cut_runs=2)),                  # no tie at the rank of the pick: one rank higher is 27
    ("depth33", dict(K15, max_occ=20), 5000, dict(cut=20)),           # the ceiling
    ("four", K15, 500000, dict(cut=10, cut_runs=0)),                  # q = 1: the floor
    ("ac_mixed", K25, 5000, dict(cut=25, cut_runs=13)),               # one run of ~70 000 in the last bin: the cut of depth33 all the same
    ("ac_mixed", K15, 5000, dict(cut=29)),
    ("ac_only", K25, 5000, dict(cut=65534, distinct=1, cut_runs=1)),  # only the last bin holds a run: never usable
    ("no_minimizers", K25, 5000, dict(cut=10, distinct=0, cut_runs=0, cut_minimizers=0)),
    ("no_minimizers", K15, 5000, dict(cut=10, distinct=13)),          # (k + w - 1 = 19: three of the four reads have windows)
]


@pytest.mark.parametrize("name,kw,ppm,expect", CENSUS, ids=[f"{n}-{i}" for i, (n, _, _, _) in enumerate(CENSUS)])
def test_the_census_and_its_figures_equal_the_reference(name, kw, ppm, expect):
    c, codes = _ctx_with(name)
    want_hist, want = OR.census(codes, ppm, **kw)
    hist, got = c.occ_census(occ_frac_ppm=ppm, **kw)
    print(dict(name=name, ppm=ppm, got=got, last_bin=int(hist[65535])))
    assert got == want and {f: want[f] for f in expect} == expect
    assert hist.dtype == want_hist.dtype and np.array_equal(hist, want_hist)
    assert int(hist.sum()) == got["distinct"]
    if name.startswith("ac_"):
        assert hist[65535] == 1 and got["cut_minimizers"] >= 69000 + int(hist[got["cut"] + 1:65535].sum())   # the long run's true length is in the figure
    hist2, got2 = c.occ_census(occ_frac_ppm=ppm, **kw)
    assert got2 == got and hist2.tobytes() == hist.tobytes()


def test_two_reads_of_one_repeat_give_no_records():
    c, codes = _ctx_with("ac_only")
    for kw in (K25, K15):
        rids, rows, aln_off, scores = c.find_overlaps(occ_frac_ppm=OC.PPM, **kw)
        assert c.last_occ_cut == 65534 and len(rids) == len(rows) == len(scores) == 0 and aln_off.tolist() == [0]
        p = c.find_overlap_pairs(occ_frac_ppm=OC.PPM, **kw)
        assert p.occ_cut == 65534 and p.n_pairs == p.n_rows == 0
        p.close()


# ---- 2. find_overlaps -------------------------------------------------------------------------------------------------------------------------
FIND = [
    ("deep", DEEP25, 5000, 180, 2 * OC.DEEP_PAIRS),                   # a cut above 128: the fixed cut finds nothing here
    ("depth33", K25, 5000, 25, 2 * 528),                              # a cut below 128
    ("depth33", K15, 5000, 29, 2 * 528),
    ("depth33", K25, 500, 26, 2 * 528),
    ("low", dict(k=15, w=5, min_score=60), 5000, 13, 2 * 78),
    ("low", dict(k=15, w=5, min_score=60), 20000, 10, 2 * 78),
    ("low", dict(min_score=100), 5000, 10, 2 * 75),
    ("low", dict(min_score=100), 20000, 10, 2 * 75),
    ("four", K15, 500000, 10, 12),                                    # the floor decides
    ("depth33", dict(K15, max_occ=20), 5000, 20, 2 * 521),            # a ceiling below q
]


@pytest.mark.parametrize("name,kw,ppm,cut,n", FIND, ids=[f"{c[0]}-{i}" for i, c in enumerate(FIND)])
def test_find_overlaps_equals_the_reference_record_for_record(name, kw, ppm, cut, n):
    c, codes = _ctx_with(name)
    want, want_cut, _ = OC.reference(name, ppm, **kw)
    assert want_cut == cut and len(want[1]) == n
    got = c.find_overlaps(occ_frac_ppm=ppm, **kw)
    assert c.last_occ_cut == cut
    for g, w, f in zip(got, want, ("rids", "rows", "aln_off", "scores")):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (name, f)
    again = c.find_overlaps(occ_frac_ppm=ppm, **kw)
    assert [x.tobytes() for x in again] == [x.tobytes() for x in got]
    if name == "deep":                                                        # the same call with today's fixed cut: nothing
        assert len(c.find_overlaps(**kw)[1]) == 0 and c.last_occ_cut == 128


# ---- 3. pairs and a core mask -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw", [("depth33", K25), ("deep", DEEP25), ("low", dict(k=15, w=5, min_score=60))])
def test_pairs_equal_the_stepwise_chain_and_a_mask_selects(name, kw):
    c, codes = _ctx_with(name)
    n = len(codes)
    kwf = dict(kw, occ_frac_ppm=OC.PPM)
    for ext in (dict(), None):
        want = PC.stepwise(c, ext, **kwf)
        cut = c.last_occ_cut
        full = c.find_overlap_pairs(**kwf) if ext is not None else c.find_overlap_pairs(extend=False, **kwf)
        PC.assert_same_fields(PC.pairs_fields(full), want, (name, ext))
        assert full.occ_cut == cut == OC.reference(name, OC.PPM, **kw)[1] and full.n_pairs > 0
        fields = PC.pairs_fields(full)
        full.close()
        for mname in ("every3rd", "one"):
            m = CC.masks(n)[mname]
            p = c.find_overlap_pairs(core=m, **kwf) if ext is not None else c.find_overlap_pairs(extend=False, core=m, **kwf)
            PC.assert_same_fields(PC.pairs_fields(p), CC.filter_pairs(fields, m), (name, ext, mname))
            assert p.occ_cut == cut and 0 < p.n_rows < len(fields["rec_of_row"])     # the cut is the unmasked one
            p.close()
    m = CC.masks(n)["every3rd"]
    got = c.find_overlaps(core=m, **kwf)
    assert c.last_occ_cut == cut
    for g, w in zip(got, CC.filter_rows(*c.find_overlaps(**kwf), m)):
        assert g.dtype == w.dtype and np.array_equal(g, w)


# ---- 4. the scratch budget --------------------------------------------------------------------------------------------------------------------
_CHILD = r"""
import json, os, sys
sys.path.insert(0, os.path.join(sys.argv[1], "tests")); sys.path.insert(0, sys.argv[1])
from herro_amd import api
import occ_cases as OC
import pair_cases as PC
c = api.Context(0)
PC.load(c, OC.deep())
kw = dict(OC.DEEP_KW[1], occ_frac_ppm=OC.PPM)
p = c.find_overlap_pairs(**kw)
out = dict(pairs=PC.pairs_bytes(p).hex(), cut=p.occ_cut)
sys.stderr.write("SECOND\n")
p2 = c.find_overlap_pairs(core=OC.deep_core(), **kw)
out["core"], out["core_cut"] = PC.pairs_bytes(p2).hex(), p2.occ_cut
print(json.dumps(out))
"""


def test_a_small_scratch_budget_gives_the_same_bytes_and_the_same_cut():
    """the deep set at (25, 17): 560 466 anchors, 72 MB of scratch, in many chunks at 1 MiB"""
    c, codes = _ctx_with("deep")
    kw = dict(DEEP25, occ_frac_ppm=OC.PPM)
    env = dict(os.environ, HERRO_OVL_SCRATCH_MB="1", HERRO_OVL_STATS="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, G.ROOT], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    child = json.loads(r.stdout.strip().splitlines()[-1])
    first, second = r.stderr.split("SECOND\n")
    ovl = [ln for ln in first.splitlines() if ln.startswith("OVL")]
    assert len(ovl) == 2, first[-500:]
    m = re.fullmatch(r"OVL kmers=(\d+) minimizers=(\d+) anchors=(\d+) groups=(\d+) chained=(\d+) chunks=(\d+)", ovl[0])     # today's line
    assert m and int(m.group(3)) == 560466 and int(m.group(6)) >= 8, ovl
    assert ovl[1] == "OVLOCC cut=180 distinct=915 cut_runs=3 cut_minimizers=556", ovl
    assert re.findall(r"OVLOCC cut=(\d+) distinct=(\d+)", second) == [("180", "915")]                                     # the cut of the whole store
    p = c.find_overlap_pairs(**kw)
    assert p.n_pairs == OC.DEEP_PAIRS and child["cut"] == p.occ_cut == 180 and child["pairs"] == PC.pairs_bytes(p).hex()
    p.close()
    p = c.find_overlap_pairs(core=OC.deep_core(), **kw)
    assert p.n_pairs == 8 * 199 - 8 * 7 // 2 and child["core_cut"] == p.occ_cut == 180 and child["core"] == PC.pairs_bytes(p).hex()
    p.close()


# ---- 5. reads to FASTA where the fixed cut finds nothing --------------------------------------------------------------------------------------
def test_reads_to_fasta_on_the_deep_set_for_eight_core_targets():
    W = 256
    c, codes = _ctx_with("deep")
    rs = OC.get("deep")[0]
    core = OC.deep_core()
    assert c.find_overlap_pairs(core=core, **DEEP25).n_pairs == 0                         # today's cut: nothing to correct with
    p = c.find_overlap_pairs(core=core, occ_frac_ppm=OC.PPM, **DEEP25)
    m = p.align()
    assert p.occ_cut == 180 and p.rids.tolist() == np.flatnonzero(core).tolist() and p.n_rows == 8 * 199 and m.failed == 0
    job = c.create_job_paired(p, m, W)
    j_rids, off2, rec = api.paired_job_args(p.rids, p.aln_off, p.rec_of_row, m.ok)
    assert (np.diff(off2.astype(np.int64)) == 199).all()
    rows2 = m.rows[rec]
    cig2 = [m.cigar(int(r)) for r in rec]
    p.close()
    m.close()
    job.featurize()
    # the oracle fed the GPU's rows and CIGARs
    lens = np.array([len(x) for x in cig2], np.uint64)
    rows10 = rows2.astype(np.uint32).copy()
    rows10[:, 9] = lens
    sb = synth.SynthBatch(seq=rs.seq, qual=rs.qual, off=rs.off, aln=rows10, cig=np.frombuffer(b"".join(cig2) + b"\0", np.uint8).copy(),
                          cig_off=np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64), tgt_aln_off=off2, tgt_rid=j_rids)
    store = G.O.store_from_synth(sb)
    assert G.compare_features(job, sb, store, W) == job.n_windows > 0
    job.infer(64, 0)
    job.consensus()
    w = n_fasta = 0
    for t in range(sb.n_targets):
        rid, orows, ocigs = G.O.target_alignments(sb, t)
        res = store.extract_features(rid, orows, ocigs, W)
        lg = [job.logits(w + wi)[1] for wi in range(len(res)) if job.info(w + wi).n_supported]
        w += len(res)
        lg = np.concatenate(lg) if lg else np.zeros((0, 5), np.float32)
        got = job.consensus_fasta(t, sb.read_name(rid))
        assert got == res.consensus_fasta(lg), f"FASTA mismatch, target {t}"
        n_fasta += got.count(">")
    assert n_fasta >= 8
    # ... and a shard's run takes the parameter through its finder keywords: the same targets, the same text
    text, ends = job.fasta([f"read{int(r)}" for r in j_rids], with_ends=True)
    job.close()
    rec = shard.correct_reads_shard(c, core, W, 64, 0, lambda r: f"read{r}", occ_frac_ppm=OC.PPM, **DEEP25)
    assert np.array_equal(rec[0], j_rids) and np.array_equal(rec[1], ends) and bytes(rec[2]) == text and text.count(b">") == n_fasta
    assert len(shard.correct_reads_shard(c, core, W, 64, 0, lambda r: f"read{r}", **DEEP25)[0]) == 0     # today's cut: no target at all


# ---- 6. the field at 0 ------------------------------------------------------------------------------------------------------------------------
def test_the_field_at_zero_is_the_entry_without_it():
    c = G.ctx()
    PC.load(c, PC.set_d())
    for kw in (PC.DEFAULTS, PC.SMALL_K):
        want = c.find_overlaps(**kw)
        assert len(want[1]) > 0 and c.last_occ_cut == 64
        got = c.find_overlaps(occ_frac_ppm=0, **kw)
        assert [x.tobytes() for x in got] == [x.tobytes() for x in want] and c.last_occ_cut == 64
        a, b = c.find_overlap_pairs(**kw), c.find_overlap_pairs(occ_frac_ppm=0, **kw)
        assert PC.pairs_bytes(a) == PC.pairs_bytes(b) and a.occ_cut == b.occ_cut == 64
        t = c.pairs_from_table(a.primaries, a.chain_scores, a.rids, a.aln_off, a.rec_of_row)
        assert t.occ_cut == 0                                                 # a handle over the caller's table used no cut
        for x in (a, b, t):
            x.close()
    assert len(c.find_overlaps(min_score=100)[1]) > 0 and c.last_occ_cut == 128          # the default
    with pytest.raises(api.HerroError) as e:
        c.find_overlaps(occ_frac_ppm=10**6)
    assert e.value.code == -1 and "occ_frac_ppm" in str(e.value)
    with pytest.raises(api.HerroError) as e:
        c.occ_census(**PC.DEFAULTS)
    assert e.value.code == -1 and "occ_frac_ppm is 0" in str(e.value)
