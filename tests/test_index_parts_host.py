"""cpu: the overlap finder's index in parts (herro_set_index_params; DESIGN.md §10, "An index in parts") — the decomposition restated in numpy
(tests/index_parts_ref.py) against the UNPARTITIONED specification on the combination trials (tests/combo_cases.py), three mutants of it that each
change the result, and the host half of the library: herro_index_plan and herro_set_index_params through a context without a device."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import combo_cases as CB  # noqa: E402
import index_parts_ref as IP  # noqa: E402
from herro_amd import api  # noqa: E402

# Chosen by number so that the fraction cut, the rescue, a look-back past 64, a core mask and both (k, w) occur at least three times each, over
# twelve different read sets (tests/test_gpu_index_parts.py runs the same trials on the device).
TRIALS = [1, 4, 8, 10, 11, 13, 15, 16, 23, 29, 32, 34, 37, 44]
MUTANT_TRIAL = 23           # G7, k = 15: fraction cut, rescue, look-back 128 — every mutant changes its result
BLOCKS = {"B": 5, "C": 2, "D": 6, "G7": 6, "G20": 6, "G40": 6, "G150": 6, "T0+T2": 4, "T1": 2, "T2+T3": 4, "T3": 2, "set_a": 4, "set_b": 5, "streaks": 5}
OVL_MAX_KMERS = 0xFFFFF000


def _lens(t):
    return np.array([len(c) for c in CB.reads(t["set"])[3]], np.int64)


def total_kmers(t) -> int:
    return int(IP.read_kmers(_lens(t), t["fkw"]["k"], t["fkw"]["w"]).sum())


def quarter(t) -> int:
    """the part size of most tests: 2 ceil(total / 4) k-mers, 2 to 6 blocks on every set"""
    return 2 * -(-total_kmers(t) // 4)


def parts(t, max_kmers, ranges=1, **mutant):
    d, rmax = t["rescue"] or (0, None)
    st = {}
    got = IP.find_overlaps_parts(CB.reads(t["set"])[3], max_kmers, ranges, d, rmax, t["ppm"], lookback=t["lookback"], stats=st, **mutant, **t["fkw"])
    return got, st


def test_the_trials_cover_every_option_three_times():
    T = [CB.trial(n) for n in TRIALS]
    assert len(T) >= 12 and len({t["set"] for t in T}) >= 12
    for kind in ("frac", "rescue", "far", "core", "k25"):
        assert sum(1 for t in T if CB.KINDS[kind](t)) >= 3, kind
    assert sum(1 for t in T if not CB.KINDS["k25"](t)) >= 3


def test_the_block_rule_gives_the_block_counts_of_the_table():
    for t in CB.trials():
        cuts = IP.block_cuts(_lens(t), t["fkw"]["k"], t["fkw"]["w"], quarter(t))
        assert len(cuts) - 1 == BLOCKS[t["set"]], CB.tag(t)


@pytest.mark.parametrize("number", TRIALS)
def test_the_decomposition_equals_the_unpartitioned_reference(number):
    t = CB.trial(number)
    want, wst = CB.reference(t)
    total = total_kmers(t)
    n_with_kmers = int((IP.read_kmers(_lens(t), t["fkw"]["k"], t["fkw"]["w"]) > 0).sum())
    for max_kmers, ranges, blocks in ((quarter(t), 3, BLOCKS[t["set"]]), (1, 16, n_with_kmers), (2 * total, 1, 1)):
        got, st = parts(t, max_kmers, ranges)
        tag = (CB.tag(t), max_kmers, ranges)
        assert st["blocks"] == blocks, tag
        assert CB.same_rows(got, want), tag
        assert st["cut"] == wst["cut"] and np.array_equal(st["rescued"], wst["rescued"]), tag
        assert np.array_equal(st["occ"], np.minimum(wst["occ"], 65535)), tag


def test_the_ranges_of_the_occurrence_pass_give_the_same_occurrences():
    import overlap_ref as R
    import rescue_ref as RR
    for name, k, w in (("streaks", 15, 5), ("G7", 25, 17), ("D", 15, 5)):
        h = R.sketch_store(CB.reads(name)[3], k, w)[0]
        want = RR.occurrences(h)
        counts = np.sort(np.unique(h, return_counts=True)[1])
        for ranges in (1, 3, 16, 65536):
            occ, c = IP.occurrences_by_range(h, k, ranges)
            assert np.array_equal(occ, want) and np.array_equal(np.sort(c), counts), (name, ranges)


@pytest.mark.parametrize("mutant", ["_local_length", "_local_classes", "_same_block"])
def test_a_mutant_of_the_decomposition_changes_the_result(mutant):
    """a run judged by its length inside the block pair; U / H / transparent from the counts inside the pair; same-block anchors once more in the
    pairs i < j — each is a different finder on this trial"""
    t = CB.trial(MUTANT_TRIAL)
    assert t["rescue"] is not None
    want = CB.reference(t)[0]
    assert CB.same_rows(parts(t, quarter(t))[0], want)
    assert not CB.same_rows(parts(t, quarter(t), **{mutant: True})[0], want)


# ---- herro_index_plan and herro_set_index_params on a context without a device ----------------------------------------------------------------
def _host():
    return api.HostContext(np.array([100, 200], np.uint32))


def test_the_plan_equals_the_block_rule_on_the_combination_sets():
    c = _host()
    for t in CB.trials():
        k, w = t["fkw"]["k"], t["fkw"]["w"]
        lens = _lens(t)
        for max_kmers in (quarter(t), 1, 0, 2 * total_kmers(t), 1000, 7001):
            assert api.index_plan(lens, k, w, max_kmers, ctx=c).tolist() == IP.block_cuts(lens, k, w, max_kmers), (CB.tag(t), max_kmers)
    assert api.index_plan(_lens(CB.trial(0)), 15, 5, 1).tolist() == api.index_plan(_lens(CB.trial(0)), 15, 5, 1, ctx=c).tolist()


def test_the_plan_at_its_edges():
    c = _host()
    k, w = 25, 17                                    # a read has k-mers from 41 bases on
    plan = lambda lens, m: api.index_plan(np.array(lens, np.uint32), k, w, m, ctx=c).tolist()      # noqa: E731
    assert plan([], 1000) == [0]                                                   # an empty store: no block
    assert plan([40, 10], 1000) == [0, 2]                                          # no read has k-mers: one block all the same
    # a read longer than cap is a block alone: cap = 500 k-mers, read 1 has 4976
    assert plan([100, 5000, 100, 100], 1000) == [0, 1, 2, 4]
    assert plan([5000], 2) == [0, 1]
    # reads without k-mers at the front, in the middle and at the end never open a block (cap 100: the reads of 124 bases have 100 k-mers)
    assert plan([30, 40, 124, 40, 30, 124, 124, 40, 40], 200) == [0, 5, 6, 9]
    assert plan([30, 124, 40], 1) == [0, 3]
    assert plan([124, 40, 124], 1) == [0, 2, 3]
    for lens, m in (([30, 40, 124, 40, 30, 124, 124, 40, 40], 200), ([100, 5000, 100, 100], 1000), ([41] * 7, 3), ([41] * 7, 4), ([41] * 7, 5)):
        assert plan(lens, m) == IP.block_cuts(lens, k, w, m), (lens, m)


def test_a_100_gbase_length_table_stays_within_the_limit():
    """lengths only, five million of them under a seed: at max_kmers = 2^32 - 4096 no block pair exceeds OVL_MAX_KMERS"""
    rng = np.random.default_rng(1003)
    lens = np.minimum(rng.lognormal(9.7, 0.6, 5_000_000), 2_000_000).astype(np.uint32)
    lens[::100_000] = rng.integers(0, 40, 50)                                      # some reads without k-mers
    assert 95e9 < int(lens.sum(dtype=np.uint64)) < 130e9
    k, w = 25, 17
    cuts = api.index_plan(lens, k, w, OVL_MAX_KMERS)
    assert cuts[0] == 0 and cuts[-1] == len(lens) and (np.diff(cuts.astype(np.int64)) > 0).all()
    nk = IP.read_kmers(lens, k, w)
    per = np.add.reduceat(nk, cuts[:-1].astype(np.int64))
    cap = OVL_MAX_KMERS // 2
    assert 40 < len(per) < 80 and int(per.sum()) == int(nk.sum()) > 2**32
    assert per.max() <= cap and int(np.sort(per)[-2:].sum()) <= OVL_MAX_KMERS        # every block pair fits one index
    # the rule: a block ends where the next read with k-mers would take it past cap
    nxt = np.array([nk[int(c):][np.flatnonzero(nk[int(c):])[0]] for c in cuts[1:-1]])
    assert (per[:-1] + nxt > cap).all()


def test_two_blocks_past_the_limit_are_refused_with_their_first_reads():
    c = _host()
    lens = np.array([1000, 0x7FFFFFFF, 500, 0x7FFFFFFF, 100], np.uint32)
    with pytest.raises(api.HerroError) as e:
        api.index_plan(lens, 25, 17, 1 << 20, ctx=c)
    assert e.value.code == -4 and "reads 1 and 3" in str(e.value) and "2^32 k-mers" in str(e.value)
    assert api.index_plan(lens[:3], 25, 17, 1 << 20, ctx=c).tolist() == [0, 1, 2, 3]
    for bad in (dict(k=4), dict(k=32), dict(w=0), dict(w=65), dict(max_kmers=OVL_MAX_KMERS + 1)):
        with pytest.raises(api.HerroError) as e:
            api.index_plan(lens[:1], **dict(dict(k=25, w=17, max_kmers=5), **bad), ctx=c)
        assert e.value.code == -1 and "herro_index_plan" in str(e.value)


def test_the_setting_is_checked_without_a_device_and_a_refused_call_leaves_it():
    c = _host()
    c.set_index_parts(12345, 7)
    assert c._index_parts == (12345, 7)
    for bad in ((OVL_MAX_KMERS + 1, 0), (1 << 40, 0), (1000, 65537), (0, 65537)):
        with pytest.raises(api.HerroError) as e:
            c.set_index_parts(*bad)
        assert e.value.code == -1 and "herro_set_index_params: max_kmers <= 2^32 - 4096" in str(e.value) and "occ_ranges <= 65536" in str(e.value)
        assert c._index_parts == (12345, 7)
    p = api.IndexParams(max_kmers=5, occ_ranges=0, reserved=1)
    assert c._l.herro_set_index_params(c.h, api.C.byref(p)) == -1 and "reserved 0" in c.last_error()
    c.set_index_parts(OVL_MAX_KMERS, 65536)                                        # the largest legal values
    c.set_index_parts(None)
    assert c._index_parts == (0, 0)
    # the finder itself still answers as on any context without a device — after the parameters were accepted
    with pytest.raises(api.HerroError) as e:
        c.find_overlaps(index_kmers=1000, occ_ranges=3)
    assert e.value.code == -2 and c._index_parts == (0, 0)
    with pytest.raises(api.HerroError) as e:
        c.find_overlaps(index_kmers=OVL_MAX_KMERS + 1)
    assert e.value.code == -1 and c._index_parts == (0, 0)


def test_the_new_entries_are_exported():
    names = ("herro_set_index_params", "herro_overlaps_index_blocks", "herro_pairs_index_blocks", "herro_index_plan")
    L = api.lib()
    for n in names:
        assert n in api.EXPORTS and hasattr(L, n), n
    with open(os.path.join(os.path.dirname(HERE), "herro_amd", "csrc", "herro_amd.map")) as f:
        assert "herro_*" in f.read()                                               # the version script exports the C ABI by its prefix
    with open(os.path.join(os.path.dirname(HERE), "include", "herro_amd.h")) as f:
        header = f.read()
    for n in names:
        assert n + "(" in header, n
    assert api.C.sizeof(api.IndexParams) == 16
