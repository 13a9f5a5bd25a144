"""not-gpu: the table of tests/combo_cases.py reaches what tests/test_gpu_combo.py claims to test — on the composed reference alone.  The
references take the look-back (rescue_ref.find_overlaps_rescue, occ_ref.find_overlaps) and hand it on; the draw is balanced; enough trials
have a look-back that changes the answer, a rescue that did something below a fractional cut, a mask that drops a record and keeps one, a
chain group of more than 1024 anchors and more than one chunk at 1 MiB; and three wrong compositions each differ from the true one.  Every
test prints the counts behind its condition."""
import itertools
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import combo_cases as CB  # noqa: E402
import occ_ref as OR  # noqa: E402
import overlap_ref as R  # noqa: E402
import rescue_ref as RR  # noqa: E402

T = CB.trials()
ON = [t for t in T if t["rescue"] is not None]


def _numbers(ts):
    return [t["number"] for t in ts]


def _rescued(t) -> int:
    return int(CB.reference(t)[1]["rescued"].sum())


def _differs(t, other) -> bool:
    """the unmasked reference result of a trial against another composition of it: rows or scores"""
    return not CB.same_rows(CB.reference(t)[0], other[0])


# ---- 1. the references state the combination ------------------------------------------------------------------------------------------------
def test_the_references_take_the_lookback_and_hand_it_on():
    codes = CB.reads("T0+T2")[3]
    kw = dict(k=15, w=5, max_occ=64, min_score=60)
    plain = {H: R.find_overlaps(codes, lookback=H, **kw) for H in (64, 256)}
    assert not CB.same_rows(plain[64], plain[256])                                     # (the look-back matters on this set)
    for H in (64, 256):
        assert CB.same_rows(RR.find_overlaps_rescue(codes, 0, lookback=H, **kw), plain[H])
    assert CB.same_rows(RR.find_overlaps_rescue(codes, 0, **kw), plain[64])            # the default stays 64
    st = {}
    with_ppm = RR.find_overlaps_rescue(codes, 0, None, CB.PPM, stats=st, lookback=256, **kw)
    got, cut = OR.find_overlaps(codes, CB.PPM, lookback=256, **kw)
    assert cut == st["cut"] == 10 and CB.same_rows(got, with_ppm)
    assert CB.same_rows(OR.find_overlaps(codes, CB.PPM, **kw)[0], RR.find_overlaps_rescue(codes, 0, None, CB.PPM, **kw))
    a = RR.find_overlaps_rescue(codes, 100, lookback=64, **kw)
    b = RR.find_overlaps_rescue(codes, 100, lookback=256, **kw)
    assert CB.same_rows(a, RR.find_overlaps_rescue(codes, 100, **kw)) and not CB.same_rows(a, b)
    assert CB.same_rows(RR.find_overlaps_rescue(codes, 100, lookback=256, _lookback_64=True, **kw), a)
    for fn in (lambda: R.params(lookback=256), lambda: RR.find_overlaps_rescue(codes, 100, look_back=256, **kw)):
        with pytest.raises(TypeError):                                                 # the name stays out of overlap_ref.params; a misspelt one is refused
            fn()
    assert R.anchors is RR._PLAIN_ANCHORS


# ---- 2. the table -----------------------------------------------------------------------------------------------------------------------------
def test_the_table_is_seeded_small_and_balanced():
    assert len(T) == CB.N_TRIALS == 48 and T == CB.trials() and all(CB.trial(t["number"]) == t for t in T)
    drawn = {name: {repr(v) for v in col} for name, col in CB._table().items()}
    assert all(drawn[name] == {repr(v) for v in pool} for name, pool in CB.COLUMNS.items())          # every value of every pool is drawn
    for name in sorted(set(CB.SETS)):
        codes = CB.reads(name)[3]
        lens = [len(c) for c in codes]
        assert len(codes) <= 42 and max(lens) <= 6000, name                                         # (set_a has 40 reads, streaks 42, T1 reads of 6 kb)
        if name in CB.GENERATED:
            assert len(codes) == 12 and max(lens) <= 3000 and lens[10] == 17 and len(R.sketch(codes[10], 15, 5)[0]) == 0
            seq, _, off, _ = CB.reads(name)
            assert set(bytes(seq[int(off[11]):int(off[12])])) - set(b"ACGT") == {ord("N"), ord("R")}
    pairs = {(a, b): sum(1 for t in T if CB.KINDS[a](t) and CB.KINDS[b](t)) for a, b in itertools.combinations(CB.KINDS, 2)}
    print("trials in which two option kinds meet:", pairs)
    assert min(pairs.values()) >= 4, pairs
    for name, pool in (("lookback", CB.LOOKBACK), ("rescue", CB.RESCUE), ("max_occ", CB.MAX_OCC), ("extend", CB.EXTEND)):
        assert all(sum(1 for v in CB._table()[name] if v == x) >= 4 for x in pool), name


# ---- 3. the conditions ------------------------------------------------------------------------------------------------------------------------
def test_the_lookback_changes_the_answer_under_the_rescue():
    far = [t for t in ON if t["lookback"] > 64]
    from_64 = [t for t in far if _differs(t, CB.reference(t, lookback=64))]
    from_off = [t for t in far if _differs(t, CB.reference(t, rescue=None))]
    print(dict(far_and_rescue=len(far), differ_from_lookback_64=_numbers(from_64), differ_from_rescue_off=_numbers(from_off)))
    assert len(from_64) >= 8 and len(from_off) >= 8


def test_the_rescue_did_something_below_a_fractional_cut():
    frac = [t for t in ON if t["ppm"]]
    did = [t for t in frac if _rescued(t) > 0 and CB.reference(t)[1]["cut"] < t["fkw"]["max_occ"]]
    print(dict(frac_and_rescue=len(frac), rescued_below_max_occ=[(t["number"], CB.reference(t)[1]["cut"], t["fkw"]["max_occ"], _rescued(t)) for t in did]))
    assert len(did) >= 6


def test_the_mask_drops_a_record_and_keeps_one():
    masked = [t for t in T if t["core"] is not None]
    both = [t for t in masked if 0 < len(CB.expected_rows(t)[1]) < len(CB.reference(t)[0][1])]
    print(dict(masked=len(masked), lose_and_keep=[(t["number"], len(CB.reference(t)[0][1]), len(CB.expected_rows(t)[1])) for t in both]))
    assert len(both) >= 6


def test_long_chain_groups_exist_under_the_rescue():
    big = [(t["number"], t["lookback"], int(CB.group_sizes(t).max())) for t in ON if _rescued(t) > 0 and len(CB.group_sizes(t)) and CB.group_sizes(t).max() > 1024]
    print(dict(groups_past_1024=big, at_lookback_1024=[b for b in big if b[1] == 1024]))
    assert len(big) >= 6
    for t in T:                                                                          # the anchors the groups are taken from are the reference's
        assert len(CB.anchors(t)[0]) == CB.reference(t)[1]["anchors"] and CB.anchors(t)[1] == CB.reference(t)[1]["cut"], CB.tag(t)


def test_a_budget_of_1_mib_cuts_several_chunks():
    small = [(t["number"], CB.chunks(t)) for t in T if t["budget"] and CB.chunks(t) > 1]
    print(dict(budget_trials=sum(1 for t in T if t["budget"]), several_chunks=small))
    assert len(small) >= 6 and all(t["budget"] in (None, 1) for t in T)
    assert all(CB.chunks(t, 4096) <= 1 for t in T)


# ---- 4. the comparison has teeth ------------------------------------------------------------------------------------------------------------
def test_three_wrong_compositions_differ_from_the_true_one():
    def rows_differ(t, **switch):
        return not CB.same_rows(CB.expected_rows(t), CB.expected_rows(t, CB.reference(t, **switch)))
    at_64 = [t for t in ON if t["lookback"] > 64 and rows_differ(t, _lookback_64=True)]
    band = [t for t in ON if t["ppm"] and rows_differ(t, _band_from_max_occ=True)]
    targets = []
    for t in T:
        if t["core"] is not None:
            u = dict(t, extend=None)                                                     # (the mask does not look at the extension)
            if not CB.same_pairs(CB.expected_pairs(u), CB.expected_pairs(u, _targets_only=True)):
                targets.append(t)
    print(dict(chained_at_64=_numbers(at_64), band_from_max_occ=_numbers(band), mask_on_targets_only=_numbers(targets)))
    assert len(at_64) >= 5 and len(band) >= 5 and len(targets) >= 5
    for t in band:                                                                       # the wrong band keeps the cut and moves the rescue's lower edge
        st, wrong = CB.reference(t)[1], CB.reference(t, _band_from_max_occ=True)[1]
        assert wrong["cut"] == st["cut"] < t["fkw"]["max_occ"] and wrong["anchors"] != st["anchors"]
