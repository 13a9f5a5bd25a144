"""The rescue of high-frequency minimizers without a GPU (herro_set_seed_rescue; DESIGN.md §10, "Rescue of high-frequency minimizers"): the
census that shows every read set of tests/rescue_cases.py reaches what it claims, hand cases for the rounding of m and the tie rule, what the
rule does on sets A and B under the reference alone, and the setter's error codes on a context without a device."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import overlap_ref as R  # noqa: E402
import rescue_cases as RC  # noqa: E402
import rescue_ref as RR  # noqa: E402
from herro_amd import api  # noqa: E402

CUT = RC.KW["max_occ"]


def _census(case, cut=CUT):
    return RC.streak_census("streaks", cut, *RC.CASES[case])


# ---- 1. the cases reach what they claim -------------------------------------------------------------------------------------------------------
def test_streak_sizes_on_either_side_of_a_block_of_64():
    c = _census("d100")
    partial = [s["size"] for s in c if 0 < s["m"] < s["size"]]
    print(sorted(partial))
    assert any(n <= 63 for n in partial) and 64 in partial and 65 in partial and any(n >= 129 for n in partial)
    by_read = {s["read"]: s for s in c if s["read"] in (0, 1, 2, 3)}
    assert [by_read[r]["size"] for r in (0, 1, 2, 3)] == [45, 64, 65, 451] and [by_read[r]["m"] for r in (0, 1, 2, 3)] == [2, 2, 2, 13]


def test_quota_above_the_size_and_at_zero():
    assert all(s["m"] >= s["size"] for s in _census("d1")) and len(_census("d1")) > 20
    assert all(s["m"] == 0 for s in _census("d_big"))
    for case in ("d100", "d200"):
        short = [s for s in _census(case) if s["read"] == 12]
        assert [(s["size"], s["m"]) for s in short] == [(2, 0)]           # H[:20] between two U: too short for one minimizer


def test_streaks_at_the_ends_of_a_read_and_reads_without_u():
    c = _census("d100")
    first = [s for s in c if s["read"] == 4][0]
    assert first["ps"] == 0 and first["pe"] < first["len"] and 0 < first["m"] < first["size"]
    last = [s for s in c if s["read"] == 5][-1]
    assert last["pe"] == last["len"] and last["ps"] > 0 and 0 < last["m"] < last["size"]
    whole = [s for s in c if s["read"] == 6]
    assert len(whole) == 1 and whole[0]["n_u"] == 0 and whole[0]["ps"] == 0 and whole[0]["pe"] == whole[0]["len"] and 0 < whole[0]["m"] < whole[0]["size"]
    h, rid, pos, st, lens = RC.sketch("streaks")
    assert lens[7] < RC.KW["k"] + RC.KW["w"] - 1 and not (rid == 7).any()


def test_transparent_minimizers_inside_a_streak():
    eight = [s for s in _census("d100") if s["read"] == 8]
    assert len(eight) == 1 and (eight[0]["inner"] == 1).sum() >= 10                       # the private bases end no streak
    for case, rmax in (("r_equal", 16), ("r_above", 29)):
        nine = [s for s in _census(case) if s["read"] == 9]
        assert len(nine) == 1 and (nine[0]["inner"] > rmax).sum() >= 30, case             # VH (30 deep) neither
    assert len([s for s in _census("d100") if s["read"] == 9]) == 1                       # ... where it is an H itself: one streak all the same


def test_ties_at_the_threshold_in_every_case_that_selects():
    for case in RC.CASES:
        c = _census(case)
        if any(0 < s["m"] < s["size"] for s in c):
            assert any(s["tied"] for s in c), case
    assert {case for case in RC.CASES if any(s["tied"] for s in _census(case))} >= {"d100", "d200", "r_below", "r_equal", "r_above"}


def test_rescue_max_occ_below_at_and_above_the_depth_and_the_occ_dists():
    h, rid, pos, st, lens = RC.sketch("streaks")
    occ = RR.occurrences(h)
    deep = int(occ[occ < RC.VH_DEPTH].max())
    assert deep == RC.H_DEPTH and int(occ.max()) == RC.VH_DEPTH
    rmaxes = sorted(RR.check(*v)[1] for v in RC.CASES.values())
    assert rmaxes[0] < deep and deep in rmaxes and any(deep < r < RC.VH_DEPTH for r in rmaxes) and rmaxes[-1] == 4095
    assert (occ == RC.CASES["r_equal"][1]).any()                                           # a hash exactly at rescue_max_occ
    assert {v[0] for v in RC.CASES.values()} >= {1, 100, 200} and max(v[0] for v in RC.CASES.values()) > lens.max()
    import occ_ref as OR
    assert OR.occ_cut(OR.run_counts(h), RC.PPM, 0) == 10 != CUT                            # the other cut mode classifies differently
    assert any(0 < s["m"] < s["size"] for s in _census("d100", 10))


# ---- 2. hand cases ----------------------------------------------------------------------------------------------------------------------------
def _hand(read0, length, occ_of):
    """read 0 = [(hash, pos)]; further reads hold the copies that give every hash its occ (each alone in a read of its own)"""
    h, rid, pos = [x for x, _ in read0], [0] * len(read0), [p for _, p in read0]
    lens = [length]
    for x, n in occ_of.items():
        have = sum(1 for y, _ in read0 if y == x)
        for _ in range(n - have):
            h.append(x); rid.append(len(lens)); pos.append(20); lens.append(100)
    return np.array(h, np.uint64), np.array(rid, np.int64), np.array(pos, np.int64), np.array(lens, np.int64)


def test_the_quota_rounds_to_nearest_and_half_up():
    for span, d, m in ((299, 200, 1), (300, 200, 2), (99, 200, 0), (100, 200, 1), (500, 200, 3), (499, 200, 2), (0, 1, 0), (7, 1, 7), (1, 2, 1)):
        assert RR.streak_quota(50, 50 + span, d) == m == (2 * span + d) // (2 * d)
    # U at 100, five H, U at 400: m = 2 where rounding down gives 1
    read0 = [(1, 100)] + [(10 + i, 150 + 40 * i) for i in range(5)] + [(2, 400)]
    occ_of = {1: 2, 2: 3, 10: 9, 11: 6, 12: 8, 13: 7, 14: 9}
    h, rid, pos, lens = _hand(read0, 1000, occ_of)
    occ, flag = RR.rescue_flags(h, rid, pos, lens, 4, 200)
    assert occ[:7].tolist() == [2, 9, 6, 8, 7, 9, 3] and flag[:7].tolist() == [0, 0, 1, 0, 1, 0, 0]
    assert RR.rescue_flags(h, rid, pos, lens, 4, 200, _round_down=True)[1][:7].tolist() == [0, 0, 1, 0, 0, 0, 0]
    # the same streak at the end of a read of 410 bases: pe = the length
    h, rid, pos, lens = _hand(read0[:-1], 410, occ_of)
    assert RR.rescue_flags(h, rid, pos, lens, 4, 200)[1][:6].tolist() == [0, 0, 1, 0, 1, 0]
    # ... and in front of the first U: ps = 0, m = (800 + 200) // 400 = 2
    h, rid, pos, lens = _hand(read0[1:], 1000, occ_of)
    assert RR.rescue_flags(h, rid, pos, lens, 4, 200)[1][:6].tolist() == [0, 1, 0, 1, 0, 0]


def test_ties_go_to_the_smaller_pos_and_transparent_minimizers_are_skipped():
    read0 = [(1, 100), (10, 150), (11, 160), (20, 165), (12, 170), (21, 175), (13, 180), (2, 400)]
    occ_of = {1: 2, 2: 2, 10: 6, 11: 5, 12: 5, 13: 5, 20: 1, 21: 40}
    h, rid, pos, lens = _hand(read0, 1000, occ_of)
    occ, flag = RR.rescue_flags(h, rid, pos, lens, 4, 200, 32)                          # m = 2 of the four H: occ 5 at 160 and 170, not 180
    assert flag[:8].tolist() == [0, 0, 1, 0, 1, 0, 0, 0]
    assert RR.rescue_flags(h, rid, pos, lens, 4, 200, 32, _larger_pos=True)[1][:8].tolist() == [0, 0, 0, 0, 1, 0, 1, 0]
    assert RR.rescue_flags(h, rid, pos, lens, 4, 200, 64)[1][:8].tolist() == [0, 0, 1, 0, 1, 0, 0, 0]     # 21 is an H now: five members, the same two
    assert RR.rescue_flags(h, rid, pos, lens, 4, 100, 32)[1][:8].tolist() == [0, 0, 1, 0, 1, 0, 1, 0]     # m = 3: every occ below the threshold and two of it
    assert RR.rescue_flags(h, rid, pos, lens, 4, 50, 32)[1][:8].tolist() == [0, 1, 1, 0, 1, 0, 1, 0]      # m = 6 >= size
    assert not RR.rescue_flags(h, rid, pos, lens, 4, 0)[1].any()                                          # off
    assert not RR.rescue_flags(h, rid, pos, lens, 5, 200, 5)[1].any() and not RR.rescue_flags(h, rid, pos, lens, 6, 200, 5)[1].any()   # no H left


def test_an_anchor_needs_one_rescued_end():
    # one hash, five occurrences in five reads, cut 4: only read 1's occurrence is rescued -> the four pairs with read 1
    h = np.array([7] * 5, np.uint64)
    rid, pos, st = np.arange(5), np.full(5, 30), np.zeros(5, np.uint8)
    lens = np.full(5, 100)
    flag = np.array([0, 1, 0, 0, 0], np.uint8)
    a = RR.anchors_rescue(h, rid, pos, st, lens, 15, 4, flag)
    assert [tuple(x[:2]) for x in a] == [(0, 1), (1, 2), (1, 3), (1, 4)]
    assert len(RR.anchors_rescue(h, rid, pos, st, lens, 15, 4, flag, _both=True)) == 0
    assert len(RR.anchors_rescue(h, rid, pos, st, lens, 15, 4, flag, 4)) == 0             # rescue_max_occ at the cut: no H
    assert len(RR.anchors_rescue(h, rid, pos, st, lens, 15, 5, flag)) == 10               # the hash is used anyway
    assert np.array_equal(RR.anchors_rescue(h, rid, pos, st, lens, 15, 5, flag * 0), R.anchors(h, rid, pos, st, lens, 15, 5))


# ---- 3. sets A and B under the reference ------------------------------------------------------------------------------------------------------
def test_set_a_no_pair_without_the_rescue_and_all_of_them_with_it():
    off, s0 = RC.reference("set_a", 0, **RC.A_KW)
    on, s1 = RC.reference("set_a", *RC.A_RESCUE, **RC.A_KW)
    print({k: v for k, v in s1.items() if k in ("minimizers", "anchors", "high")}, int(s1["rescued"].sum()), len(s1["pairs"]))
    assert s0["minimizers"] == 27625 and int((s0["occ"] > 16).sum()) == 23499
    assert s0["anchors"] == 263 and len(s0["pairs"]) == 0 and len(off[1]) == 0
    assert int(s1["rescued"].sum()) == 790 and s1["anchors"] == 15622 and len(s1["pairs"]) == 780 >= 770 and len(on[1]) == 2 * 780


def test_set_b_more_pairs_with_a_repeat_only_read():
    off, s0 = RC.reference("set_b", 0, **RC.B_KW)
    on, s1 = RC.reference("set_b", *RC.B_RESCUE, **RC.B_KW)
    ro = set(RC.b_repeat_only().tolist())
    n0, n1 = (sum(1 for t, q in s["pairs"] if t in ro or q in ro) for s in (s0, s1))
    print(len(s0["pairs"]), len(s1["pairs"]), n0, n1)
    assert (len(s0["pairs"]), len(s1["pairs"]), n0, n1) == (12, 28, 0, 15) and n1 > n0
    assert set(s0["pairs"]) <= set(s1["pairs"])


def test_off_is_the_plain_reference():
    codes = RC.get("set_b")[1]
    want = R.find_overlaps(codes, **RC.B_KW)
    for got in (RR.find_overlaps_rescue(codes, 0, **RC.B_KW), RR.find_overlaps_rescue(codes, None, 64, **RC.B_KW)):
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
    assert R.anchors is RR._PLAIN_ANCHORS


# ---- 4. the setter on a context without a device ----------------------------------------------------------------------------------------------
def test_the_setter_validates_at_the_call_on_a_device_free_context():
    c = api.HostContext([100, 200])
    L = c._l
    for d, m in ((200, 0), (1, 65534), (1 << 20, 4095), (0, 0), (0, 17)):
        p = api.SeedRescueParams(occ_dist=d, rescue_max_occ=m)
        assert L.herro_set_seed_rescue(c.h, api.C.byref(p)) == 0, (d, m)
    assert L.herro_set_seed_rescue(c.h, None) == 0
    for d, m in (((1 << 20) + 1, 0), (0xFFFFFFFF, 0), (200, 65535), (0, 65535)):
        p = api.SeedRescueParams(occ_dist=d, rescue_max_occ=m)
        assert L.herro_set_seed_rescue(c.h, api.C.byref(p)) == -1, (d, m)
        assert "herro_set_seed_rescue" in c.last_error()
    p = api.SeedRescueParams(occ_dist=200)
    p.reserved[1] = 1
    assert L.herro_set_seed_rescue(c.h, api.C.byref(p)) == -1
    assert L.herro_set_seed_rescue(None, None) == -1
    c.set_seed_rescue()                                   # the defaults: 200, 4095
    c.set_seed_rescue(None)
    with pytest.raises(api.HerroError) as e:
        c.set_seed_rescue(200, 70000)
    assert e.value.code == -1
    with pytest.raises(api.HerroError):
        c.set_seed_rescue(-1)
    assert L.herro_overlaps_rescued(None) == 0 and L.herro_pairs_rescued(None) == 0
    for d in (0, 200):
        with pytest.raises(ValueError):
            RR.check(d, 65535)
    with pytest.raises(ValueError):
        RR.check((1 << 20) + 1)
    c.close()
