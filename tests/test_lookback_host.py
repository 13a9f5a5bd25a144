"""not-gpu: the longer chain look-back ("A longer look-back") where no device is needed — the scores of tests/lookback_cases.py
from tests/overlap_ref.py::chain, the mutant that lets a farther round win a tie, chain_many against chain beyond 64, and every refusal of
herro_set_chain_params and of herro_debug_chain's argument checks on a device-free context."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import lookback_cases as L  # noqa: E402
import overlap_ref as R  # noqa: E402
from herro_amd import api  # noqa: E402

TABLE = [(name, H) for name, (_, _, scores) in L.SETS.items() for H in scores if name != "T4" or H in L.T4_USED]


def test_the_generator_reproduces_the_tandem_pair_of_the_finder_tests():
    rng = np.random.default_rng(5)                       # tests/test_gpu_overlap.py::_tandem_pair, restated
    u = rng.integers(0, 4, 40)
    g = np.concatenate([rng.integers(0, 4, 2400), np.tile(u, 30), rng.integers(0, 4, 2400)])
    want = []
    for _ in range(2):
        r = g.copy()
        m = rng.random(len(r)) < 0.01
        r[m] = (r[m] + rng.integers(1, 4, m.sum())) & 3
        want.append(bytes(b"ACGT"[x] for x in r))
    assert list(L.reads("T1")) == want
    for name, (_, n_anchors, _) in L.SETS.items():
        tp, qp = L.group(name)
        assert len(tp) == n_anchors, name
        key = (tp << 32) | qp
        assert (np.diff(key) > 0).all() and tp.max() < 1 << 31 and qp.max() < 1 << 31


@pytest.mark.parametrize("name,H", TABLE, ids=[f"{n}-{h}" for n, h in TABLE])
def test_the_scores_of_the_table_are_the_references(name, H):
    assert L.ref_group(name, H)[0] == L.SETS[name][2][H]


def test_the_table_separates_every_adjacent_pair_of_lookbacks():
    for a, b in zip(L.LOOKBACKS, L.LOOKBACKS[1:]):
        assert any(a in s and b in s and s[a] != s[b] for _, _, s in L.SETS.values()), (a, b)
    t1 = L.SETS["T1"][2]
    assert t1[512] == t1[1024] == R.chain(*L.group("T1"), L.KW["k"], L.KW["bandwidth"], L.KW["max_gap"], None)[0]     # the unlimited look-back's


@pytest.mark.parametrize("H", (128, 256, 1024))
def test_a_farther_round_must_not_win_a_tie(H):
    """the mutant differs from the reference on every slice of 127 anchors or more (at 128 under the early-stop gap too): a kernel with its bug
    cannot pass"""
    for gap in (L.KW["max_gap"], L.EARLY_STOP_GAP)[:2 if H == 128 else 1]:
        ref = L.ref_slices(H, gap)
        for n, (tp, qp), want in zip(L.SLICE_LENGTHS, L.slices(), ref):
            got = L.chain_far_round_wins_ties(tp, qp, L.KW["k"], L.KW["bandwidth"], gap, H)
            assert (got != want) == (n >= 127), (H, gap, n, got, want)


def test_the_early_stop_set_skips_whole_rounds():
    """Round r >= 1 of an anchor lies beyond the gap as a whole where its nearest predecessor, i - 64 r - 1, already does.  At max_gap = 120 that
    holds for a share of the anchors of the longest slice in the far rounds of a look-back of 1024; at 30 the stop falls behind each of the
    rounds 0 .. 5 for some anchors and not for others, and no anchor reaches round 6; at 5000 no round is ever skipped."""
    tp, _ = L.slices()[-1]

    def beyond(r, gap):
        d = 64 * r + 1
        return tp[d:] - tp[:-d] > gap
    assert beyond(15, L.EARLY_STOP_GAP).mean() > 0.25 and beyond(8, L.EARLY_STOP_GAP).any() and not beyond(1, L.EARLY_STOP_GAP).any()
    for r in range(1, 6):
        assert beyond(r, L.NEAR_STOP_GAP).any() and not beyond(r, L.NEAR_STOP_GAP).all(), r
    assert beyond(6, L.NEAR_STOP_GAP).all()
    assert not beyond(15, L.KW["max_gap"]).any()


@pytest.mark.parametrize("H", (128, 1024))
def test_chain_many_equals_chain(H):
    for gap in L.GAPS:
        tps, qps = [s[0] for s in L.slices()], [s[1] for s in L.slices()]
        assert R.chain_many(tps, qps, L.KW["k"], L.KW["bandwidth"], gap, H) == list(L.ref_slices(H, gap)), (H, gap)


# ---- the setting and the hook's argument checks on a context without a device ------------------------------------------------------------------
def _set(c, lookback, reserved=(0, 0, 0)):
    p = api.ChainParams(lookback=lookback, reserved=(C.c_uint32 * 3)(*reserved))
    return c._l.herro_set_chain_params(c.h, C.byref(p))


def _no_device(c, groups, **kw):
    """the hook passed its argument checks: a device-free context is HERRO_E_NO_DEVICE"""
    with pytest.raises(api.HerroError) as e:
        c.chain(groups, **kw)
    assert e.value.code == -2, str(e.value)


def test_the_setter_validates_on_a_device_free_context():
    c = api.HostContext([100, 200])
    assert c.chain_lookback == 64
    for H in (0,) + L.LOOKBACKS + tuple(range(64, 1025, 64)):
        assert _set(c, H) == 0, H
    assert c._l.herro_set_chain_params(c.h, None) == 0
    c.set_chain_lookback(256)
    for bad in (63, 65, 1088, 1 << 31, 1, 100, 2048, 0xFFFFFFFF):
        assert _set(c, bad) == -1, bad
        msg = c._l.herro_last_error(c.h).decode()
        assert "herro_set_chain_params" in msg and "multiple of 64" in msg and "64 .. 1024" in msg, msg
        with pytest.raises(api.HerroError) as e:
            c.set_chain_lookback(bad)
        assert e.value.code == -1 and c.chain_lookback == 256
    for res in ((1, 0, 0), (0, 1, 0), (0, 0, 7)):
        assert _set(c, 128, res) == -1, res
        assert "reserved" in c._l.herro_last_error(c.h).decode()
    with pytest.raises(api.HerroError):
        c.set_chain_lookback(-64)
    assert c.chain_lookback == 256
    c.set_chain_lookback(None)
    assert c.chain_lookback == 64


def test_a_refused_value_leaves_the_previous_setting_in_force():
    """the library's own state, not the binding's: the hook refuses a look-back keyword through the setter and still holds the old one — a
    non-multiple given for one call raises before the call and the context's 192 is put back"""
    c = api.HostContext([100])
    ok = [(np.arange(10, 80, 7), np.arange(5, 75, 7))]
    c.set_chain_lookback(192)
    assert _set(c, 200) == -1 and _set(c, 128, (0, 0, 1)) == -1
    with pytest.raises(api.HerroError) as e:
        c.chain(ok, lookback=100)
    assert e.value.code == -1 and c.chain_lookback == 192
    _no_device(c, ok, lookback=512)
    assert c.chain_lookback == 192
    assert _set(c, 0) == 0


def test_the_hook_checks_its_groups_before_it_asks_for_a_device():
    c = api.HostContext([100])
    t, q = np.arange(10, 2000, 3), np.arange(7, 1997, 3)
    good = (t, q)
    _no_device(c, [good])
    _no_device(c, [good, (t[:1], q[:1])], k=15, bandwidth=150, max_gap=120)
    _no_device(c, [])
    swapped_t, dup, q_back = t.copy(), t.copy(), q.copy()
    swapped_t[[100, 101]] = swapped_t[[101, 100]]
    q_back[5] = q_back[4]
    dup[7], q_dup = dup[6], q.copy()
    q_dup[7] = q_dup[6]
    big_t, big_q = t.astype(np.uint32), q.astype(np.uint32)
    big_t[-1], big_q[-1] = 1 << 31, 0xFFFFFFFF
    cases = [((swapped_t, q), "not strictly ascending"), ((dup, q_dup), "not strictly ascending"), ((t[:0], q[:0]), "empty"),
             ((big_t, q), "2^31"), ((t, big_q), "2^31")]
    for at in (0, 2):
        for bad, word in cases:
            groups = [good] * at + [bad, good]
            with pytest.raises(api.HerroError) as e:
                c.chain(groups)
            assert e.value.code == -1 and f"group {at} " in str(e.value) and word in str(e.value), (at, word, str(e.value))
    _no_device(c, [(t, q_back)])                       # equal qpos under ascending tpos: a valid group
    two_bad = [good, (swapped_t, q), (t[:0], q[:0])]   # the first offending group is the one named
    with pytest.raises(api.HerroError) as e:
        c.chain(two_bad)
    assert "group 1 " in str(e.value)
    for bad_param in (dict(k=4), dict(k=32)):
        with pytest.raises(api.HerroError) as e:
            c.chain([good], **bad_param)
        assert e.value.code == -1
    out = np.zeros(4, np.int32)
    off = np.array([0, 3], np.uint64)
    tt = np.array([1, 2, 3], np.uint32)
    Lb = c._l
    assert Lb.herro_debug_chain(c.h, 1, None, tt.ctypes.data, tt.ctypes.data, None, out.ctypes.data) == -1
    assert Lb.herro_debug_chain(c.h, 1, off.ctypes.data, None, tt.ctypes.data, None, out.ctypes.data) == -1
    assert Lb.herro_debug_chain(c.h, 1, off.ctypes.data, tt.ctypes.data, tt.ctypes.data, None, None) == -1
    off1 = np.array([1, 3], np.uint64)
    assert Lb.herro_debug_chain(c.h, 1, off1.ctypes.data, tt.ctypes.data, tt.ctypes.data, None, out.ctypes.data) == -1
    assert Lb.herro_debug_chain(c.h, 1, off.ctypes.data, tt.ctypes.data, tt.ctypes.data, None, out.ctypes.data) == -2


def test_the_binding_and_the_abi_list_agree():
    assert {"herro_set_chain_params", "herro_debug_chain"} <= set(api.EXPORTS)
    assert C.sizeof(api.ChainParams) == 16
