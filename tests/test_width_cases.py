"""not-gpu: every width case (width_cases.py) crosses the switch it exists for, by the margin stated here, with the widths read from the source; and the
same census on the named data sets of test_gpu_features.py and on capacity_cases.CASES finds none of these events — the gap the width cases close.

The census is taken from the host-built job (each slice's qlen, ops and the insertion events in front of each op) and from the oracle (L', rows per
position, informative rows, which overlaps a window keeps).  If a width changes in pileup.hip, or a case is edited so that it no longer reaches its
switch, this fails instead of test_gpu_width.py quietly running the common path.

One half of the directory word's guard cannot be reached by any input: a kept slice has no insertion above 50 bases (features.rs:315-324) behind each of at
most 8192 positions, so its query index stays below 8192 * 51 = 417 792 < 2^20 — `dQ < (1u << 20)` fails on no kept slice (largest_window_w8192 holds the
maximum), and only HERRO_DEBUG_CDIR_OVERFLOW=1 (test_gpu_e2e.py) runs the counting path for it."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import capacity_cases as K
import width_cases as Wc
from herro_amd import model_io as mio
from herro_amd import synth

_CENSUS = {}


def _census(name):
    if name not in _CENSUS:
        sb, W = Wc.build(name)
        _CENSUS[name] = (sb, W) + Wc.census(sb, W)
    return _CENSUS[name]


def _carrier(name, s):
    cs = Wc.CASES[name]
    return s["win"] == cs["win"] and 1 <= s["qid"] <= cs["carriers"]


def test_the_widths_are_where_the_cases_expect_them():
    lim = Wc.limits()
    assert lim["SCAN"] == 1 << 16 and lim["EV_LEN"] == lim["EV_LEN_RAW"] == 0xffff   # the halves of the shared scan, the event's two lengths
    assert lim["DIR_EV"] == 0xfff and lim["DIR_Q"] == 1 << 20                        # 12 + 20 bits of a directory word
    assert lim["NR_ROWS"] == 51 < 1 << 6                                             # sup_nr's 6-bit fields
    assert 8192 * lim["NR_ROWS"] < lim["DIR_Q"]                                      # a kept slice's query index always fits (module docstring)
    assert -(-8192 * lim["NR_ROWS"] // lim["ROWCAP"]) == 408 <= lim["TCAP"]          # the tiles of the largest window


@pytest.mark.parametrize("name", list(Wc.CASES))
def test_case_reaches_its_switch(name):
    cs = Wc.CASES[name]
    lim = Wc.limits()
    sb, W, slices, wins = _census(name)
    assert sb.n_targets == 1 and len(wins) == -(-cs["tl"] // W)
    car = [s for s in slices if _carrier(name, s)]
    rest = [s for s in slices if not _carrier(name, s)]
    n_ins, length = cs["ins"][1], cs["ins"][2]
    assert len(car) == cs["carriers"] and {s["strand"] for s in car} == {0, 1}
    print(name, {k: car[0][k] for k in ("qlen", "ops", "batches", "n_ev", "longest_ins", "two_scans", "unstaged", "clamped", "flagged_words", "first_flagged")},
          [{k: w[k] for k in ("lp", "irows", "nsup", "nsup_ins", "tiles", "rows_per_pos", "events")} for w in wins])
    # ---- everything but the carriers' slices of the case's window is ordinary, and kept
    for s in rest:
        assert s["kept"] and not (s["two_scans"] or s["clamped"] or s["flagged_words"] or s["long_indel"] or s["dq_beyond"]), s
    span = min(W, cs["tl"] - cs["win"] * W) + n_ins * length
    for s in car:
        assert s["qlen"] == span and s["n_ev"] == n_ins and s["longest_ins"] == length and s["ops"] >= 2 * n_ins, s
        assert not s["dq_beyond"] and s["q_total"] < lim["DIR_Q"], s
    this, others = wins[cs["win"]], [w for i, w in enumerate(wins) if i != cs["win"]]
    for w in others:
        assert w["n_alns"] == cs["carriers"] + cs["plain"] and w["irows"] == 0 and 1 <= w["nsup"] <= lim["RW_SUPCAP"], w
    if name.startswith("dropped_long_insertion"):
        for s in car:   # 66 000 + the window's bases: 464 (w64) / 4 560 (w4096) above the scan's half; the op 465 above the event's 16 bits
            assert s["two_scans"] and s["qlen"] - lim["SCAN"] == 66000 + W - 65536 and s["unstaged"], s
            assert s["clamped"] and s["longest_ins"] - lim["EV_LEN"] == 465 and s["long_indel"] and not s["kept"], s
        assert this["n_alns"] == cs["plain"] == 2 and this["lp"] == W and this["nsup"] == 0, this   # the slices are dropped, the two plain queries stay
        return
    for s in car:
        assert s["kept"] and not s["long_indel"] and not s["clamped"] and s["unstaged"], s
    assert this["n_alns"] == cs["carriers"] + cs["plain"] and this["lp"] == span and this["irows"] == n_ins * length, this
    if name == "kept_wide_slice_w2048":
        for s in car:   # 2048 + 65 000: 1 512 above the scan's half, in 14 batches of ops; the directory fits throughout
            assert s["two_scans"] and s["qlen"] - lim["SCAN"] == 1512 and s["batches"] == 14 and s["flagged_words"] == 0 and s["fitting_words"] == W // 32, s
        assert this["rows_per_pos"] == lim["NR_ROWS"] and this["irows"] > lim["CP_ICAP"] and this["events"] > lim["QEVCAP"], this
        assert 1 <= this["nsup"] <= lim["RW_SUPCAP"] and 1 <= this["nsup_ins"] < this["nsup"], this
    elif name == "directory_events_w8192":
        for s in car:   # one scan (12 392 bases); 4 200 events: 105 above the directory's 12 bits, reached at word 128 (32 events per word) of 256
            assert not s["two_scans"] and s["ev_before_max"] - lim["DIR_EV"] == 105, s
            assert (s["fitting_words"], s["flagged_words"], s["first_flagged"]) == (128, 128, 128), s
        assert 1 <= this["nsup"] <= lim["RW_SUPCAP"] and 1 <= this["nsup_ins"] < this["nsup"], this
        assert this["irows"] > lim["CP_ICAP"] and this["lp"] > lim["CP_OCAP"], this
    else:
        assert name == "largest_window_w8192"
        for s in car:   # 8192 * 51 bases, the most a kept slice can span; 8192 events
            assert s["two_scans"] and s["qlen"] == 8192 * lim["NR_ROWS"] == 417792 and s["batches"] == 86, s
            assert s["ev_before_max"] == 8191 and (s["fitting_words"], s["flagged_words"], s["first_flagged"]) == (128, 128, 128), s
        assert this["lp"] == 417792 and this["rows_per_pos"] == lim["NR_ROWS"] and this["tiles"] == 408 <= lim["TCAP"], this
        assert this["irows"] > max(lim["RW_ICAP"], lim["CP_ICAP"]) and this["lp"] > lim["CP_OCAP"] and this["events"] > lim["QEVCAP"], this
        assert lim["RW_SUPCAP"] < this["nsup"] < 2 * lim["RW_SUPCAP"] and this["nsup_ins"] == 0, this   # (two carriers: no insertion row can be informative)


def _old_sets():
    import test_gpu_features as F
    for name, cs in F.CASES.items():
        yield "features:" + name, cs["W"], (lambda cs=cs, name=name: synth.generate(cs["n"], cs["tl"], cs["ov"], seed=synth.SEED + sum(map(ord, name)), **cs["kw"]))
    for name, cs in K.CASES.items():
        yield "capacity:" + name, cs["W"], (lambda name=name: K.generate(name))


@pytest.mark.parametrize("which", [n for n, _, _ in _old_sets()])
def test_the_old_data_sets_reach_none_of_these(which):
    """The named data sets of test_gpu_features.py and the capacity cases: no slice with a query span of 2^16, no insertion of 2^16 bases, no 4 095 insertion
    events in one slice (so no flagged directory word), no position of 51 rows, nowhere near 408 tiles."""
    lim = Wc.limits()
    W, gen = next((W, g) for n, W, g in _old_sets() if n == which)
    sb = gen()
    slices, wins = Wc.census(sb, W, lim)
    if which != "features:no_overlaps":
        assert slices
    seen = dict(qlen=max([s["qlen"] for s in slices] + [0]), ins=max([s["longest_ins"] for s in slices] + [0]), n_ev=max([s["n_ev"] for s in slices] + [0]),
                rows_per_pos=max(w["rows_per_pos"] for w in wins), tiles=max(w["tiles"] for w in wins))
    print(which, seen)
    assert not any(s["two_scans"] or s["clamped"] or s["flagged_words"] or s["dq_beyond"] for s in slices)
    assert seen["qlen"] < lim["SCAN"] // 4 and seen["ins"] < lim["EV_LEN"] // 64 and seen["n_ev"] < lim["DIR_EV"] // 2
    assert seen["rows_per_pos"] < lim["NR_ROWS"] and seen["tiles"] < 408 // 8


def test_compact_twin_inputs_compute_the_uncut_batch():
    """width_cases.compact_twin_inputs (what test_gpu_width.py feeds the fp32 twin for a window of 417 792 rows) against the dense module on the whole batch:
    rows at both ends of a window, next to the collate padding, at the end of the longest window, in clusters and alone."""
    import model_ref as MR
    hp = mio.Hyper()
    raw = mio.random_raw_params(hp, seed=11)
    twin = MR.build(raw, hp)
    rng = np.random.default_rng(8)
    L = 160
    win_len = [160, 70, 131, 160]
    rows = [np.array([0, 1, 7, 8, 9, 60, 100, 158, 159]), np.array([2, 40, 68, 69]), np.array([66, 130]), np.array([159])]
    bases = np.full((4, L, 31), 11, np.uint8)
    quals = np.full((4, L, 31), 126, np.uint8)
    wins = []
    for k, n in enumerate(win_len):
        bases[k, :n] = rng.integers(0, 11, (n, 31))
        quals[k, :n] = rng.integers(33, 90, (n, 31))
        wins.append((bases[k, :n].copy(), quals[k, :n].copy(), rows[k]))
    lens = np.array([len(r) for r in rows], np.int32)
    ti, tb = MR.run_batch(twin, bases, quals, lens, np.concatenate(rows).astype(np.int32))
    cb, cq, cl, cidx, cpos = Wc.compact_twin_inputs(wins, 2 * (hp.kw // 2))
    assert cb.shape[1] < L // 2 and cl.tolist() == lens.tolist() and cpos.tolist() == np.concatenate(rows).tolist()
    gi, gb = MR.run_batch(twin, cb, cq, cl, cidx, gemm=True, positions_flat=cpos)
    assert ti.shape == gi.shape and tb.shape == gb.shape
    assert np.abs(ti - gi).max() < 2e-5 and np.abs(tb - gb).max() < 2e-5, (np.abs(ti - gi).max(), np.abs(tb - gb).max())
