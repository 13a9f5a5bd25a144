"""not-gpu: the host build of herro_job_create (the reference of tests/test_gpu_build_sizes.py) on the cases of tests/build_cases.py —
8191 .. 16385 alignments, 1023 .. 3077 windows, targets of 64 .. 200 alignments, targets that contribute nothing, and the hand-made
alignments of tests/aligned_dev_cases.py at W = 16 and W = 40 — against descriptors derived from the oracle's extract_windows per
alignment (_expected of tests/test_host_job_layout.py): the parallel merge in target order with rebased offsets and job-level ratio
classes, at the sizes the device build is held to it."""
import numpy as np
import pytest

import aligned_dev_cases as AC
import build_cases as BC
from herro_amd import api
from test_host_job_layout import _expected


def _against_oracle(case, tag):
    """host job of `case` == the oracle's windows: ops, every ow and win field _expected derives, tiles, tgt_win_off; the scr_off
    tiling (disjoint, covering [0, sum op_cnt)); the fin_off / row_off / pos_off prefixes.  Returns the job's arrays."""
    sb, W, rids, rows, aln_off, cigars = case
    lens = (sb.off[1:] - sb.off[:-1]).astype(np.uint32)
    c = api.HostContext(lens)
    job = c.create_job(rids, rows, aln_off, cigars, W)
    try:
        got = c.job_arrays(job)
        seen, dropped = BC.kept(case)
        assert job.skipped() == (dropped, 0), tag
    finally:
        job.close()
        c.close()
    ops, ow, win, tiles, tgt_off = _expected(BC.batch_of(seen), W, range(len(rids)))
    assert np.array_equal(got["ops"], np.array(ops, np.uint32)), tag
    assert got["tgt_win_off"].tolist() == tgt_off, tag
    assert len(got["ow"]) == len(ow) and len(got["win"]) == len(win) == BC.n_windows(case), (tag, len(got["ow"]), len(ow))
    for k in (ow[0] if ow else ()):
        want = np.array([e[k] for e in ow], np.int64)
        assert np.array_equal(got["ow"][k].astype(np.int64), want), (tag, "ow", k, np.flatnonzero(got["ow"][k] != want)[:5])
    word_off = np.concatenate([[0], np.cumsum((lens.astype(np.uint64) + 31) // 32)]).astype(np.int64)
    qual_off = np.concatenate([[0], np.cumsum(lens.astype(np.uint64))]).astype(np.int64)
    if ow:
        qid = np.array([e["qid"] for e in ow], np.int64)
        rid = np.array([win[e["win"]]["rid"] for e in ow], np.int64)
        assert np.array_equal(got["ow"]["t_woff"].astype(np.int64), word_off[rid]), tag
        assert np.array_equal(got["ow"]["q_woff"].astype(np.int64), word_off[qid]), tag
        assert np.array_equal(got["ow"]["q_qual_off"].astype(np.int64), qual_off[qid]), tag
        order = np.argsort(got["ow"]["scr_off"], kind="stable")
        so, sn = got["ow"]["scr_off"][order].astype(np.int64), got["ow"]["op_cnt"][order].astype(np.int64)
        assert so[0] == 0 and np.array_equal(so[1:], np.cumsum(sn)[:-1]), tag
    for k in win[0]:
        want = np.array([e[k] for e in win], np.int64)
        assert np.array_equal(got["win"][k].astype(np.int64), want), (tag, "win", k, np.flatnonzero(got["win"][k] != want)[:5])
    lub = np.array([e["lub"] for e in win], np.int64)
    row = np.concatenate([[0], np.cumsum(lub)[:-1]])
    assert np.array_equal(got["win"]["row_off"].astype(np.int64), row), tag
    assert np.array_equal(got["win"]["fin_off"].astype(np.int64), 31 * row), tag
    assert np.array_equal(got["win"]["pos_off"].astype(np.int64), np.arange(len(win), dtype=np.int64) * (W + 1)), tag
    assert list(zip(got["tile_win"].tolist(), got["tile_r0"].tolist())) == tiles, tag
    return got


@pytest.mark.parametrize("name", list(BC.SIZE_CASES))
def test_host_build_equals_the_oracle_at_the_sizes_of_the_device_loops(monkeypatch, name):
    monkeypatch.setenv("HERRO_HOST_THREADS", "4")       # the parallel build and merge
    case = BC.SIZE_CASES[name]()                         # (asserts the count it is named for)
    got = _against_oracle(case, name)
    assert len(got["ow"]) > 0
    depth = np.diff(case[4].astype(np.int64))
    per_win = got["win"]["ow_cnt"]
    if name.startswith("aln_"):
        assert len(case[3]) == int(name[4:]) and depth.max() == 66 and per_win.max() > BC.WAVE
    if name.startswith("win_"):
        assert len(got["win"]) == int(name[4:])
    if name.startswith("deep_"):
        assert depth.tolist() == [int(x) for x in name.split("_")[1:]]
        # the rounds are not only walked, their alignments reach the windows: some window holds overlaps of the last round
        # (a last round of one alignment, 65 and 129, need not reach the fullest window)
        for t, d in enumerate(depth):
            w0, w1 = int(got["tgt_win_off"][t]), int(got["tgt_win_off"][t + 1])
            assert d % BC.WAVE == 1 or per_win[w0:w1].max() > BC.WAVE * ((d - 1) // BC.WAVE), (name, t, int(per_win[w0:w1].max()))
        assert depth.sum() == len(case[3])
    if name == "holes":
        BC.check_holes(got["win"])


@pytest.mark.parametrize("W", [AC.HAND_W, AC.HAND_W40])
def test_host_build_equals_the_oracle_on_the_hand_cases(W):
    names, lst, want = BC.hand_set(W)                    # (asserts the stated overlap counts against the oracle)
    assert len(names) == (19 if W == AC.HAND_W else 7)
    all_in_one = _against_oracle(BC.hand_case(W), f"hand W={W}")
    total = 0
    for i, name in enumerate(names):
        got = _against_oracle(BC.hand_case(W, i), name)
        assert name not in want or len(got["ow"]) == want[name], (name, len(got["ow"]))
        total += len(got["ow"])
    assert len(all_in_one["ow"]) == total
    with_windows = [i + 1 for i, n in enumerate(names) if want.get(n, 1)]
    assert sorted(set(all_in_one["ow"]["qid"].tolist())) == with_windows
