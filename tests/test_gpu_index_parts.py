"""gpu: the overlap finder with its index built in parts (herro_set_index_params; csrc/overlap_dev.hip: k_sketch_part, k_occ16, k_occ_pick,
k_part_cls, k_part_gather, k_part_runs, k_part_expand, k_rec_keys, k_rec_gather; DESIGN.md §10, "An index in parts") against the UNPARTITIONED
references, record for record: the combination trials of tests/test_index_parts_host.py with every option, a block per read and a single block, the
hash ranges of the occurrence pass, the low-complexity working set, the scratch budget, the memory figure, and the setting switched off again."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import combo_cases as CB  # noqa: E402
import gpu_common as G  # noqa: E402
import index_parts_ref as IP  # noqa: E402
import occ_ref as OR  # noqa: E402
import overlap_ref as R  # noqa: E402
import pair_cases as PC  # noqa: E402
import rescue_ref as RR  # noqa: E402
import test_index_parts_host as H  # noqa: E402
import test_lowcomplexity_host as LH  # noqa: E402
from herro_amd import api  # noqa: E402
from test_gpu_combo import _load, _plain, _same_rows, _stderr_of  # noqa: E402

pytestmark = pytest.mark.gpu

PARTS = 7


def _ctx():
    c = G.ctx()
    _plain(c)
    c.set_index_parts(None)
    return c


def _off(c):
    _plain(c)
    c.set_index_parts(None)
    assert getattr(c, "_index_parts", (0, 0)) == (0, 0)


def _both_calls(c, t, fkw, ext, m, tag, blocks=None):
    """find_overlaps and find_overlap_pairs of a trial under fkw (index_kmers among them) against the composed reference; the pairs' bytes"""
    st = CB.reference(t)[1]
    cut, rescued = st["cut"], int(st["rescued"].sum())
    got = c.find_overlaps(core=m, **fkw)
    assert (c.last_occ_cut, c.last_rescued) == (cut, rescued), tag
    if blocks is not None:
        assert c.last_index_blocks == blocks, (tag, c.last_index_blocks)
    assert CB.same_rows(got, CB.expected_rows(t)), tag
    _same_rows(got, CB.expected_rows(t), tag)
    p = c.find_overlap_pairs(core=m, **ext, **fkw)
    try:
        assert (p.occ_cut, p.rescued) == (cut, rescued), tag
        if blocks is not None:
            assert p.index_blocks == blocks, (tag, p.index_blocks)
        assert CB.same_pairs(PC.pairs_fields(p), CB.expected_pairs(t)), tag
        PC.assert_same_fields(PC.pairs_fields(p), CB.expected_pairs(t), tag)
        return [x.tobytes() for x in got], PC.pairs_bytes(p)
    finally:
        p.close()


# ---- 1. equality over the options ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("part", range(PARTS))
def test_every_option_in_parts_equals_the_unpartitioned_reference(part):
    c = _ctx()
    try:
        for number in H.TRIALS[part::PARTS]:
            t = CB.trial(number)
            codes, fkw, ext, m = _load(c, t)
            lens = [len(x) for x in codes]
            blocks = len(IP.block_cuts(lens, t["fkw"]["k"], t["fkw"]["w"], H.quarter(t))) - 1
            assert blocks >= 2 and blocks == H.BLOCKS[t["set"]] == len(api.index_plan(lens, t["fkw"]["k"], t["fkw"]["w"], H.quarter(t))) - 1
            _both_calls(c, t, dict(fkw, index_kmers=H.quarter(t)), ext, m, CB.tag(t), blocks)
            assert c._index_parts == (0, 0)                                        # the keyword left the context's setting alone
    finally:
        _off(c)


# ---- 2. a block per read, and a single block ------------------------------------------------------------------------------------------------------
def test_a_block_per_read_and_a_single_block_on_set_d(monkeypatch):
    t = CB.trial(38)                                                               # D, k = 15: rescue, look-back 256
    assert t["set"] == "D" and t["rescue"] is not None
    c = _ctx()
    monkeypatch.setenv("HERRO_OVL_STATS", "1")
    try:
        codes, fkw, ext, m = _load(c, t)
        _, err = _stderr_of(lambda: _both_calls(c, t, dict(fkw, index_kmers=1), ext, m, "a block per read", 10))
        lines = re.findall(r"^OVLPART blocks=(\d+) pairs=(\d+) ranges=(\d+) peak_bytes=(\d+)$", err, re.M)
        assert len(lines) == 2 and all(ln[:2] == ("10", "55") for ln in lines), err[-800:]
        _, err = _stderr_of(lambda: _both_calls(c, t, dict(fkw, index_kmers=10**9), ext, m, "one block", 1))
        lines = re.findall(r"^OVLPART blocks=(\d+) pairs=(\d+) ranges=(\d+) peak_bytes=(\d+)$", err, re.M)
        assert len(lines) == 2 and all(ln[:3] == ("1", "1", "1") for ln in lines), err[-800:]
    finally:
        _off(c)


# ---- 3. the hash ranges of the occurrence pass ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("number", [10, 23])
def test_the_hash_ranges_give_the_same_bytes_occurrences_and_census(number):
    t = CB.trial(number)
    assert t["set"] in ("streaks", "G7") and t["rescue"] is not None and t["ppm"]
    c = _ctx()
    try:
        codes, fkw, ext, m = _load(c, t)
        k, w = t["fkw"]["k"], t["fkw"]["w"]
        lens = np.array([len(x) for x in codes], np.int64)
        h, rid, pos, _ = R.sketch_store(codes, k, w)
        cut = CB.reference(t)[1]["cut"]
        want_occ = np.minimum(RR.occurrences(h), 65535)
        want_flag = RR.rescue_flags(h, rid, pos, lens, cut, *t["rescue"])[1]
        want_hist, want_fig = OR.census(codes, t["ppm"], k=k, w=w, max_occ=t["fkw"]["max_occ"])
        seen = set()
        for ranges in (1, 3, 16):
            kw = dict(fkw, index_kmers=H.quarter(t), occ_ranges=ranges)
            rows_bytes, pairs_bytes = _both_calls(c, t, kw, ext, m, (CB.tag(t), ranges))
            seen.add((tuple(rows_bytes), pairs_bytes))
            occ, flag = c.seed_rescue(k=k, w=w, max_occ=t["fkw"]["max_occ"], occ_frac_ppm=t["ppm"], index_kmers=H.quarter(t), occ_ranges=ranges)
            assert np.array_equal(occ, want_occ) and np.array_equal(flag, want_flag), (CB.tag(t), ranges)
            hist, fig = c.occ_census(k=k, w=w, max_occ=t["fkw"]["max_occ"], occ_frac_ppm=t["ppm"], index_kmers=H.quarter(t), occ_ranges=ranges)
            assert np.array_equal(hist, want_hist) and fig == want_fig, (CB.tag(t), ranges, fig, want_fig)
        assert len(seen) == 1
    finally:
        _off(c)


# ---- 4. low complexity ------------------------------------------------------------------------------------------------------------------------------
def test_the_low_complexity_working_set_in_four_blocks():
    """palindromic k-mers, hashes repeated inside a read, runs with a read more than once"""
    kw = dict(k=16, w=8, max_occ=32, min_score=60)
    assert kw == LH.PARAM_SETS[2]
    ws, codes = LH.low()
    c = _ctx()
    try:
        c.set_reads(ws.seq, ws.qual, ws.off)
        lens = [len(x) for x in codes]
        total = int(IP.read_kmers(lens, 16, 8).sum())
        max_kmers = 2 * -(-total // 3)                                             # (a third per block: the fourth block takes what the reads' sizes leave over)
        assert len(IP.block_cuts(lens, 16, 8, max_kmers)) - 1 == 4
        want = R.find_overlaps(codes, **kw)
        got = c.find_overlaps(index_kmers=max_kmers, **kw)
        assert c.last_index_blocks == 4
        _same_rows(got, want, "low complexity")
        assert (got[1][:, 4] == 0).any() and (got[1][:, 4] == 1).any() and len(got[1]) > 50
    finally:
        _off(c)


# ---- 5, 6. the scratch budget, determinism, the memory figure: fresh child processes ---------------------------------------------------------------
_CHILD = r"""
import hashlib, json, os, sys
sys.path.insert(0, os.path.join(sys.argv[1], "tests")); sys.path.insert(0, sys.argv[1])
from herro_amd import api
import combo_cases as CB
import pair_cases as PC
t = CB.trial(int(sys.argv[2]))
seq, qual, off, codes = CB.reads(t["set"])
c = api.Context(0)
c.set_reads(seq, qual, off)
c.set_seed_rescue(*(t["rescue"] or (None,)))
fkw = dict(t["fkw"], lookback=t["lookback"], index_kmers=int(sys.argv[3]), **(dict(occ_frac_ppm=t["ppm"]) if t["ppm"] else {}))
out = []
for _ in range(int(sys.argv[4])):
    rows = c.find_overlaps(**fkw)
    p = c.find_overlap_pairs(extend=False, **fkw)
    out.append(hashlib.sha256(b"|".join(x.tobytes() for x in rows) + PC.pairs_bytes(p)).hexdigest())
    p.close()
print(json.dumps(out))
"""


def _child(number, index_kmers, calls, budget):
    env = dict(os.environ, HERRO_OVL_STATS="1")
    env.pop("HERRO_OVL_SCRATCH_MB", None)
    if budget is not None:
        env["HERRO_OVL_SCRATCH_MB"] = str(budget)
    p = subprocess.run([sys.executable, "-c", _CHILD, G.ROOT, str(number), str(index_kmers), str(calls)], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    parts = [tuple(int(x) for x in ln) for ln in re.findall(r"^OVLPART blocks=(\d+) pairs=(\d+) ranges=(\d+) peak_bytes=(\d+)$", p.stderr, re.M)]
    chunks = [int(x) for x in re.findall(r"^OVL .* chunks=(\d+)$", p.stderr, re.M)]
    assert len(parts) == 2 * calls and len(chunks) == 2 * calls, p.stderr[-800:]
    return json.loads(p.stdout.strip().splitlines()[-1]), parts, chunks


def test_a_budget_of_1_mib_gives_the_same_bytes_and_so_does_a_second_call():
    t = CB.trial(1)                                                                # G40: rescue, fraction cut, look-back 256
    assert t["rescue"] is not None and t["ppm"] and t["lookback"] == 256
    small, parts, chunks = _child(1, H.quarter(t), 2, 1)
    assert small[0] == small[1] and parts[0][0] == H.BLOCKS["G40"]
    plain, _, chunks_plain = _child(1, H.quarter(t), 1, None)
    assert plain[0] == small[0]
    print(dict(chunks_at_1_mib=chunks, chunks_at_the_default=chunks_plain))
    assert chunks[0] >= chunks_plain[0]


def test_smaller_parts_hold_less_scratch_at_once():
    t = CB.trial(36)                                                               # set_a: 40 reads of one genome
    assert t["set"] == "set_a"
    total = H.total_kmers(t)
    eighth, p8, _ = _child(36, 2 * -(-total // 8), 1, 1)
    whole, p1, _ = _child(36, 2 * total, 1, 1)
    print(dict(eighths=p8, one_block=p1))
    assert eighth == whole and p1[0][0] == 1 and p8[0][0] > 4
    assert p8[0][3] < p1[0][3] and p8[1][3] < p1[1][3]                              # peak_bytes of both calls


# ---- 7. off is off ----------------------------------------------------------------------------------------------------------------------------------
def test_the_setting_switched_off_runs_what_ran_before(monkeypatch):
    t = CB.trial(23)
    c = _ctx()
    monkeypatch.setenv("HERRO_OVL_STATS", "1")
    try:
        codes, fkw, ext, m = _load(c, t)
        before, err0 = _stderr_of(lambda: _both_calls(c, t, fkw, ext, m, "before"))
        assert "OVLPART" not in err0 and c.last_index_blocks == 0
        c.set_index_parts(H.quarter(t), 3)
        on, err1 = _stderr_of(lambda: _both_calls(c, t, fkw, ext, m, "on", H.BLOCKS["G7"]))      # the context's setting, no keyword
        assert len(re.findall(r"^OVLPART blocks=6 pairs=\d+ ranges=3 ", err1, re.M)) == 2, err1[-800:]
        c.set_index_parts(None)
        after, err2 = _stderr_of(lambda: _both_calls(c, t, fkw, ext, m, "after", 0))
        assert "OVLPART" not in err2 and before == on == after
        # the figures of the other lines are the sums over the parts
        ovl = lambda e: [re.sub(r" chunks=\d+", "", ln) for ln in e.splitlines() if ln.startswith(("OVL ", "OVLOCC", "OVLRESC", "OVLCHAIN"))]      # noqa: E731
        assert ovl(err0) == ovl(err1) == ovl(err2) and len(ovl(err0)) == 8, (ovl(err0), ovl(err1))
    finally:
        _off(c)


# ---- 8. errors ----------------------------------------------------------------------------------------------------------------------------------------
def test_the_codes_of_the_setting_on_a_device_context():
    c = _ctx()
    try:
        c.set_index_parts(1000, 3)
        for bad in ((H.OVL_MAX_KMERS + 1, 0), (1000, 65537)):
            with pytest.raises(api.HerroError) as e:
                c.set_index_parts(*bad)
            assert e.value.code == -1 and "herro_set_index_params" in str(e.value) and c._index_parts == (1000, 3)
        t = CB.trial(4)
        codes, fkw, ext, m = _load(c, t)
        with pytest.raises(api.HerroError) as e:
            c.find_overlaps(occ_ranges=65537, **fkw)
        assert e.value.code == -1 and c._index_parts == (1000, 3)
        got = c.find_overlaps(core=m, **fkw)                                       # the setting still holds: two blocks of one read each
        assert c.last_index_blocks == 2
        _same_rows(got, CB.expected_rows(t), CB.tag(t))
    finally:
        _off(c)
