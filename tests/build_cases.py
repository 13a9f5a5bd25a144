"""Inputs for the device job build (csrc/build_dev.hip, csrc/cigar_dev.hip) past the sizes at which its loops run once, shared by
tests/test_build_cases.py (host build against the oracle, no device) and tests/test_gpu_build_sizes.py (device build against the host
build).  Every case is (sb, W, rids, rows, aln_off, cigars): the reads to load, the window size and the arguments of create_job.  Each
helper asserts the count it is named for, so a change of the generator cannot move a case below the threshold it is there to cross:

  k_scan_alns   8192 alignments per pass (E = 8 records x 1024 threads), a running total into the next   -> aln_case
  k_scan_wins   ceil(n_win / 1024) consecutive windows per thread                                           -> win_case
  k_win_pass    a target's alignments 64 lanes at a time; four windows per workgroup                        -> deep_cases, hole_case
  k_window_cuts extract_windows restated from cut records (sorted by the thread: they arrive unordered)    -> win_case(2049), hand_set
"""
import dataclasses
import functools

import numpy as np

import aligned_dev_cases as AC
import oracle_lib as O
from herro_amd import synth

ALN_COUNTS = (8191, 8192, 8193, 16384, 16385)
WIN_CASES = {1023: (496, 33, 31), 1024: (1024, 16, 64), 1025: (656, 25, 41), 2049: (10928, 3, 683), 3077: (2896, 17, 181)}   # n_win: tl, nt, windows per target
SCAN_ALNS_PASS = 8192
SCAN_WINS_THREADS = 1024
WAVE = 64


def _cigars(sb, lo, hi):
    return [sb.cigar(a) for a in range(lo, hi)]


def batch_of(case):
    """The case as a SynthBatch whose targets and alignments are the job's (for api.job_from_synth and for _expected of
    tests/test_host_job_layout.py, which reads tgt_rid, tgt_aln_off, aln and cigar())."""
    sb, _, rids, rows, aln_off, cigars = case
    aln = np.zeros((len(rows), 10), np.uint32)
    aln[:, :9] = rows[:, :9]
    aln[:, 9] = [len(c) for c in cigars]
    cig_off = np.zeros(len(rows), np.uint64)
    if len(rows):
        cig_off[1:] = np.cumsum(aln[:-1, 9].astype(np.uint64))
    cig = np.frombuffer(b"".join(cigars) + b"\0", np.uint8).copy()
    return dataclasses.replace(sb, aln=aln, cig_off=cig_off, cig=cig, tgt_aln_off=np.asarray(aln_off, np.uint64), tgt_rid=np.asarray(rids, np.uint32))


def kept(case):
    """The case without the alignments parse_paf drops (overlaps.rs:175-185: self overlaps, a second alignment of a (query, target)
    pair) and the number dropped: what the oracle's extract_windows would have been given."""
    sb, W, rids, rows, aln_off, cigars = case
    keep, off = [], [0]
    for t in range(len(rids)):
        seen = set()
        for a in range(int(aln_off[t]), int(aln_off[t + 1])):
            q = int(rows[a, 0])
            if q != int(rids[t]) and q not in seen:
                seen.add(q)
                keep.append(a)
        off.append(len(keep))
    return (sb, W, rids, rows[keep], np.array(off, np.uint64), [cigars[a] for a in keep]), len(rows) - len(keep)


def n_windows(case):
    sb, W, rids = case[:3]
    lens = (sb.off[1:] - sb.off[:-1]).astype(np.int64)
    return int(((lens[np.asarray(rids, np.int64)] + W - 1) // W).sum())


# ---- alignment counts around one and two passes of k_scan_alns ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _aln_batch():
    sb = synth.generate(250, 320, 66, seed=7, flank_min=10, flank_max=40, p_partial=0.3, min_partial_len=80)
    assert (np.diff(sb.tgt_aln_off.astype(np.int64)) == 66).all()       # every window of every target: two rounds of k_win_pass
    return sb


@functools.lru_cache(maxsize=None)
def aln_case(n):
    sb, W = _aln_batch(), 64
    nt = int(np.searchsorted(sb.tgt_aln_off, n, "left"))
    aln_off = np.minimum(sb.tgt_aln_off[:nt + 1], n).astype(np.uint64)
    case = (sb, W, sb.tgt_rid[:nt].copy(), sb.aln[:n].copy(), aln_off, _cigars(sb, 0, n))
    assert len(case[3]) == n == int(aln_off[-1]) and (np.diff(aln_off.astype(np.int64)) > 0).all()
    assert (n - 1) // SCAN_ALNS_PASS == {8191: 0, 8192: 0, 8193: 1, 16384: 1, 16385: 2}[n]      # index of the last pass
    return case


# ---- window counts around 1, 2 and 3 windows per thread of k_scan_wins ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def win_case(n_win):
    tl, nt, per_target = WIN_CASES[n_win]
    W = 16
    sb = synth.generate(nt, tl, 5, seed=tl, flank_min=10, flank_max=40, p_partial=0.3)
    case = (sb, W, sb.tgt_rid.copy(), sb.aln.copy(), sb.tgt_aln_off.astype(np.uint64), _cigars(sb, 0, len(sb.aln)))
    assert -(-tl // W) == per_target and n_windows(case) == n_win == nt * per_target
    per = -(-n_win // SCAN_WINS_THREADS)
    assert per == {1023: 1, 1024: 1, 1025: 2, 2049: 3, 3077: 4}[n_win]
    busy = -(-n_win // per)                                              # threads with a window: the rest have an empty range
    assert (busy == SCAN_WINS_THREADS) == (n_win == 1024) and (n_win % per != 0) == (n_win in (1025, 3077))   # a short last range
    if n_win == 2049:   # several hundred cuts per alignment, in whatever order the scan's lanes found them: the sort of k_window_cuts
        span = (sb.aln[:, 8].astype(np.int64) - sb.aln[:, 7]) // W
        assert span.max() > 64 and span.max() > 300
    return case


# ---- targets of 64, 65, 128, 129 and 200 alignments: rounds of k_win_pass -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _deep_batch():
    sb = synth.generate(3, 600, 200, seed=9, flank_min=10, flank_max=40, p_partial=0.2)
    assert (np.diff(sb.tgt_aln_off.astype(np.int64)) == 200).all()
    return sb


def _truncated(sb, W, depths):
    sel = np.concatenate([np.arange(int(sb.tgt_aln_off[t]), int(sb.tgt_aln_off[t]) + d) for t, d in enumerate(depths)])
    aln_off = np.concatenate([[0], np.cumsum(depths)]).astype(np.uint64)
    case = (sb, W, sb.tgt_rid[:len(depths)].copy(), sb.aln[sel].copy(), aln_off, [sb.cigar(int(a)) for a in sel])
    assert np.diff(aln_off.astype(np.int64)).tolist() == list(depths)
    return case


@functools.lru_cache(maxsize=None)
def deep_case(name):
    depths = {"deep_128_129_200": (128, 129, 200), "deep_64_65": (64, 65)}[name]
    assert sorted({-(-d // WAVE) for d in depths}) == ([2, 3, 4] if len(depths) == 3 else [1, 2])
    return _truncated(_deep_batch(), 64, depths)


# ---- targets without alignments, without windowed alignments, without kept alignments -----------------------------------------------------
@functools.lru_cache(maxsize=None)
def hole_case():
    """Nine targets of 300 bp at W = 64 (five windows each): E N E S N K N N E.  E has no alignment (aln_off[t] == aln_off[t + 1]), N
    keeps its generated ones (the second N with the query of its first alignment once more, in third place), S has four alignments
    that are all too short to be windowed (target span, or query span, below W), K has two that parse_paf leaves out: self overlaps,
    the second of them a repeated pair as well.  (A repeated pair alone cannot empty a target: its first alignment is kept.)"""
    W = 64
    sb = synth.generate(9, 300, 6, seed=11, flank_min=10, flank_max=40, p_partial=0.3)
    kinds = "ENESNKNNE"
    rows, cigars, off = [], [], [0]
    second_n = [t for t, k in enumerate(kinds) if k == "N"][1]
    for t, kind in enumerate(kinds):
        a0, a1 = int(sb.tgt_aln_off[t]), int(sb.tgt_aln_off[t + 1])
        rid, tlen = int(sb.tgt_rid[t]), int(sb.aln[a0, 6])
        if kind == "N":
            r, c = [sb.aln[a, :9].copy() for a in range(a0, a1)], _cigars(sb, a0, a1)
            if t == second_n:
                again = r[1].copy()
                again[0:2] = r[0][0:2]                                   # rows[0]'s query, with rows[1]'s coordinates and text
                assert again[3] <= again[1]
                r.insert(2, again); c.insert(2, c[1])
            rows += r; cigars += c
        elif kind == "S":
            for a, (tstart, text, tspan, qspan) in zip(range(a0, a0 + 4), [(64, b"50M", 50, 50), (10, b"63M", 63, 63), (100, b"30M40D20M", 90, 50),
                                                                          (128, b"40M30I23M", 63, 93)]):
                q = sb.aln[a, :9].copy()
                assert min(tspan, qspan) < W and qspan <= int(q[1]) and tstart + tspan <= tlen
                q[2], q[3], q[4], q[7], q[8] = 0, qspan, 0, tstart, tstart + tspan
                rows.append(q); cigars.append(text)
        elif kind == "K":
            for a in (a0, a0 + 1):
                q = sb.aln[a, :9].copy()
                q[0], q[1], q[2], q[3] = rid, tlen, q[7], q[8]            # the target onto itself
                q[4] = 0
                rows.append(q); cigars.append(b"%dM" % (int(q[8]) - int(q[7])))
        off.append(len(rows))
    case = (sb, W, sb.tgt_rid.copy(), np.array(rows, np.uint32), np.array(off, np.uint64), cigars)
    n = np.diff(case[4].astype(np.int64))
    assert [int(x) == 0 for x in n] == [k == "E" for k in kinds] and n[0] == n[2] == n[-1] == 0
    assert n_windows(case) == 45 and n_windows(case) % 4 != 0           # k_win_pass: four windows per workgroup, the last one short
    _, dropped = kept(case)
    assert dropped == 3
    return case


def check_holes(win):
    """the window descriptors of hole_case's job: windows without overlaps at the start, inside and at the end of the list"""
    empty = win["ow_cnt"] == 0
    assert empty[:5].all() and empty[10:20].all() and empty[25:30].all() and empty[-5:].all()
    assert not empty[5:10].all() and not empty[20:25].all() and not empty[30:40].all()


SIZE_CASES = {**{f"aln_{n}": functools.partial(aln_case, n) for n in ALN_COUNTS},
              **{f"win_{n}": functools.partial(win_case, n) for n in WIN_CASES},
              "deep_128_129_200": functools.partial(deep_case, "deep_128_129_200"), "deep_64_65": functools.partial(deep_case, "deep_64_65"),
              "holes": hole_case}


# ---- hand cases ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hand_set(W):
    """(names, [(tstart, ops)], {name: overlaps the alignment gives alone, where stated}) of the hand cases run at W.  The stated
    counts are checked against the oracle's extract_windows here."""
    if W == AC.HAND_W:
        old = AC.hand_cases()
        more = AC.hand_cases_more()
        cases = {**old, **{k: v for k, (v, _) in more.items()}}
        assert len(cases) == len(old) + len(more) and list(cases)[:len(old)] == list(old)
    else:
        assert W == AC.HAND_W40
        more = AC.hand_cases_w40()
        cases = {k: v for k, (v, _) in more.items()}
    want = {k: n for k, (_, n) in more.items()}
    names, lst = list(cases), list(cases.values())
    _, _, _, rows = AC.hand_reads(lst)
    n_win = -(-AC.HAND_TLEN // W)
    for name, row, (_, ops) in zip(names, rows, lst):
        got = len(O.extract_windows(tuple(int(x) for x in row), AC.pairs_text(ops), n_win, W))
        assert name not in want or got == want[name], (W, name, got, want[name])
        assert name in want or got > 0, name
    zthr = int(0.1 * W)
    if W == AC.HAND_W40:
        assert zthr == 4 and AC.HAND_TLEN % W == 24
        assert cases["tstart_below_zthr"][0] == zthr - 1 and cases["tstart_at_zthr"][0] == zthr
        ends = {k: t0 + sum(ln for ln, ty in ops if ty != "I") for k, (t0, ops) in cases.items()}
        assert (ends["tend_above_nthr"], ends["tend_at_nthr"], ends["tend_at_tlen"]) == (AC.HAND_TLEN - zthr + 1, AC.HAND_TLEN - zthr, AC.HAND_TLEN)
    else:
        assert zthr == 1
    return names, lst, want


def hand_case(W, pick=None):
    """The job of the hand cases at W: all of them on one target, or case number `pick` alone (the reads are those of the whole
    set either way, so one set_reads serves every job of a W)."""
    _, lst, _ = hand_set(W)
    seq, qual, off, rows = AC.hand_reads(lst)
    sb = synth.SynthBatch(seq=seq, qual=qual, off=off, aln=np.zeros((0, 10), np.uint32), cig_off=np.zeros(0, np.uint64), cig=np.zeros(1, np.uint8),
                          tgt_aln_off=np.zeros(1, np.uint64), tgt_rid=np.zeros(0, np.uint32))
    sel = list(range(len(lst))) if pick is None else [pick]
    return (sb, W, np.array([0], np.uint32), rows[sel], np.array([0, len(sel)], np.uint64), [AC.pairs_text(lst[i][1]) for i in sel])
