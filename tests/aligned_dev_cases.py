"""Helpers shared by tests/test_aligned_dev_host.py and tests/test_gpu_aligned_dev.py: CIGAR text <-> the binary ops of
herro_aligned_dev_from_ops (len << 2 | {0 M, 1 I, 2 D}), the comparison of an aligned job with the text path's, the hand-made
alignments at the edges of k_ops_scan and of the windowing (the latter for tests/build_cases.py) and the records of the aligner's test."""
import re

import numpy as np

_OP = re.compile(rb"(\d+)([MID])")
_TY = {"M": 0, "I": 1, "D": 2}


def cigar_ops(cigar: bytes) -> np.ndarray:
    got = _OP.findall(cigar)
    assert b"".join(n + t for n, t in got) == cigar, cigar[:60]
    return np.array([(int(n) << 2) | _TY[t.decode()] for n, t in got], np.uint32)


def cigars_to_ops(cigars):
    """(op_off u64 [n + 1], ops u32) of a list of CIGAR texts"""
    per = [cigar_ops(c) for c in cigars]
    off = np.zeros(len(per) + 1, np.uint64)
    off[1:] = np.cumsum([len(p) for p in per])
    return off, (np.concatenate(per) if per else np.zeros(0, np.uint32)).astype(np.uint32)


def pairs_text(pairs) -> bytes:
    return "".join(f"{ln}{ty}" for ln, ty in pairs).encode()


def pairs_ops(pairs) -> np.ndarray:
    return np.array([(ln << 2) | _TY[ty] for ln, ty in pairs], np.uint32)


def same_jobs(c, ja, jt, tag):
    """job_arrays of an aligned job and of the text path's: equal field for field; ow.op_begin through the slices it opens
    (the aligned job's op array has exactly n_ops slots per alignment, the text path's len / 2 + 1)"""
    a, t = c.job_arrays(ja), c.job_arrays(jt)
    assert set(a) == set(t)
    for k in ("win", "tile_win", "tile_r0", "tgt_win_off"):
        assert a[k].dtype == t[k].dtype and len(a[k]) == len(t[k]), (tag, k, len(a[k]), len(t[k]))
        for f in a[k].dtype.names or [None]:
            x, y = (a[k], t[k]) if f is None else (a[k][f], t[k][f])
            assert np.array_equal(x, y), (tag, k, f, np.flatnonzero(x != y)[:5])
    assert len(a["ow"]) == len(t["ow"]), (tag, len(a["ow"]), len(t["ow"]))
    for f in a["ow"].dtype.names:
        if f != "op_begin":
            assert np.array_equal(a["ow"][f], t["ow"][f]), (tag, "ow", f, np.flatnonzero(a["ow"][f] != t["ow"][f])[:5])
    for i in range(len(a["ow"])):
        n = int(a["ow"]["op_cnt"][i])
        ba, bt = int(a["ow"]["op_begin"][i]), int(t["ow"]["op_begin"][i])
        assert ba + n <= len(a["ops"]) and np.array_equal(a["ops"][ba:ba + n], t["ops"][bt:bt + n]), (tag, "ops of overlap", i)
    assert ja.skipped() == jt.skipped(), tag
    return a, t


# ---- hand cases: W = 16, one target of 704 bp, every query read made of the bases its ops consume ---------------------------------
HAND_W = 16
HAND_TLEN = 704


def _alt(n, tspan):
    """n ops that start and end with M and never repeat a type: M D M I M D ... (an even n gets 'M D I M ...'); gaps of one base, the
    M lengths share what is left of tspan target bases"""
    ty = ["M" if i % 2 == 0 else "DI"[(i // 2) % 2] for i in range(n if n % 2 else n - 1)]
    if n % 2 == 0:
        ty.insert(2, "I")
    assert len(ty) == n and ty[0] == ty[-1] == "M" and all(x != y for x, y in zip(ty, ty[1:]))
    n_m, n_d = ty.count("M"), ty.count("D")
    each, extra = divmod(tspan - n_d, n_m)
    assert each >= 1
    out, k = [], 0
    for x in ty:
        if x == "M":
            out.append((each + (1 if k < extra else 0), "M"))
            k += 1
        else:
            out.append((1, x))
    return out


def hand_cases():
    """name -> (tstart, [(len, type)]).  Window boundaries are the multiples of 16, a step of k_ops_scan is 64 ops."""
    cut63 = [(1, t) for _, t in _alt(63, 63)]        # ops 0 .. 62, one base each: 32 M + 16 D = 48 target bases, 17 -> 65
    cut63 += [(20, "D"), (100, "M"), (2, "I"), (50, "M")]   # op 63 (lane 63 of step 0): 65 -> 85 across 80; o1, o2 are ops 64, 65 of step 1
    return {
        "one_op": (32, [(640, "M")]),                                                     # also one M over forty windows
        "ops_64": (16, _alt(64, 600)),
        "ops_65": (16, _alt(65, 600)),
        "ops_201": (8, _alt(201, 680)),                                                   # four steps: three carries
        "cut_on_op_63": (17, cut63),
        "m_three_windows": (48, [(5, "M"), (1, "I"), (60, "M"), (2, "D"), (40, "M")]),    # 60M: 53 -> 113 across 64, 80, 96, 112
        "d_across_boundary": (32, [(14, "M"), (5, "D"), (45, "M"), (1, "I"), (64, "M")]), # 5D: 46 -> 51 across 48
        "i_before_boundary": (32, [(16, "M"), (3, "I"), (48, "M"), (1, "D"), (63, "M")]), # 16M ends on 48, the insertion sits on the boundary
        "tstart_odd": (37, [(100, "M"), (1, "D"), (2, "I"), (150, "M")]),
    }


def hand_cases_more():
    """name -> ((tstart, [(len, type)]), overlaps the alignment gives alone).  More cases at W = 16 beside hand_cases(), which
    tests/test_gpu_aligned_dev.py reads by name and expects a window from every entry of: ends of the target, gaps on and around a
    boundary, the shortest alignment that is windowed and the two that just are not.  704 = 44 * 16."""
    return {
        "d_three_windows": ((40, [(6, "M"), (40, "D"), (30, "M")]), 4),                       # 40D: 46 -> 86 across 48, 64, 80
        "ends_on_boundary": ((32, [(20, "M"), (1, "I"), (44, "M")]), 4),                      # 32 -> 96, the last op ends on 96
        "from_zero_to_tail": ((0, [(300, "M"), (2, "D"), (1, "I"), (402, "M")]), 44),         # the whole target
        "tail_short": ((600, [(50, "M"), (1, "D"), (53, "M")]), 6),                           # ends at 704, an exact multiple
        "tail_inexact": ((601, [(50, "M"), (1, "D"), (45, "M")]), 5),                         # ends at 697: the tail window rule
        "i_then_d_on_boundary": ((32, [(16, "M"), (2, "I"), (3, "D"), (60, "M")]), 4),        # 16M ends on 48, 2I stays, 3D opens the next
        "d_ends_on_boundary_then_i": ((32, [(10, "M"), (6, "D"), (2, "I"), (60, "M")]), 4),   # 6D ends on 48 with an insertion behind it
        "exactly_W": ((32, [(16, "M")]), 1),
        "W_minus_1": ((32, [(15, "M")]), 0),
        "q_short": ((32, [(5, "M"), (20, "D"), (5, "M")]), 0),                                # 30 target bases, 10 of the query: below W
    }


HAND_W40 = 40


def hand_cases_w40():
    """name -> ((tstart, ops), overlaps alone) at W = 40 on the same target: the zero-threshold rules (windowing.rs:65-85, 261-272)
    with a threshold of 4 (at W = 16 it is 1 and `tstart < 1` is `tstart == 0`), and a ragged last window: 704 = 17 * 40 + 24,
    tlen - 4 = 700."""
    mid = [(100, "M"), (1, "D"), (2, "I"), (150, "M")]                                        # 251 target bases
    return {
        "tstart_below_zthr": ((3, mid), 6),                                                   # 3 < 4: window 0 is opened at 3
        "tstart_at_zthr": ((4, mid), 5),                                                      # 4 is not: the first window is 1
        "tend_above_nthr": ((500, [(100, "M"), (1, "I"), (101, "M")]), 5),                    # ends at 701 > 700: the tail window
        "tend_at_nthr": ((500, [(100, "M"), (1, "I"), (100, "M")]), 4),                       # ends at 700: none
        "tend_at_tlen": ((500, [(100, "M"), (1, "I"), (104, "M")]), 5),                       # ends at 704
        "whole": ((0, [(704, "M")]), 18),
        "d_over_tail_boundary": ((600, [(70, "M"), (20, "D"), (14, "M")]), 3),                # 20D: 670 -> 690 across 680, the last boundary
    }


INS_PAIR_CASE = (16, [(30, "M"), (2, "I"), (3, "I"), (60, "M")])
ZERO_LEN_CASE = (16, [(30, "M"), (0, "D"), (60, "M")])


def hand_reads(cases, seed=5):
    """(seq, qual, off, rows): read 0 is the target, read 1 + i the query of case i — ten random bases, the bases its ops consume
    (M: the target's, I: random), ten random bases; forward strand.  rows u32 [n, 9] with consistent coordinates."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    target = acgt[rng.integers(0, 4, HAND_TLEN)]
    reads, rows = [target], []
    for i, (tstart, ops) in enumerate(cases):
        t, q = tstart, [acgt[rng.integers(0, 4, 10)]]
        for ln, ty in ops:
            if ty == "M":
                q.append(target[t:t + ln])
            elif ty == "I":
                q.append(acgt[rng.integers(0, 4, ln)])
            if ty != "I":
                t += ln
        assert t <= HAND_TLEN
        q.append(acgt[rng.integers(0, 4, 10)])
        q = np.concatenate(q)
        reads.append(q)
        rows.append([1 + i, len(q), 10, len(q) - 10, 0, 0, HAND_TLEN, tstart, t])
    off = np.zeros(len(reads) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads])
    seq = np.concatenate(reads)
    return seq, np.full(len(seq), ord("5"), np.uint8), off, np.array(rows, np.uint32)


# ---- the aligner's handle: ~300 records ---------------------------------------------------------------------------------------------
def align_batch():
    """(sb, rows): both strands, partial overlaps, 0.5 .. 8 % error, one region of one base, one of >= 10 kb, two records that fail
    (one side empty: nothing but an indel, which the trim drops)"""
    from herro_amd import synth
    sb = synth.merge([
        synth.generate(3, 1024, 32, seed=111, p_partial=0.3, min_partial_len=64),                      # ~1.6 % error
        synth.generate(3, 1024, 32, seed=112, p_sub=0.03, p_ins=0.025, p_del=0.025, p_partial=0.2),    # 8 %
        synth.generate(3, 1024, 32, seed=113, p_sub=0.002, p_ins=0.0015, p_del=0.0015),                # 0.5 %
        synth.generate(1, 12000, 4, seed=114, flank_min=200, flank_max=400),                           # >= 10 kb
    ])
    rows = sb.aln[:, :9].copy()
    one = rows[5].copy()                      # one base of each read, the same offset into both regions
    if one[4] == 0:
        one[2], one[3] = one[2] + 100, one[2] + 101
    else:
        one[3], one[2] = one[3] - 100, one[3] - 101
    one[7], one[8] = one[7] + 100, one[7] + 101
    no_q, no_t = rows[40].copy(), rows[41].copy()
    no_q[3] = no_q[2]
    no_t[8] = no_t[7]
    return sb, np.concatenate([rows, np.array([one, no_q, no_t], np.uint32)])
