"""not-gpu: the specification of the device FASTA (tests/chop_ref.py) against texts written out by hand, herro_chop_plan (csrc/chop_plan.h)
against the specification's piece table, every refusal with its message, and the case family of tests/chop_cases.py proving — with chop_ref
alone — that it holds what tests/test_gpu_fasta_dev.py is there to run."""
import ctypes as C

import numpy as np
import pytest

import chop_cases as CC
import chop_ref as R
from herro_amd import api


# ---- the specification against hand-written texts ------------------------------------------------------------------------------------------
HOST = b">r1 \nACGTACGTAC\n>r2:0 some words\nAAAAC\n>r2:1 some words\nGGGGGGGGGGGG\n"
HOST_ENDS = [16, len(HOST)]


def test_all_zero_is_the_identity():
    text, st, ends = R.chop(HOST, 0, 0, 0, HOST_ENDS)
    assert text == HOST and ends == HOST_ENDS
    assert st == R.Stats(records=3, bases=27, pieces_dropped=0, bases_dropped=0, segments=3, targets=2)


def test_sliding_names_and_remainders():
    text, st, ends = R.chop(HOST, 4, 0, 0, HOST_ENDS)
    assert text == (b">r1_sliding:1-4 \nACGT\n>r1_sliding:5-8 \nACGT\n>r1_sliding:9-10 \nAC\n"
                    b">r2:0_sliding:1-4 some words\nAAAA\n>r2:0_sliding:5-5 some words\nC\n"
                    b">r2:1_sliding:1-4 some words\nGGGG\n>r2:1_sliding:5-8 some words\nGGGG\n>r2:1_sliding:9-12 some words\nGGGG\n")
    assert st == R.Stats(8, 27, 0, 0, 3, 2) and ends == [text.index(b">r2"), len(text)]


def test_one_piece_still_gets_the_suffix_and_the_filter_keeps_the_segment_numbers():
    text, st, ends = R.chop(HOST, 12, 6, 0, HOST_ENDS)
    assert text == b">r1_sliding:1-10 \nACGTACGTAC\n>r2:1_sliding:1-12 some words\nGGGGGGGGGGGG\n"      # r2:0 (5 bases) is gone, r2:1 keeps its number
    assert st == R.Stats(2, 22, 1, 5, 3, 2)
    text, st, ends = R.chop(HOST, 0, 11, 0, HOST_ENDS)
    assert text == b">r2:1 some words\nGGGGGGGGGGGG\n" and ends == [0, len(text)] and st == R.Stats(1, 12, 2, 15, 3, 1)


def test_line_width():
    assert R.chop(HOST, 0, 0, 5, HOST_ENDS)[0] == b">r1 \nACGTA\nCGTAC\n>r2:0 some words\nAAAAC\n>r2:1 some words\nGGGGG\nGGGGG\nGG\n"   # no empty line behind a full one
    assert R.chop(HOST, 6, 4, 3, HOST_ENDS)[0] == (b">r1_sliding:1-6 \nACG\nTAC\n>r1_sliding:7-10 \nGTA\nC\n>r2:0_sliding:1-5 some words\nAAA\nAC\n"
                                                   b">r2:1_sliding:1-6 some words\nGGG\nGGG\n>r2:1_sliding:7-12 some words\nGGG\nGGG\n")
    assert R.chop(HOST, 0, 0, 60, HOST_ENDS)[0] == HOST


def test_pieces_rule():
    assert R.pieces(10, 0) == [(0, 10)] and R.pieces(0, 0) == [(0, 0)] and R.pieces(0, 3) == []
    assert R.pieces(9, 3) == [(0, 3), (3, 6), (6, 9)] and R.pieces(10, 3)[-1] == (9, 10) and R.pieces(2, 3) == [(0, 2)]
    assert R.kept_pieces(10, 3, 2) == [(0, 3), (3, 6), (6, 9)] and R.kept_pieces(10, 3, 4) == [] and R.kept_pieces(10, 0, 10) == [(0, 10)]


# ---- herro_chop_plan against the piece table ----------------------------------------------------------------------------------------------------
def _same_plan(lengths, C_, M):
    pieces, off, st = api.chop_plan(lengths, chop_len=C_, min_length=M)
    rows, roff, rst = R.piece_table(lengths, C_, M)
    assert [tuple(int(x) for x in p) for p in pieces.tolist()] == rows, (lengths[:8], C_, M)
    assert off.tolist() == roff and tuple(st) == rst


def test_chop_plan_on_the_case_lengths():
    for W in (16, 40):
        text, _ = CC.host_text(CC.hand_case(W))
        lengths = [len(s) for _, _, s in R.parse(text)]
        for C_, M, _ in CC.param_sets(text, W):
            _same_plan(lengths, C_, M)


def test_chop_plan_on_random_lengths():
    rng = np.random.default_rng(15)
    for trial in range(300):
        n = int(rng.integers(0, 12))
        lengths = [int(x) for x in rng.integers(0, [4, 40, 2000][trial % 3], n)]
        C_ = int(rng.integers(0, 50)) if trial % 4 else 0
        M = int(rng.integers(0, 60)) if trial % 5 else 0
        _same_plan(lengths, C_, M)
    _same_plan([100000, 29999, 30000, 30001, 9999, 70000], **{"C_": api.POSTPROCESS["chop_len"], "M": api.POSTPROCESS["min_length"]})
    _same_plan([(1 << 32) - 1], (1 << 31) - 1, 0)      # the longest sequence that is taken


def test_postprocess_numbers():
    assert api.POSTPROCESS == dict(chop_len=30000, min_length=10000)    # seqkit sliding -s 30000 -W 30000 -g | seqkit seq -m 10000


def _plan_rc(n, lens, p):
    L = api.lib()
    h, err = C.c_void_p(), C.create_string_buffer(256)
    arr = None if lens is None else np.ascontiguousarray(lens, np.uint64)
    rc = L.herro_chop_plan(n, None if arr is None else arr.ctypes.data, None if p is None else C.byref(p), C.byref(h), err, 256)
    if h:
        L.herro_trim_free(h)
    return rc, err.value.decode()


def test_every_refusal_and_its_message():
    L = api.lib()
    inv = _plan_rc(2, None, None)
    assert inv[0] != 0 and inv[1] == "herro_chop_plan: null argument"
    code_invalid = inv[0]
    err = C.create_string_buffer(256)
    assert L.herro_chop_plan(0, None, None, None, err, 256) == code_invalid and err.value == b"herro_chop_plan: null argument"
    assert _plan_rc(0, None, None) == (0, "")                                   # no sequences, no parameters: an empty plan
    p = api.ChopParams(chop_len=5)
    p.reserved[3] = 1
    assert _plan_rc(1, [7], p) == (code_invalid, "herro_chop_plan: reserved fields must be 0")
    assert _plan_rc(1, [7], api.ChopParams(flags=1)) == (code_invalid, "herro_chop_plan: unknown flag")
    assert _plan_rc(1, [7], api.ChopParams(chop_len=1 << 31)) == (code_invalid, "herro_chop_plan: chop_len = 2147483648: at most 2^31 - 1")
    assert _plan_rc(1, [7], api.ChopParams(line_width=1 << 31)) == (code_invalid, "herro_chop_plan: line_width = 2147483648: at most 2^31 - 1")
    assert _plan_rc(1, [7], api.ChopParams(chop_len=(1 << 31) - 1, line_width=(1 << 31) - 1, min_length=0xFFFFFFFF))[0] == 0
    uns = _plan_rc(2, [5, 1 << 32], None)
    assert uns[0] not in (0, code_invalid) and uns[1] == "herro_chop_plan: sequence 1: 4294967296 bases, 2^32 or more"
    many = _plan_rc(2, [(1 << 32) - 1, 1], api.ChopParams(chop_len=1))
    assert many == (uns[0], "herro_chop_plan: more than 2^32 - 1 pieces")
    with pytest.raises(ValueError, match="more than 2\\^32 - 1 pieces"):
        api.chop_plan([(1 << 32) - 1, 1], chop_len=1)
    with pytest.raises(ValueError, match="32-bit"):
        api.chop_plan([1], chop_len=1 << 32)


# ---- the case family proves its own coverage -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["w16", "w40", "big"])
def test_the_cases_hold_what_the_gpu_test_is_there_to_run(name):
    case = CC.big_case() if name == "big" else CC.hand_case(int(name[1:]))
    text, ends = CC.host_text(case)
    params = CC.BIG_PARAMS if name == "big" else CC.param_sets(text, case.W)
    cov = CC.coverage(text, ends, params)
    assert all(cov.values()), cov
    lens = [len(s) for _, _, s in R.parse(text)]
    pats = [t.pattern for t in case.targets]
    if name == "big":
        assert sum(len(p) for p in pats) > CC.SCAN_TILE and max(R.chop(text, C_, M, L, ends)[1].records for C_, M, L in params) > CC.SCAN_TILE
        return
    W = case.W
    # the patterns: none, all, gaps at the front, at the back, at both ends, one in the middle, alternating, a single window, a target without id
    assert any(set(p) == {"0"} for p in pats) and any(set(p) == {"1"} for p in pats)
    assert any(p[0] == "0" and p[-1] == "1" for p in pats) and any(p[0] == "1" and p[-1] == "0" for p in pats) and any(p[0] == p[-1] == "0" and "1" in p for p in pats)
    assert any(len(CC.runs_of(p)) == 2 for p in pats) and any(len(CC.runs_of(p)) >= 11 for p in pats) and any(p.count("1") == 1 for p in pats)
    assert any(t.id is None for t in case.targets) and any(t.id is not None and len(t.id) == 1 for t in case.targets)
    assert any(t.id is not None and len(t.id) > 256 for t in case.targets) and any(t.desc for t in case.targets) and any(not t.desc for t in case.targets)
    assert max(lens) >= 1000                                                # coordinates across 9 -> 10, 99 -> 100, 999 -> 1000 at chop_len 1
    Cs, Ms, Ls = ({p[i] for p in params} for i in range(3))
    n0 = max(lens)
    assert {0, 1, W - 1, W, W + 1, n0 - 1, n0 + 1} <= Cs and any(1 < c < n0 and n0 % c == 0 for c in Cs)
    assert {0, 1, 7, 60} <= Ls and {0, 1} <= Ms
    for C_ in Cs - {0}:
        mine = {m for c, m, _ in params if c == C_}
        assert {C_, C_ + 1} <= mine
        rems = {n % C_ for n in lens if n % C_}
        assert not rems or any(r in mine and r + 1 in mine for r in rems)
        piece = min(C_, n0)
        assert piece <= 1 or {piece, piece - 1} <= {l for c, _, l in params if c == C_}
