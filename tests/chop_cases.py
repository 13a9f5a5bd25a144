"""Jobs for the device FASTA (csrc/fasta_dev.hip), shared by tests/test_chop_host.py (no device: the family proves its own coverage with
chop_ref alone) and tests/test_gpu_fasta_dev.py.  A hand case is a set of targets with a pattern of corrected windows each, made the way
aligned_dev_cases.hand_reads makes its reads: a window is corrected iff two alignments cover it, and every maximal run of corrected windows
gets two query reads that are copies of the target's bases under the run (one M op from the run's first window boundary to its last), so
the corrected bases are the target's and the text herro_job_fasta gives is known without a device (`host_text`): the GPU test asserts that
prediction first, and the coverage proved from it here is then coverage of what the kernels were given.

A run whose windows all have cons_len 0 cannot be built from alignments: a window loses all its bases only under a deletion that spans it,
an alignment neither begins nor ends with a deletion, and whatever M op carries it into the window's neighbours corrects them as well — the
run is longer than the empty window.  herro_job_fasta drops such a segment before chop_ref sees any text; the rule is stated in DESIGN.md."""
import dataclasses
import functools

import numpy as np

import chop_ref as R

FLANK = 10
SCAN_TILE = 2048          # elements of one tile of the scan the kernels use (scan_sort_dev.h: 256 threads x 8)


@dataclasses.dataclass(frozen=True)
class Target:
    name: str
    pattern: str          # one character per window: '1' corrected, '0' not
    short: int            # bases the last window lacks
    id: object            # bytes, or None: the target gives nothing
    desc: object          # bytes or None


@dataclasses.dataclass(frozen=True)
class Case:
    W: int
    seq: np.ndarray
    qual: np.ndarray
    off: np.ndarray
    rids: np.ndarray
    rows: np.ndarray
    aln_off: np.ndarray
    cigars: list
    ids: list
    descs: list
    targets: tuple
    tlen: tuple


def runs_of(pattern: str):
    out, a = [], None
    for w, ch in enumerate(pattern + "0"):
        if ch == "1" and a is None:
            a = w
        elif ch != "1" and a is not None:
            out.append((a, w))
            a = None
    return out


def build(W: int, targets, seed: int) -> Case:
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    tlen = [len(t.pattern) * W - t.short for t in targets]
    reads = [acgt[rng.integers(0, 4, n)] for n in tlen]
    rows, cigars, aln_off = [], [], [0]
    for t, tg in enumerate(targets):
        assert 0 <= tg.short < W and tg.pattern
        for a, b in runs_of(tg.pattern):
            t0, t1 = a * W, min(b * W, tlen[t])
            assert t1 - t0 >= W, (tg.name, "a run must span a whole window to be windowed at all")
            for _ in range(2):
                q = np.concatenate([acgt[rng.integers(0, 4, FLANK)], reads[t][t0:t1], acgt[rng.integers(0, 4, FLANK)]])
                rows.append([len(reads), len(q), FLANK, len(q) - FLANK, 0, t, tlen[t], t0, t1])
                cigars.append(b"%dM" % (t1 - t0))
                reads.append(q)
        aln_off.append(len(rows))
    off = np.zeros(len(reads) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads])
    seq = np.concatenate(reads)
    return Case(W, seq, np.full(len(seq), ord("5"), np.uint8), off, np.arange(len(targets), dtype=np.uint32), np.array(rows, np.uint32).reshape(-1, 9),
                np.array(aln_off, np.uint64), cigars, [t.id for t in targets], [t.desc for t in targets], tuple(targets), tuple(tlen))


def host_text(case: Case, with_none: bool = False):
    """(text, rec_end) herro_job_fasta gives for the case: every run of corrected windows is a segment holding the target's bases under it"""
    out, ends, n = [], [], 0
    for t, tg in enumerate(case.targets):
        if tg.id is not None or with_none:
            name = tg.id if tg.id is not None else b"none%d" % t
            runs = runs_of(tg.pattern)
            tb = case.seq[int(case.off[t]):int(case.off[t + 1])].tobytes()
            for i, (a, b) in enumerate(runs):
                rec = b">" + name + (b":%d" % i if len(runs) > 1 else b"") + b" " + (tg.desc or b"") + b"\n" + tb[a * case.W:min(b * case.W, case.tlen[t])] + b"\n"
                out.append(rec)
                n += len(rec)
        ends.append(n)
    return b"".join(out), ends


LONG_ID = b"L" + b"o" * 298 + b"ng"      # 301 bytes


@functools.lru_cache(maxsize=None)
def hand_case(W: int) -> Case:
    n_long = -(-1030 // W)                # segment coordinates cross 9 -> 10, 99 -> 100, 999 -> 1000 at chop_len 1
    T = [
        Target("none", "00000", 0, b"none", None),
        Target("all", "111111", 3, b"a", b"d e s c"),                      # an id of one byte; a ragged last window
        Target("front_gap", "00111", 0, LONG_ID, None),                    # an id above 256 bytes
        Target("back_gap", "11100", 5, b"back", b""),
        Target("both_gaps", "01110", 0, b"both", LONG_ID),
        Target("middle_gap", "110111", 1, b"mid", b"x"),                   # two segments
        Target("alternating", "10" * 11 + "1", 0, b"alt", None),           # twelve segments: ':9' -> ':10'
        Target("single", "00100", 0, b"s", None),
        Target("no_id", "1111", 0, None, b"never written"),
        Target("long", "1" * n_long, W // 2, b"long", b"1 kb"),
    ]
    c = build(W, T, seed=100 + W)
    assert max(c.tlen) >= 1000
    return c


@functools.lru_cache(maxsize=None)
def big_case() -> Case:
    """more windows, more runs' worth of scan entries and (at chop_len <= 16) more pieces than one tile of the scan"""
    W = 16
    T = [Target("alt", "10" * 5 + "1", 0, b"alt", None), Target("big", "1" * 2100, 7, b"big", b"33 kb"), Target("tail", "0110", 0, b"t", None)]
    c = build(W, T, seed=7)
    assert sum(len(t.pattern) for t in T) > SCAN_TILE
    return c


BIG_PARAMS = ((0, 0, 0), (16, 0, 0), (1, 1, 0), (30000, 10000, 60), (1000, 593, 60), (15, 15, 7))


def param_sets(text: bytes, W: int):
    """(chop_len, min_length, line_width) triples for a case whose host text is `text`: every value of the three lists of DESIGN.md section 15's
    tests, each list against the neutral value of the other two, and the mixed triples that matter (filter and wrap together)."""
    lens = sorted({len(s) for _, _, s in R.parse(text)})
    n0 = lens[-1]
    assert n0 >= 4
    d = next((k for k in range(2, n0) if n0 % k == 0), 1)
    Cs = [0, 1, W - 1, W, W + 1, n0 // d, n0 - 1, n0 + 1]            # ..., divides the longest segment, leaves 1 of it, above every segment
    out = []
    for C in Cs:
        rem = next((n % C for n in lens if C and n % C), 0)
        piece = C if 0 < C <= n0 else n0
        Ms = [0, 1, rem, rem + 1, C, C + 1]
        Ls = [0, 1, 7, 60, piece, piece - 1] if piece > 1 else [0, 1, 7, 60]
        out += [(C, M, 0) for M in Ms] + [(C, 0, L) for L in Ls] + [(C, rem, piece), (C, rem + 1, 7)]
    return list(dict.fromkeys(out))


def coverage(text: bytes, ends, params):
    """what a set of calls covers, from chop_ref alone: a dict of condition -> bool"""
    recs = [R.parse(text[a:b]) for a, b in zip([0] + list(ends[:-1]), ends)]
    cov = dict(two_segments=any(len(r) >= 2 for r in recs), kept_remainder=False, dropped_remainder=False, one_piece=False, exact_lines=False,
               silent_target=False)
    for C, M, L in params:
        _, st, out_ends = R.chop(text, C, M, L, ends)
        cov["silent_target"] |= any(b == a for a, b in zip([0] + out_ends[:-1], out_ends))
        for r in recs:
            for _, _, s in r:
                ps = R.pieces(len(s), C)
                if C and len(s) % C:
                    cov["kept_remainder" if len(s) % C >= M else "dropped_remainder"] = True
                cov["one_piece"] |= C > 0 and len(ps) == 1
                cov["exact_lines"] |= L > 0 and any(b - a >= M and b - a >= L and (b - a) % L == 0 for a, b in ps)
    return cov
