"""The read sets and piece tables of the store-cut tests (tests/test_cut_host.py, tests/test_gpu_cut.py): the smallest shapes at which
k_store_cut_words and k_store_cut_qual (csrc/store_dev.hip) can go wrong.  All seeded; qualities are random bytes, so that a byte taken from
the wrong place shows.

grid      source reads of 1, 31, 32, 33, 64, 65, 96 and 600 bases, each followed by a read of all T (code 3: a missing tail mask or a read
          past the piece shows as set bits); pieces at start & 31 in {0, 1, 15, 31} of 0, 1, 31, 32, 33, 63, 64 and 65 bases and to the
          read's last base.  The store's last read is a source read too: its second source word is the pad word.
residues  pieces of 0 .. 40 bases placed so that the source and the destination quality offset take every residue modulo 16 against each
          other, once with a piece short enough to lie in boundary chunks only and once with one that holds a whole 16-byte chunk.
nonacgt   adapter_cases.set_nonacgt() and a read whose last base is N (its smear reaches above the read's end in the old store): pieces that
          end at the read's end, pieces that start one base behind a non-ACGT byte.  The host path differs here (acgt False).
shapes    several pieces of one read in descending order, the same piece twice, an empty table, the identity table.
long      one read of 200 000 bases cut into three pieces of more than 2048 words each: every kernel spans several workgroups and strides."""
import numpy as np

import adapter_cases as AC
import lowcomplexity as LC
from herro_amd import api

START_RESIDUES = (0, 1, 15, 31)
PIECE_LENGTHS = (0, 1, 31, 32, 33, 63, 64, 65)
GRID_READS = (1, 31, 32, 33, 64, 65, 96, 600)


def pieces(rows) -> np.ndarray:
    a = np.zeros(len(rows), api.PIECE_DTYPE)
    for i, (r, s, e) in enumerate(rows):
        a[i] = (r, s, e)
    return a


def _quals(rng, reads):
    return [rng.integers(33, 127, len(r)).astype(np.uint8) for r in reads]


def set_grid():
    rng = np.random.default_rng(301)
    reads, rows = [], []
    for k, n in enumerate(GRID_READS + (65,)):                                          # the last one stays the store's last read
        rid = len(reads)
        reads.append(LC._rand(rng, n))
        starts = sorted({s for r in START_RESIDUES for s in (r, 32 + r, (n - 1) // 32 * 32 + r, n // 32 * 32 + r) if s <= n})
        for s in starts:
            rows += [(rid, s, s + m) for m in PIECE_LENGTHS if s + m <= n]
            rows.append((rid, s, n))                                        # to the read's last base
        if k < len(GRID_READS):
            reads.append(b"T" * 40)
    assert len(reads) == 2 * len(GRID_READS) + 1 and len(reads[-1]) == 65
    return dict(reads=reads, quals=_quals(rng, reads), tables=[("grid", pieces(rows))], acgt=True)


def set_residues():
    rng = np.random.default_rng(302)
    reads = [LC._rand(rng, 5), LC._rand(rng, 700), LC._rand(rng, 20)]       # read 1 begins at quality byte 5
    rows, dst, seen_short, seen_long = [], 0, set(), set()
    k = 0
    for want_dst in range(16):
        for src in range(16):
            for long_one in (False, True):
                fill = (want_dst - dst) % 16                                # a filler piece moves the destination to the residue wanted
                rows.append((2, 0, fill))
                dst += fill
                start = (src - 5) % 16 + 16 * (k % 20)                      # (5 + start) % 16 == src
                length = 32 + (k // 2) % 9 if long_one else (k // 2) % 32   # 32 .. 40: a whole aligned chunk lies inside; 0 .. 31
                rows.append((1, start, start + length))
                (seen_long if long_one else seen_short).add(((5 + start) % 16, dst % 16))
                dst += length
                k += 1
    assert len(seen_long) == 256 and len(seen_short) == 256
    assert {e - s for _, s, e in rows} >= set(range(41))
    return dict(reads=reads, quals=_quals(rng, reads), tables=[("residues", pieces(rows))], acgt=True)


def set_nonacgt():
    rng = np.random.default_rng(303)
    reads = list(AC.set_nonacgt()["reads"]) + [LC._rand(rng, 70) + b"N", LC._rand(rng, 63) + b"N" + LC._rand(rng, 40), b"T" * 40]
    rows = []
    for rid, r in enumerate(reads):
        n = len(r)
        rows.append((rid, 0, n))
        for p in [i for i, b in enumerate(r) if b not in b"ACGTacgt"][:6]:
            rows += [(rid, s, n) for s in (max(p - 33, 0), p, p + 1) if s <= n]           # ends at the read's end
            rows += [(rid, p + 1, e) for e in (p + 1, p + 2, p + 5, p + 34) if p + 1 <= e <= n]   # starts one base behind the byte
            rows.append((rid, max(p - 40, 0), p + 1))                                     # ends on it
    return dict(reads=reads, quals=_quals(rng, reads), tables=[("nonacgt", pieces(rows))], acgt=False)


def set_shapes():
    rng = np.random.default_rng(304)
    reads = [LC._rand(rng, n) for n in (100, 257, 64, 33)]
    ident = [(i, 0, len(r)) for i, r in enumerate(reads)]
    return dict(reads=reads, quals=_quals(rng, reads), acgt=True,
                tables=[("descending", pieces([(1, 200, 257), (1, 130, 200), (1, 64, 129), (1, 0, 64), (0, 3, 99)])),
                        ("twice", pieces([(2, 7, 50), (3, 0, 33), (2, 7, 50)])),
                        ("empty", pieces([])),
                        ("identity", pieces(ident))])


def set_long():
    rng = np.random.default_rng(305)
    reads = [LC._rand(rng, 200000), b"T" * 40]
    table = pieces([(0, 5, 66000), (0, 66031, 133000), (0, 133001, 200000)])
    assert all((int(p["end"]) - int(p["start"])) // 32 > 2048 for p in table)
    return dict(reads=reads, quals=_quals(rng, reads), tables=[("long", table)], acgt=True)


MAKERS = dict(grid=set_grid, residues=set_residues, nonacgt=set_nonacgt, shapes=set_shapes, long=set_long)
_SETS, _REF = {}, {}


def get(name):
    if name not in _SETS:
        _SETS[name] = MAKERS[name]()
    return _SETS[name]


ALL_TABLES = [(name, i) for name in MAKERS for i in range(len(get(name)["tables"]))]
IDS = [f"{n}-{get(n)['tables'][i][0]}" for n, i in ALL_TABLES]


def arrays(name):
    """(seq, qual, off) of Context.set_reads"""
    s = get(name)
    seq = np.frombuffer(b"".join(s["reads"]), np.uint8)
    qual = np.concatenate(s["quals"]).astype(np.uint8)
    off = np.concatenate([[0], np.cumsum([len(r) for r in s["reads"]])]).astype(np.uint64)
    return seq, qual, off


def reference(name, table: int):
    """(the old store, cut_ref.cut of it) of table `table` of the set: computed once, shared and left unchanged"""
    import cut_ref as CR
    if (name, None) not in _REF:
        s = get(name)
        _REF[name, None] = CR.store_of(s["reads"], s["quals"])
        for a in _REF[name, None].values():
            a.setflags(write=False)
    if (name, table) not in _REF:
        _REF[name, table] = CR.cut(_REF[name, None], get(name)["tables"][table][1])
        for a in _REF[name, table].values():
            a.setflags(write=False)
    return _REF[name, None], _REF[name, table]
