"""The read sets of the adapter tests (tests/test_adapters_host.py, tests/test_gpu_adapters.py).  All seeded and small: reads of at most a
few kilobases, a few hundred reads in all, so that tests/adapter_ref.py answers each set in about a second.

grid      reads of 1 .. 600 bases (every length around a 32-base plane word, a 64-base store word and the default segment) against
          adapters of 8 .. 64 bases at every error bound; texts shorter than the pattern.
planted   copies of three adapters (28, 22 and a palindromic 24 bases) at the read's first base, ending at its last, across a plane-word
          boundary, a store-word boundary and the default segment's seam; with 0, k and k + 1 substitutions, insertions, deletions; on
          both strands; two copies back to back and one base apart.
runs      homopolymer and dinucleotide reads against AAAAAAAA and (AC)x16: one run over many segments that ends at the read's last base.
nonacgt   reads with bytes that are not ACGT (the store's codes for them), adapters planted beside them.
random    random text: an 8-base adapter at k = 1 (many chance hits), 28- and 22-base adapters at 150 per mille (none).
chimera   pair_cases.set_d's reads with an exact adapter in front of every read, the second adapter's reverse complement behind every
          third, and two chimeras joined through tail + head adapters."""
import numpy as np

import adapter_ref as AR
import lowcomplexity as LC
import pair_cases as PC

_RNG = np.random.default_rng(100)
A28, A22 = LC._rand(_RNG, 28), LC._rand(_RNG, 22)          # arbitrary sequences: no adapter list is built in anywhere
PAL = b"ACGGTCATGCAT" + LC.rc(b"ACGGTCATGCAT")
GRID_LENGTHS = (1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 95, 96, 97, 255, 256, 257, 600)
GRID_ADAPTER_LENGTHS = (8, 9, 31, 32, 33, 63, 64)
GRID_PM = (0, 1, 100, 250, 500)          # 0: the default 250; 1: k = 0
SEGS = (8, 33, 64, None)                 # HERRO_ADAPT_SEG settings the GPU test compares (None: the default 256)
assert PAL == LC.rc(PAL) and len(A28) == 28 and len(A22) == 22


def mutate(seq: bytes, n: int, kind: str, rng) -> bytes:
    """n edits of one kind, spread over the inside of seq"""
    s = list(seq)
    for x in sorted((1 + (i * (len(seq) - 2)) // max(n, 1) for i in range(n)), reverse=True):
        if kind == "sub":
            s[x] = b"ACGT"[(b"ACGT".index(s[x]) + 1 + int(rng.integers(0, 3))) % 4]
        elif kind == "ins":
            s.insert(x, b"ACGT"[int(rng.integers(0, 4))])
        else:
            del s[x]
    return bytes(s)


def _plant(rng, length: int, copy: bytes, at: int) -> bytes:
    """a random read of `length` bases with `copy` at `at` (at < 0: ending at the last base)"""
    at = length - len(copy) if at < 0 else at
    body = LC._rand(rng, length)
    return (body[:at] + copy + body[at + len(copy):])[:max(length, at + len(copy))]


def set_grid():
    rng = np.random.default_rng(101)
    adapters = [LC._rand(rng, m) for m in GRID_ADAPTER_LENGTHS]
    reads = []
    for i, n in enumerate(GRID_LENGTHS):
        a = adapters[i % len(adapters)]
        if n < len(a):
            reads.append(a[:n] if i % 2 else LC.rc(a)[-n:])                 # a text shorter than its pattern: a prefix / a suffix of the other strand
        else:
            reads.append(_plant(rng, n, mutate(a, i % 3, "sub", rng), int(rng.integers(0, n - len(a) + 1))))
    reads.append(b"")                                                       # a read without a base
    return dict(reads=reads, adapters=adapters, calls=[dict(max_err_pm=pm) for pm in GRID_PM])


def set_planted(pm=150):
    rng = np.random.default_rng(102)
    adapters = [A28, A22, PAL]
    reads = []
    for a in adapters:
        k = len(a) * pm // 1000
        for strand in (0, 1):
            p = LC.rc(a) if strand else a
            for at in (0, -1, 20, 50, 250):
                for n_err, kind in [(0, "sub")] + [(e, kd) for e in (k, k + 1) for kd in ("sub", "ins", "del")]:
                    reads.append(_plant(rng, 300, mutate(p, n_err, kind, rng), at))
        body = LC._rand(rng, 300)
        reads.append(body[:100] + a + a + body[100:])                       # back to back
        reads.append(body[:100] + a + b"C" + LC.rc(a) + body[100:])         # one base apart, the other strand
        reads.append(a + a)                                                 # nothing but two copies
    return dict(reads=reads, adapters=adapters, calls=[dict(max_err_pm=pm), dict(max_err_pm=pm, forward_only=True)])


def set_runs():
    rng = np.random.default_rng(103)
    reads = [b"A" * 700, b"AC" * 330, b"A" * 400 + LC._rand(rng, 100), LC._rand(rng, 90) + b"T" * 530, b"CA" * 150 + b"A"]
    return dict(reads=reads, adapters=[b"AAAAAAAA", b"AC" * 16], calls=[dict(max_err_pm=0), dict(max_err_pm=500)])


def set_nonacgt():
    rng = np.random.default_rng(104)
    reads = []
    for i in range(12):
        r = bytearray(_plant(rng, 200 + 17 * i, A22 if i % 2 else LC.rc(A28), 10 * i))
        for x in rng.integers(0, len(r), 1 + i % 4):
            r[int(x)] = b"Nn*-RYK"[int(rng.integers(0, 7))]
        reads.append(bytes(r))
    reads += [b"N" * 70, b"ACGTN" * 20, A28[:14] + b"N" + A28[15:] + b"ACGT" * 9]
    return dict(reads=reads, adapters=[A28, A22], calls=[dict(max_err_pm=250)])


def set_random():
    rng = np.random.default_rng(105)
    reads = [LC._rand(rng, 1500 + 13 * i) for i in range(20)]
    return dict(reads=reads, adapters=[A28, A22, b"ACGTTGCA"], calls=[dict(max_err_pm=150)],
                alone=[dict(adapters=[b"GATTACAG"], max_err_pm=200), dict(adapters=[A28, A22], max_err_pm=150)])


CHIMERA_PM = 150       # k = 4 and 3: random text holds no chance hit (at the default 250 this set has one, 22 bases at 5 errors)


def chimera_parts(head=A28, tail=A22):
    """(clean reads, raw reads, for every raw read the clean reads it is made of): head in front of every read, rc(tail) behind every third,
    clean reads 2 + 3 and 6 + 7 joined through rc(tail) + head"""
    clean = PC.set_d().reads
    assert len(clean) == 10 and len(clean[8]) == 30
    raw, made_of = [], []
    i = 0
    while i < len(clean):
        body, parts = clean[i], [i]
        if i in (2, 6):
            body, parts = clean[i] + LC.rc(tail) + head + clean[i + 1], [i, i + 1]
        raw.append(head + body + (LC.rc(tail) if i % 3 == 0 else b""))
        made_of.append(parts)
        i += len(parts)
    return clean, raw, made_of


def set_chimera():
    clean, raw, _ = chimera_parts()
    return dict(reads=raw, adapters=[A28, A22], calls=[dict(max_err_pm=CHIMERA_PM)])


MAKERS = dict(grid=set_grid, planted=set_planted, runs=set_runs, nonacgt=set_nonacgt, random=set_random, chimera=set_chimera)
_SETS, _REF = {}, {}


def get(name):
    if name not in _SETS:
        _SETS[name] = MAKERS[name]()
    return _SETS[name]


def calls(name):
    """every (adapters, keywords) the set is scanned with"""
    s = get(name)
    out = [(s["adapters"], kw) for kw in s["calls"]]
    for kw in s.get("alone", ()):
        kw = dict(kw)
        out.append((kw.pop("adapters"), kw))
    return out


def reference(name, call: int):
    """adapter_ref.find_adapters of call `call` of the set: computed once, shared and left unchanged"""
    if (name, call) not in _REF:
        adapters, kw = calls(name)[call]
        hits, off = AR.find_adapters([AR.store_codes(r) for r in get(name)["reads"]], adapters, **kw)
        hits.setflags(write=False)
        off.setflags(write=False)
        _REF[name, call] = (hits, off)
    return _REF[name, call]


ALL_CALLS = [(name, i) for name in MAKERS for i in range(len(calls(name)))]


def as_reads(reads):
    """the arrays of Context.set_reads"""
    return PC.Reads(reads)
