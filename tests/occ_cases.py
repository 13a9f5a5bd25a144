"""The read sets of the fraction-cut tests (tests/test_occ_host.py, tests/test_gpu_occ.py).  All seeded and small; loaded as pair_cases.load does.

deep       200 reads of one 400-bp genome (0.5 % substitutions, every third read reversed and complemented): every true minimizer occurs ~190
           times, so the fixed cut of 128 leaves nothing and every one of the 19 900 pairs needs a cut taken from the index.
depth33    synth.generate(1, 2048, 32): 33 reads of one 2-kb genome; the index's own cut is far below 128.
low        lowcomplexity.working_set(): 24 low-complexity reads.
four       four reads of one genome: no run is long, the floor of 10 is the cut.
ac_mixed   depth33's reads and one (AC)n read of 140 kb, whose ~70 000 minimizers are one hash: the last bin of the census.
ac_only    two such reads: one run in the last bin, the cut is 65 534 and nothing is used.
no_minimizers   reads shorter than k + w - 1."""
import numpy as np

import lowcomplexity as LC
import pair_cases as PC

PPM = 5000                                        # the reference's -f0.005
DEEP_KW = (dict(k=15, w=5, min_score=60), dict(k=25, w=17, min_score=60))
DEEP_PAIRS = 200 * 199 // 2
AC_LEN = 140_000


def deep(n=200, L=400, p_sub=0.005, seed=43) -> PC.Reads:
    rng = np.random.default_rng(seed)
    g = np.frombuffer(LC._rand(rng, L), np.uint8)
    out = []
    for r in range(n):
        x = g.copy()
        for at in np.flatnonzero(rng.random(L) < p_sub):
            x[at] = b"ACGT"[(b"ACGT".index(bytes([x[at]])) + 1 + int(rng.integers(0, 3))) % 4]
        out.append(LC.rc(x.tobytes()) if r % 3 == 2 else x.tobytes())
    return PC.Reads(out)


def deep_core(n=200, n_core=8) -> np.ndarray:
    """eight targets spread over the set, both strands among them"""
    m = np.zeros(n, np.uint8)
    m[np.arange(n_core) * (n // n_core) + 2] = 1
    return m


def depth33(seed=31):
    from herro_amd import synth
    sb = synth.generate(1, 2048, 32, seed=seed)
    assert sb.n_reads == 33
    return sb


def reads_of(sb) -> list:
    """the ASCII reads of a synth batch"""
    off = np.asarray(sb.off).astype(np.int64)
    return [bytes(np.asarray(sb.seq[off[r]:off[r + 1]])) for r in range(len(off) - 1)]


def low():
    return LC.working_set()


def four(seed=43) -> PC.Reads:
    rng = np.random.default_rng(seed)
    rd, _, _ = LC.reads(rng, LC._rand(rng, 3000), 4, min_len=2000, max_len=2600, p_rep=0.0)
    return PC.Reads(rd)


def ac_read() -> bytes:
    return b"AC" * (AC_LEN // 2)


def ac_mixed() -> PC.Reads:
    rd = reads_of(depth33())
    return PC.Reads(rd[:5] + [ac_read()] + rd[5:])


def ac_only() -> PC.Reads:
    return PC.Reads([ac_read(), ac_read()])


def no_minimizers() -> PC.Reads:
    rng = np.random.default_rng(44)
    return PC.Reads([LC._rand(rng, n) for n in (5, 18, 30, 40)])          # k + w - 1 = 41 at the defaults


SETS = dict(deep=deep, depth33=depth33, low=low, four=four, ac_mixed=ac_mixed, ac_only=ac_only, no_minimizers=no_minimizers)
_CACHE = {}


def get(name):
    """(the set as pair_cases.load takes it, its 2-bit codes), made once"""
    if name not in _CACHE:
        import overlap_ref as R
        rs = SETS[name]()
        _CACHE[name] = (rs, [R.store_codes(r) for r in (rs.reads if hasattr(rs, "reads") else reads_of(rs))])
    return _CACHE[name]


def reference(name, ppm, **kw):
    """occ_ref.find_overlaps on a set, computed once per (set, parameters): ((rids, rows, aln_off, scores), cut, stats)"""
    import occ_ref as OR
    key = (name, ppm, tuple(sorted(kw.items())))
    if key not in _CACHE:
        st = {}
        res, cut = OR.find_overlaps(get(name)[1], ppm, stats=st, **kw)
        _CACHE[key] = (res, cut, st)
    return _CACHE[key]
