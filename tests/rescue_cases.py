"""The read sets of the rescue tests (tests/test_rescue_host.py, tests/test_gpu_rescue.py).  All seeded, a few dozen reads of at most 6 kb; loaded
as pair_cases.load does.

streaks   42 reads built from segments: HSEG, 1 500 bases of which 16 reads carry stretches (above the cut: H), VH, 150 bases that 30 reads carry
          (above rescue_max_occ where that is below 30), the segments U0 .. U9 that two or three reads share (U) and private bases
          (singletons).  The reads put H streaks of at most 63, exactly 64, 65 and more than 129 minimizers between two U, at a read's start, at its
          end and over a whole read, with private bases and with VH inside a streak; one read is shorter than k + w - 1.  CASES runs it under
          several (occ_dist, rescue_max_occ); tests/test_rescue_host.py takes the census that shows each claim is reached.
set_a     40 reads of one 2 000-bp genome with 1 % substitutions: 22 000 of 27 000 minimizers lie above max_occ = 16.
set_b     six loci of 1 500 unique bases around a copy of one 2 500-bp repeat (0.3 % locus-specific differences), five reads per locus, two of them
          inside the repeat only."""
import numpy as np

import lowcomplexity as LC
import pair_cases as PC

KW = dict(k=15, w=5, max_occ=4, min_score=60)      # `streaks`: the fixed cut 4; H is 16 deep
PPM = 100000                                       # ... and occ_frac_ppm: the floor of 10 is the cut
H_DEPTH, VH_DEPTH = 16, 30
X63, X64, X65 = 150, 214, 218                      # stretches of HSEG that give streaks of <= 63, 64 and 65 minimizers (the host test's census)

# name -> (occ_dist, rescue_max_occ)
CASES = {
    "d100": (100, None),
    "d200": (200, None),
    "d1": (1, None),                               # m >= size everywhere
    "d_big": (1 << 20, None),                      # larger than any read: m = 0 everywhere
    "r_below": (100, 8),                           # rescue_max_occ below the depth of H: H is transparent
    "r_equal": (100, H_DEPTH),                     # equal to it: VH is transparent inside its streak
    "r_above": (200, 29),                          # above it and still below VH
}

A_KW = dict(k=15, w=5, max_occ=16, min_score=100)
A_RESCUE = (100, 64)
B_KW = dict(k=15, w=5, max_occ=8, min_score=200)
B_RESCUE = (200, 64)


def _mutate(rng, seq: bytes, p_sub: float) -> bytes:
    x = np.frombuffer(seq, np.uint8).copy()
    for at in np.flatnonzero(rng.random(len(x)) < p_sub):
        x[at] = b"ACGT"[(b"ACGT".index(bytes([x[at]])) + 1 + int(rng.integers(0, 3))) % 4]
    return x.tobytes()


def streaks(seed=77) -> PC.Reads:
    rng = np.random.default_rng(seed)
    H = LC._rand(rng, 1500)
    VH = LC._rand(rng, 150)
    U = [LC._rand(rng, 300) for _ in range(10)]
    priv = lambda n: LC._rand(rng, n)              # noqa: E731
    rd = [
        U[0] + H[:X63] + U[1],                                    # 0: a streak of at most 63
        U[0] + H[:X64] + U[1],                                    # 1: exactly 64
        U[1] + H[:X65] + U[2],                                    # 2: 65
        U[2] + H[:1300] + U[3],                                   # 3: more than 129
        H[:600] + U[3],                                           # 4: a streak at the read's start
        U[4] + H[200:900],                                        # 5: ... and at its end
        H[100:1000],                                              # 6: no U at all
        priv(17),                                                 # 7: shorter than k + w - 1
        U[4] + H[:300] + priv(60) + H[300:600] + U[5],            # 8: singletons inside a streak
        U[5] + H[:300] + VH + H[300:700] + U[6],                  # 9: a hash above rescue_max_occ inside a streak
        U[6] + H[:1500] + U[7],                                   # 10
        U[7] + LC.rc(H[:1500]) + U[8],                            # 11: the other strand
        U[8] + H[:20] + U[9],                                     # 12: a streak too short for one per 200 bases
        U[9] + H[400:1500] + VH,                                  # 13
        VH + H[:1200] + U[0],                                     # 14
        H[700:1500] + VH + U[2],                                  # 15
    ]
    assert len(rd) == H_DEPTH
    rd += [VH + priv(200 + 10 * i) if i % 2 else priv(150 + 10 * i) + VH + priv(100) for i in range(VH_DEPTH - 4)]
    assert sum(VH in r for r in rd) == VH_DEPTH
    return PC.Reads(rd)


def set_a(seed=3) -> PC.Reads:
    rng = np.random.default_rng(seed)
    g = LC._rand(rng, 2000)
    return PC.Reads([_mutate(rng, g, 0.01) for _ in range(40)])


B_SPANS = ((0, 2600), (400, 4000), (1900, 4000), (900, 2900), (1200, 3100))     # the last two lie inside the repeat (750 .. 3250)


def set_b(seed=5) -> PC.Reads:
    rng = np.random.default_rng(seed)
    rep = LC._rand(rng, 2500)
    rd = []
    for _ in range(6):
        u = LC._rand(rng, 1500)
        locus = u[:750] + _mutate(rng, rep, 0.003) + u[750:]
        rd += [locus[a:b] for a, b in B_SPANS]
    return PC.Reads(rd)


def b_repeat_only() -> np.ndarray:
    """set_b's reads that lie inside the repeat only"""
    return np.array([5 * i + j for i in range(6) for j in (3, 4)])


SETS = dict(streaks=streaks, set_a=set_a, set_b=set_b)
_CACHE = {}


def get(name):
    """(the set as pair_cases.load takes it, its 2-bit codes), made once"""
    if name not in _CACHE:
        import overlap_ref as R
        rs = SETS[name]()
        _CACHE[name] = (rs, [R.store_codes(r) for r in rs.reads])
    return _CACHE[name]


def sketch(name, k=15, w=5):
    """overlap_ref.sketch_store of a set and its read lengths, made once: (h, rid, pos, st, lens)"""
    key = (name, "sketch", k, w)
    if key not in _CACHE:
        import overlap_ref as R
        codes = get(name)[1]
        _CACHE[key] = R.sketch_store(codes, k, w) + (np.array([len(c) for c in codes], np.int64),)
    return _CACHE[key]


def streak_census(name, cut, occ_dist, rescue_max_occ=None, k=15, w=5):
    """every streak of a set under the reference: dicts of read, size, m, ps, pe, len, inner (the occ of everything between its first and its last
    member, transparent minimizers included), tied (0 < m < size and more members share the threshold occ than are taken at it)"""
    import rescue_ref as RR
    h, rid, pos, st, lens = sketch(name, k, w)
    occ = RR.occurrences(h)
    rmax = RR.check(occ_dist, rescue_max_occ)[1]
    b = np.searchsorted(rid, np.arange(len(lens) + 1))
    out = []
    for r in range(len(lens)):
        o, p = occ[b[r]:b[r + 1]], pos[b[r]:b[r + 1]]
        for idx, ps, pe in RR.streaks(o, p, int(lens[r]), cut, rmax):
            m = RR.streak_quota(ps, pe, occ_dist)
            tied = False
            if 0 < m < len(idx):
                so = np.sort(o[idx])
                tied = int((so == so[m - 1]).sum()) > m - int((so < so[m - 1]).sum())
            out.append(dict(read=r, size=len(idx), m=m, ps=ps, pe=pe, len=int(lens[r]), inner=o[idx[0]:idx[-1] + 1], tied=tied,
                            n_u=int(((o >= 2) & (o <= cut)).sum())))
    return out


def reference(name, occ_dist, rescue_max_occ=None, occ_frac_ppm=0, **kw):
    """rescue_ref.find_overlaps_rescue on a set, computed once per (set, parameters): ((rids, rows, aln_off, scores), stats)"""
    import rescue_ref as RR
    key = (name, occ_dist, rescue_max_occ, occ_frac_ppm, tuple(sorted(kw.items())))
    if key not in _CACHE:
        st = {}
        _CACHE[key] = (RR.find_overlaps_rescue(get(name)[1], occ_dist, rescue_max_occ, occ_frac_ppm, stats=st, **kw), st)
    return _CACHE[key]
