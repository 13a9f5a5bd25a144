"""Seeded low-complexity reads for the front end's tests (tests/test_lowcomplexity_host.py, tests/test_gpu_lowcomplexity.py): genomes of
homopolymers, short tandem repeats and tandem copies between random stretches, reads of them with substitutions, insertions, deletions
and length errors inside repeats, the lopsided alignment grid, the query that equals its own reverse complement, and the census of
the events the kernels' tie and edge rules govern.  numpy only; the census uses nothing but the reference modules' public functions."""
from __future__ import annotations

import dataclasses

import numpy as np

import align_ref as A
import extend_ref as E
import overlap_ref as R

COMP = bytes.maketrans(b"ACGTN", b"TGCAN")
SELF_RC_UNITS = (b"AT", b"CG", b"ACGT")                   # units that equal their own reverse complement
GRID_LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 300, 600)  # the band's half width, its width, and past it
GRID_KINDS = ("one_gap", "unrelated", "homopolymer", "repeat3")


def rc(seq: bytes) -> bytes:
    return seq.translate(COMP)[::-1]


def _rand(rng, n) -> bytes:
    return bytes(b"ACGT"[x] for x in rng.integers(0, 4, n))


# ---- the genome -----------------------------------------------------------------------------------------------------------------------
def genome(rng, L: int, weights=(0.40, 0.20, 0.30, 0.10)) -> bytes:
    """segments drawn by weight: a uniform stretch of 5-40 bases, a homopolymer of 3 + geometric bases, a 2-6-bp unit 3-15 times
    (every fourth one of SELF_RC_UNITS), a 30-80-bp unit 2-3 times; cut to L bases"""
    segs, n = [], 0
    while n < L:
        kind = int(rng.choice(4, p=weights))
        if kind == 0:
            s = _rand(rng, int(rng.integers(5, 41)))
        elif kind == 1:
            s = _rand(rng, 1) * (3 + int(rng.geometric(0.25)))
        elif kind == 2:
            unit = SELF_RC_UNITS[int(rng.integers(0, 3))] if rng.random() < 0.25 else _rand(rng, int(rng.integers(2, 7)))
            s = unit * int(rng.integers(3, 16))
        else:
            s = _rand(rng, int(rng.integers(30, 81))) * int(rng.integers(2, 4))
        segs.append(s)
        n += len(s)
    return b"".join(segs)[:L]


# ---- reads ------------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class ReadSet:
    reads: list            # ASCII, as stored (a reverse-strand read is written reversed and complemented)
    truth: list            # per read (group, genome start, genome end, strand)
    gpos: list             # per read int64 [len]: the genome position every stored base came from
    seq: np.ndarray        # u8: Context.set_reads' three arrays
    qual: np.ndarray
    off: np.ndarray

    def codes(self):
        return [R.store_codes(r) for r in self.reads]


def reads(rng, g: bytes, n: int, min_len=2500, max_len=3500, p_sub=0.01, p_ins=0.01, p_del=0.01, p_rep=0.05, n_bases=0, group=0):
    """n reads of sub-spans of g -> ([ASCII], [(group, start, end, strand)], [gpos]).  A base equal to its predecessor is dropped or
    doubled with p_rep (the length errors of repeats); every third read is reversed and complemented; n_bases bases become N."""
    out, truth, maps = [], [], []
    for r in range(n):
        ln = int(rng.integers(min_len, min(max_len, len(g)) + 1))
        s = int(rng.integers(0, len(g) - ln + 1))
        seq, gp = bytearray(), []
        for x in range(s, s + ln):
            b = g[x]
            if x > s and b == g[x - 1]:
                u = rng.random()
                if u < p_rep / 2:
                    continue
                if u < p_rep:
                    seq.append(b)
                    gp.append(x)
            u = rng.random()
            if u < p_del:
                continue
            if u < p_del + p_ins:
                seq.append(b"ACGT"[int(rng.integers(0, 4))])
                gp.append(x)
            elif u < p_del + p_ins + p_sub:
                seq.append(b"ACGT"[(b"ACGT".index(b) + 1 + int(rng.integers(0, 3))) % 4])
                gp.append(x)
                continue
            seq.append(b)
            gp.append(x)
        for at in rng.integers(0, len(seq), n_bases):
            seq[int(at)] = ord("N")
        seq, gp = bytes(seq), np.array(gp, np.int64)
        strand = int(r % 3 == 2)
        if strand:
            seq, gp = rc(seq), gp[::-1].copy()
        out.append(seq)
        truth.append((group, s, s + ln, strand))
        maps.append(gp)
    return out, truth, maps


def read_set(rng, rd, truth, maps) -> ReadSet:
    seq = np.frombuffer(b"".join(rd), np.uint8).copy()
    off = np.concatenate([[0], np.cumsum([len(r) for r in rd])]).astype(np.uint64)
    qual = (33 + rng.integers(2, 50, len(seq))).astype(np.uint8)
    return ReadSet(list(rd), list(truth), list(maps), seq, qual, off)


def working_set(seed=7, n_genomes=3, L=6000, n_reads=8, n_bases=0, **kw) -> ReadSet:
    """three genomes of 6 kb, eight reads each of 2.5-3.5 kb"""
    rng = np.random.default_rng(seed)
    rd, truth, maps = [], [], []
    for gi in range(n_genomes):
        a, b, c = reads(rng, genome(rng, L), n_reads, n_bases=n_bases, group=gi, **kw)
        rd += a; truth += b; maps += c
    return read_set(rng, rd, truth, maps)


def short_and_n_reads(seed=8):
    """reads around and below the k + w - 1 of the sketch tests (9 .. 93 bases) and three reads with N: ([ASCII], truth, gpos)"""
    rng = np.random.default_rng(seed)
    g = genome(rng, 2000)
    rd, truth, maps = [], [], []
    for ln in (5, 8, 9, 10, 22, 23, 24, 40, 41, 42, 92, 93, 94):
        a, b, c = reads(rng, g, 1, min_len=ln, max_len=ln, p_rep=0.0, p_sub=0.0, p_ins=0.0, p_del=0.0, group=9)
        rd += a; truth += b; maps += c
    a, b, c = reads(rng, g, 3, min_len=600, max_len=900, n_bases=4, group=9)
    return rd + a, truth + b, maps + c


def true_pairs(rs: ReadSet, min_overlap=1000):
    """{(t, q) with t < q: (strand, (t0, t1), (q0, q1))}: reads of one genome sharing >= min_overlap of it, the shared stretch as the
    stored reads' half-open spans"""
    out = {}
    for t in range(len(rs.reads)):
        for q in range(t + 1, len(rs.reads)):
            (ga, sa, ea, ra), (gb, sb, eb, rb) = rs.truth[t], rs.truth[q]
            lo, hi = max(sa, sb), min(ea, eb)
            if ga != gb or hi - lo < min_overlap:
                continue
            spans = []
            for x in (t, q):
                at = np.flatnonzero((rs.gpos[x] >= lo) & (rs.gpos[x] < hi))
                spans.append((int(at[0]), int(at[-1]) + 1))
            out[(t, q)] = (ra ^ rb, spans[0], spans[1])
    return out


# ---- the lopsided grid and the palindromic pair ---------------------------------------------------------------------------------------
def lopsided_grid(rng):
    """400 records: query length n x target length m over GRID_LENGTHS, in GRID_KINDS — the longer read is the shorter with one gap of
    |n - m| bases, two unrelated reads, one homopolymer, one 3-bp repeat.  Every record has its own two reads and spans both of them;
    every second record is a reverse-strand one.  Returns ([ASCII reads], rows u32 [400, 9], kinds [400])."""
    rd, rows, kinds = [], [], []
    for kind in GRID_KINDS:
        for n in GRID_LENGTHS:
            for m in GRID_LENGTHS:
                if kind == "one_gap":
                    long_ = _rand(rng, max(n, m))
                    at = int(rng.integers(0, min(n, m) + 1))
                    short = long_[:at] + long_[at + abs(n - m):]
                    q, t = (long_, short) if n >= m else (short, long_)
                elif kind == "unrelated":
                    q, t = _rand(rng, n), _rand(rng, m)
                elif kind == "homopolymer":
                    b = _rand(rng, 1)
                    q, t = b * n, b * m
                else:
                    u = b"ACG"[int(rng.integers(0, 3)):][:1] + _rand(rng, 1) + b"T"
                    q, t = (u * n)[:n], (u * m)[:m]
                strand = len(rows) & 1
                rows.append([len(rd) + 1, n, 0, n, strand, len(rd), m, 0, m])
                rd += [t, rc(q) if strand else q]
                kinds.append(kind)
    return rd, np.array(rows, np.uint32), kinds


def palindromic_pair(rng, x_len=1500, flank=300):
    """[T, Q] with Q = X + revcomp(X), its own reverse complement, and T = flank + Q + flank"""
    x = _rand(rng, x_len)
    q = x + rc(x)
    assert q == rc(q)
    return [_rand(rng, flank) + q + _rand(rng, flank), q]


# ---- the census -------------------------------------------------------------------------------------------------------------------------
def census_sketch(codes, k: int, w: int) -> dict:
    """minimizers; the ones whose hash their read holds more than once (`repeated`); hash runs of the index with three or more reads,
    one of them more than once (`runs3_repeated`); k-mers equal to their reverse complement (`palindromic`)"""
    h, rid, pos, st = R.sketch_store(codes, k, w)
    key = np.stack([rid.astype(np.uint64), h], 1)
    _, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    repeated = int((cnt[inv.ravel()] > 1).sum())
    runs3 = 0
    o = np.argsort(h, kind="stable")
    hs, rs = h[o], rid[o]
    b = np.flatnonzero(np.concatenate([[True], hs[1:] != hs[:-1], [True]])) if len(hs) else np.zeros(1, np.int64)
    for s, e in zip(b[:-1], b[1:]):
        if e - s >= 4:
            r, c = np.unique(rs[s:e], return_counts=True)
            runs3 += int(len(r) >= 3 and c.max() >= 2)
    pal = 0
    for c in codes:
        f, r = R.kmers(c, k)
        pal += int((f == r).sum())
    return dict(minimizers=len(h), repeated=repeated, runs3_repeated=runs3, palindromic=pal)


def cut_hashes_in_true_overlaps(rs: ReadSet, k: int, w: int, max_occ: int) -> int:
    """hashes dropped by the frequency cut that both reads of a true pair hold inside their shared stretch"""
    h, rid, pos, st = R.sketch_store(rs.codes(), k, w)
    u, cnt = np.unique(h, return_counts=True)
    pairs = true_pairs(rs)
    n = 0
    for x in u[cnt > max_occ]:
        at = np.flatnonzero(h == x)
        where = {}
        for a in at:
            where.setdefault(int(rid[a]), []).append(int(pos[a]))
        n += int(any(t in where and q in where and any(t0 <= p < t1 for p in where[t]) and any(q0 <= p < q1 for p in where[q])
                     for (t, q), (_, (t0, t1), (q0, q1)) in pairs.items()))
    return n


def chains(codes, **kw):
    """the chains find_overlaps keeps before it picks a strand: [(t, q, rel, score, ts, te, qs, qe, count)] in ascending (t, q, rel),
    from the reference's sketch_store, anchors and chain_many"""
    P = R.params(**kw)
    k = P["k"]
    lens = np.array([len(c) for c in codes], np.int64)
    a = R.anchors(*R.sketch_store(codes, k, P["w"]), lens, k, P["max_occ"])
    if not len(a):
        return []
    b = np.flatnonzero(np.concatenate([[True], (a[1:, :3] != a[:-1, :3]).any(axis=1), [True]]))
    spans = [(s, e) for s, e in zip(b[:-1], b[1:]) if e - s >= P["min_anchors"]]
    got = R.chain_many([a[s:e, 3] for s, e in spans], [a[s:e, 4] for s, e in spans], k, P["bandwidth"], P["max_gap"])
    out = []
    for (s, e), (sc, s0, e0, cnt) in zip(spans, got):
        if sc < P["min_score"] or cnt < P["min_anchors"]:
            continue
        t, q, rel = (int(x) for x in a[s, :3])
        ts, te = int(a[s + s0, 3]) - k + 1, int(a[s + e0, 3]) + 1
        qs, qe = int(a[s + s0, 4]) - k + 1, int(a[s + e0, 4]) + 1
        if rel:
            qs, qe = int(lens[q]) - qe, int(lens[q]) - qs
        out.append((t, q, rel, sc, ts, te, qs, qe, cnt))
    return out


def pairs_chained_on_both_strands(codes, **kw) -> int:
    seen = {}
    for c in chains(codes, **kw):
        seen.setdefault(c[:2], set()).add(c[2])
    return sum(1 for v in seen.values() if len(v) == 2)


def grid_net_indel_above(rows, d=64) -> int:
    rows = np.asarray(rows, np.int64)
    return int((np.abs((rows[:, 3] - rows[:, 2]) - (rows[:, 8] - rows[:, 7])) > d).sum())


def whole_matrix(T, Q):
    """H of every cell (i over Q, j over T) of the extension's recurrence from its definition, python integers: [n + 1][m + 1]"""
    T, Q = [int(x) for x in T], [int(x) for x in Q]
    n, m = len(Q), len(T)
    ninf = -(1 << 40)
    oe, e = A.GAP_OPEN + A.GAP_EXT, A.GAP_EXT
    H = [[ninf] * (m + 1) for _ in range(n + 1)]
    I = [[ninf] * (m + 1) for _ in range(n + 1)]
    H[0][0] = 0
    for i in range(n + 1):
        d = ninf                                      # D runs along the row
        for j in range(m + 1):
            if i == 0 and j == 0:
                continue
            best = ninf
            if i > 0:
                I[i][j] = best = max(H[i - 1][j] - oe, I[i - 1][j] - e)
            if j > 0:
                d = max(H[i][j - 1] - oe, d - e)
                best = max(best, d)
            if i > 0 and j > 0:
                best = max(best, H[i - 1][j - 1] + (A.MATCH if Q[i - 1] == T[j - 1] else A.MISMATCH))
            H[i][j] = best
    return H


def best_cell(H):
    """(score, i, j) of the extension's best-cell rule on a whole matrix: the greatest H over i, j >= 1 if above 0, the first on the
    earliest anti-diagonal, the smallest i on it; and how many cells hold that maximum"""
    n, m = len(H) - 1, len(H[0]) - 1
    top = max((H[i][j] for i in range(1, n + 1) for j in range(1, m + 1)), default=0)
    if top <= 0:
        return (0, 0, 0), 0
    at = [(i + j, i, j) for i in range(1, n + 1) for j in range(1, m + 1) if H[i][j] == top]
    d, i, j = min(at)
    return (top, i, j), len(at)


def short_sides(codes, rows, cap=63):
    """the extension sides (T', Q') of rows as max_ext = cap cuts them, the ones with two flanks of 1 .. cap bases"""
    out = []
    for row in rows:
        for T, Q in E.side_seqs(codes, row, cap):
            if len(T) and len(Q):
                out.append((T, Q))
    return out


def tied_extension_sides(sides) -> int:
    """sides where two or more cells of the whole matrix share the maximum H"""
    return sum(1 for T, Q in sides if best_cell(whole_matrix(T, Q))[1] >= 2)


def shrunk_rows(rng, rs: ReadSet, per_pair=4, lo=1, hi=63):
    """per_pair records per true pair: the shared stretch shrunk by lo .. hi bases at each of its four ends, so that the flanks are
    related low-complexity sequence; u32 [n, 9]"""
    rows = []
    for (t, q), (strand, (t0, t1), (q0, q1)) in true_pairs(rs).items():
        for _ in range(per_pair):
            a, b, c, d = (int(x) for x in rng.integers(lo, hi + 1, 4))
            rows.append([q, len(rs.reads[q]), q0 + a, q1 - b, strand, t, len(rs.reads[t]), t0 + c, t1 - d])
    return np.array(rows, np.uint32)


def true_rows(rs: ReadSet):
    """one record per true pair over the shared stretch itself; u32 [n, 9]"""
    return np.array([[q, len(rs.reads[q]), q0, q1, strand, t, len(rs.reads[t]), t0, t1]
                     for (t, q), (strand, (t0, t1), (q0, q1)) in true_pairs(rs).items()], np.uint32)


def hand_flank_batch(rng, lengths, span=60):
    """([ASCII reads], rows u32 [n, 9]): a random span of `span` bases between flanks of pure homopolymer or of a 2-3-bp repeat, every
    pair of `lengths` as (target, query) flank lengths on the right and, rotated, on the left; both strands.  The two reads' flanks
    are the same repeat, so every cell of the diagonal and its neighbours is a candidate for the best cell."""
    rd, rows = [], []
    combos = [(a, b) for a in lengths for b in lengths]
    for x, (a, b) in enumerate(combos):
        la, lb = combos[(x * 7 + 3) % len(combos)]
        unit = (_rand(rng, 1), b"AC", b"CG", b"GAT", b"AT")[x % 5]
        core = _rand(rng, span)
        t = (unit * (la + 3))[:la] + core + (unit * (a + 3))[:a]
        q = (unit * (lb + 3))[:lb] + core + (unit * (b + 3))[:b]
        strand = x & 1
        qs = lb
        if strand:
            q = rc(q)
            qs = len(q) - lb - span
        rows.append([len(rd) + 1, len(q), qs, qs + span, strand, len(rd), len(t), la, la + span])
        rd += [t, q]
    return rd, np.array(rows, np.uint32)


def gapped_flank_batch(rng, n=60, span=60):
    """([ASCII reads], rows u32 [n, 9]): behind a common span of `span` bases one read goes on with X (150-600 bases: random, low-complexity
    or a 3-bp repeat by turns) and the other with X and 65-195 further bases put into its first 120 — a gap wider than half the band that
    costs less than the default z-drop, so the band follows it along its bottom or top cell; the longer flank is the target's on every
    second record; every third record is a reverse-strand one.  The rows hold the span; `whole_rows` makes them the whole reads."""
    rd, rows = [], []
    for x in range(n):
        L, g, at = int(rng.integers(150, 601)), int(rng.integers(65, 196)), int(rng.integers(5, 121))
        kind = x % 3
        X = _rand(rng, L) if kind == 0 else genome(rng, L) if kind == 1 else (_rand(rng, 2) + b"T") * (L // 3 + 1)
        X = X[:L]
        G = _rand(rng, g) if kind != 2 else (X[:3] * g)[:g]
        longer = X[:at] + G + X[at:]
        core = _rand(rng, span)
        t, q = (core + longer, core + X) if x & 1 else (core + X, core + longer)
        strand = int(x % 3 == 2)
        qs = 0
        if strand:
            q = rc(q)
            qs = len(q) - span
        rows.append([len(rd) + 1, len(q), qs, qs + span, strand, len(rd), len(t), 0, span])
        rd += [t, q]
    return rd, np.array(rows, np.uint32)


def whole_rows(rows):
    """the records of rows over their two whole reads"""
    out = np.asarray(rows, np.uint32).copy()
    out[:, 2], out[:, 3], out[:, 7], out[:, 8] = 0, out[:, 1], 0, out[:, 6]
    return out


def evaluate(rs: ReadSet, pairs: dict):
    """(missed, wrong strand, cross-group, least coverage of the true target span) of find_overlaps' stats["pairs"] against the truth"""
    truth = true_pairs(rs)
    cross = sum(1 for (t, q) in pairs if rs.truth[t][0] != rs.truth[q][0])
    miss = wrong = 0
    cov = []
    for (t, q), (strand, (t0, t1), _) in truth.items():
        r = pairs.get((t, q))
        if r is None:
            miss += 1
            continue
        wrong += int(r[1] != strand)
        cov.append(max(0, min(t1, r[3]) - max(t0, r[2])) / (t1 - t0))
    return miss, wrong, cross, min(cov) if cov else 0.0


def fix_cigar_shifted(cigar, target, query) -> int:
    """the bases the left-shift loop of align_ref.fix_cigar moves: a copy of that loop with a counter"""
    cig = [list(op) for op in cigar]
    tpos = qpos = moved = 0
    for i in range(len(cig)):
        ln, t = cig[i]
        if t == A.M_:
            tpos += ln
            qpos += ln
            continue
        if 0 < i < len(cig) - 1 and cig[i - 1][1] == A.M_ and cig[i + 1][1] == A.M_:
            prev_len = cig[i - 1][0]
            l = 0
            if t == A.I_:
                while l < prev_len and query[qpos - 1 - l] == query[qpos + ln - 1 - l]:
                    l += 1
            else:
                while l < prev_len and target[tpos - 1 - l] == target[tpos + ln - 1 - l]:
                    l += 1
            if l > 0:
                cig[i - 1][0] -= l
                cig[i + 1][0] += l
                tpos -= l
                qpos -= l
                moved += l
        if t == A.I_:
            qpos += ln
        else:
            tpos += ln
    return moved
