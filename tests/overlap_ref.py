"""numpy restatement of the overlap finder herro_find_overlaps runs on the GPU (csrc/overlap_dev.hip).

This file is the reference the kernels are held to, bit for bit.  All integer:

  sketch   over the read store's 2-bit codes: per k-mer f (first base most significant), r (reverse complement), canonical
           min(f, r), strand r < f, f == r never selected; hash = minimap2's invertible hash64 on 2k bits; every k-mer whose
           hash equals the minimum of a window of w consecutive k-mers is a minimizer (ties select all).
  index    all minimizers grouped by hash; a hash with more than max_occ occurrences in the store is dropped.
  anchors  every two occurrences of a hash in reads t < q: rel = s_t ^ s_q, tpos = pos_t, qpos = pos_q or qlen - pos_q + k - 2.
  chain    per (t, q, rel), anchors sorted by (tpos, qpos): f[i] = max(k, max_j f[j] + min(k, dt, dq) - cost(|dt - dq|)) over the
           `lookback` (64) nearest predecessors with 0 < dt, dq <= max_gap and |dt - dq| <= bandwidth; the nearest wins ties;
           the chain ends at argmax f (smallest i) and is kept with f >= min_score and >= min_anchors anchors.
  overlap  the anchor span; one per pair (the better strand, 0 on a tie); two records per pair (the dual), grouped by target.

The sketch is vectorised over the read and the chain over its predecessors (one numpy step per anchor)."""
from __future__ import annotations

import numpy as np

from align_ref import store_codes  # noqa: F401  (the store's codes, the non-ACGT quirk included)

INF = np.uint64(0xFFFFFFFFFFFFFFFF)
DEFAULTS = dict(k=25, w=17, max_occ=128, bandwidth=150, max_gap=5000, min_score=2500, min_anchors=3)
LOOKBACK = 64


def params(**kw) -> dict:
    """the specification's parameters: 0 / missing = default; ValueError where the library returns HERRO_E_INVALID"""
    p = dict(DEFAULTS)
    for name, v in kw.items():
        if name not in p:
            raise TypeError(name)
        if v:
            p[name] = int(v)
    if not (5 <= p["k"] <= 31 and 1 <= p["w"] <= 64):
        raise ValueError("5 <= k <= 31 and 1 <= w <= 64")
    return p


def hash64(x, k: int):
    m = np.uint64((1 << (2 * k)) - 1)
    x = np.asarray(x, np.uint64)
    u = np.uint64
    with np.errstate(over="ignore"):
        x = (~x + (x << u(21))) & m
        x = x ^ (x >> u(24))
        x = (x + (x << u(3)) + (x << u(8))) & m
        x = x ^ (x >> u(14))
        x = (x + (x << u(2)) + (x << u(4))) & m
        x = x ^ (x >> u(28))
        x = (x + (x << u(31))) & m
    return x


def hash64_inverse(y: int, k: int) -> int:
    """the inverse of hash64 on 2k bits (python integers): every step of the mix is undone in turn"""
    bits = 2 * k
    m = (1 << bits) - 1

    def unxorshift(v, s):
        out = v
        for _ in range(bits // s + 1):
            out = v ^ (out >> s)
        return out

    def undo_mul(v, mult):
        return (v * pow(mult, -1, 1 << bits)) & m
    y = undo_mul(y, 1 + (1 << 31))
    y = unxorshift(y, 28)
    y = undo_mul(y, 21)
    y = unxorshift(y, 14)
    y = undo_mul(y, 265)
    y = unxorshift(y, 24)
    # x -> ~x + (x << 21) = (2^21 - 1) x - 1
    return undo_mul((y + 1) & m, (1 << 21) - 1)


def kmers(codes: np.ndarray, k: int):
    """(f, r) of every k-mer of a read (uint64)"""
    c = np.asarray(codes).astype(np.uint64)
    nk = len(c) - k + 1
    if nk <= 0:
        return np.zeros(0, np.uint64), np.zeros(0, np.uint64)
    f = np.zeros(nk, np.uint64)
    r = np.zeros(nk, np.uint64)
    for i in range(k):
        f |= c[i:i + nk] << np.uint64(2 * (k - 1 - i))
        r |= (np.uint64(3) - c[i:i + nk]) << np.uint64(2 * i)
    return f, r


def sketch(codes: np.ndarray, k: int, w: int):
    """minimizers of one read: (hash u64, pos i64 = last base of the k-mer, strand u8), ascending pos"""
    nk = len(codes) - k + 1
    if nk < w:
        return np.zeros(0, np.uint64), np.zeros(0, np.int64), np.zeros(0, np.uint8)
    f, r = kmers(codes, k)
    h = np.where(f == r, INF, hash64(np.minimum(f, r), k))
    st = (r < f).astype(np.uint8)
    nw = nk - w + 1
    wm = np.lib.stride_tricks.sliding_window_view(h, w).min(axis=1)
    sel = np.zeros(nk, bool)
    for o in range(w):
        sel[o:o + nw] |= (h[o:o + nw] == wm) & (wm != INF)
    idx = np.flatnonzero(sel)
    return h[idx], idx + (k - 1), st[idx]


def sketch_store(read_codes, k: int, w: int):
    """minimizers of every read, sorted by (rid, pos): hash u64, rid i64, pos i64, strand u8"""
    hs, rs, ps, ss = [np.zeros(0, np.uint64)], [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.uint8)]
    for i, c in enumerate(read_codes):
        h, p, s = sketch(c, k, w)
        hs.append(h); ps.append(p); ss.append(s); rs.append(np.full(len(h), i, np.int64))
    return np.concatenate(hs), np.concatenate(rs), np.concatenate(ps), np.concatenate(ss)


def anchors(h, rid, pos, st, lens, k: int, max_occ: int):
    """(t, q, rel, tpos, qpos) int64 arrays sorted by that tuple"""
    o = np.lexsort((pos, rid, h))
    h, rid, pos, st = h[o], rid[o], pos[o], st[o].astype(np.int64)
    n = len(h)
    out = [np.zeros((0, 5), np.int64)]
    if n:
        b = np.flatnonzero(np.concatenate([[True], h[1:] != h[:-1], [True]]))
        start, cnt = b[:-1], np.diff(b)
        for c in np.unique(cnt):
            if c < 2 or c > max_occ:
                continue
            S = start[cnt == c]
            ia, ib = np.triu_indices(int(c), 1)
            for s0 in range(0, len(S), max(1, (1 << 22) // len(ia))):
                Sx = S[s0:s0 + max(1, (1 << 22) // len(ia))]
                x = (Sx[:, None] + ia[None, :]).ravel()
                y = (Sx[:, None] + ib[None, :]).ravel()
                keep = rid[x] != rid[y]              # sorted by rid inside a run: rid[x] < rid[y] where they differ
                x, y = x[keep], y[keep]
                rel = st[x] ^ st[y]
                qpos = np.where(rel == 0, pos[y], lens[rid[y]] - pos[y] + k - 2)
                out.append(np.stack([rid[x], rid[y], rel, pos[x], qpos], axis=1))
    a = np.concatenate(out)
    o = np.lexsort((a[:, 4], a[:, 3], a[:, 2], a[:, 1], a[:, 0]))
    return a[o]


def _ilog2(x):
    """floor(log2(x)) of positive int64 (exact: no floating point)"""
    x = np.asarray(x, np.int64)
    r = np.zeros(x.shape, np.int64)
    for s in (32, 16, 8, 4, 2, 1):
        big = x >= (np.int64(1) << np.int64(s))
        r += np.where(big, s, 0)
        x = np.where(big, x >> np.int64(s), x)
    return r


def chain(tp, qp, k: int, bandwidth: int, max_gap: int, lookback: int | None = LOOKBACK):
    """(score, first anchor, last anchor, anchors in the chain) of the best chain of one (t, q, rel) group"""
    tp = np.asarray(tp, np.int64)
    qp = np.asarray(qp, np.int64)
    n = len(tp)
    f = np.zeros(n, np.int64)
    p = np.full(n, -1, np.int64)
    H = n if lookback is None else lookback
    for i in range(n):
        lo = max(0, i - H)
        best, bp = k, -1
        if i > lo:
            dt = tp[i] - tp[lo:i][::-1]            # nearest predecessor first
            dq = qp[i] - qp[lo:i][::-1]
            dd = np.abs(dt - dq)
            ok = (dt > 0) & (dq > 0) & (dt <= max_gap) & (dq <= max_gap) & (dd <= bandwidth)
            sc = f[lo:i][::-1] + np.minimum(np.minimum(dt, dq), k) - ((dd * k) >> 6) - (_ilog2(dd + 1) >> 1)
            sc = np.where(ok, sc, np.iinfo(np.int64).min)
            j = int(np.argmax(sc))                  # first maximum = the nearest
            if sc[j] > best:
                best, bp = int(sc[j]), i - 1 - j
        f[i], p[i] = best, bp
    e = int(np.argmax(f))
    s, cnt = e, 1
    while p[s] >= 0:
        s = int(p[s])
        cnt += 1
    return int(f[e]), s, e, cnt


def chain_many(tps, qps, k: int, bandwidth: int, max_gap: int, lookback: int = LOOKBACK, cells: int = 1 << 22):
    """`chain` for many groups at once: step i of every group that has an anchor i is one numpy step over [groups, lookback].
    Same recurrence, same tie rules; returns the list of (score, first, last, count) in the order given."""
    order = sorted(range(len(tps)), key=lambda g: -len(tps[g]))
    out = [None] * len(tps)
    H = lookback
    MIN = np.iinfo(np.int64).min
    d = np.arange(bandwidth + 2, dtype=np.int64)
    COST = ((d * k) >> 6) + (_ilog2(d + 1) >> 1)                       # cost(d) for every d a valid step can have
    at = 0
    while at < len(order):
        nmax = len(tps[order[at]])
        nb = max(1, min(len(order) - at, cells // (nmax + H)))
        gs = order[at:at + nb]
        at += nb
        sizes = np.array([len(tps[g]) for g in gs], np.int64)          # descending
        TP = np.zeros((nb, nmax + H), np.int64)
        QP = np.zeros((nb, nmax + H), np.int64)
        F = np.zeros((nb, nmax + H), np.int64)
        OK = np.zeros((nb, nmax + H), bool)                             # a real anchor (the H columns in front are not)
        for r, g in enumerate(gs):
            TP[r, H:H + sizes[r]] = tps[g]
            QP[r, H:H + sizes[r]] = qps[g]
            OK[r, H:H + sizes[r]] = True
        PR = np.full((nb, nmax), -1, np.int64)
        for i in range(nmax):
            ga = int(np.searchsorted(-sizes, -i, side="left"))          # groups with more than i anchors: a prefix
            dt = TP[:ga, H + i, None] - TP[:ga, i:i + H][:, ::-1]       # nearest predecessor first
            dq = QP[:ga, H + i, None] - QP[:ga, i:i + H][:, ::-1]
            dd = np.abs(dt - dq)
            ok = OK[:ga, i:i + H][:, ::-1] & (dt > 0) & (dq > 0) & (dt <= max_gap) & (dq <= max_gap) & (dd <= bandwidth)
            sc = F[:ga, i:i + H][:, ::-1] + np.minimum(np.minimum(dt, dq), k) - COST[np.minimum(dd, bandwidth + 1)]
            sc = np.where(ok, sc, MIN)
            j = np.argmax(sc, axis=1)
            best = sc[np.arange(ga), j]
            take = best > k
            F[:ga, H + i] = np.where(take, best, k)
            PR[:ga, i] = np.where(take, i - 1 - j, -1)
        for r, g in enumerate(gs):
            f = F[r, H:H + sizes[r]]
            e = int(np.argmax(f))
            s, cnt = e, 1
            while PR[r, s] >= 0:
                s = int(PR[r, s])
                cnt += 1
            out[g] = (int(f[e]), s, e, cnt)
    return out


def pick_strands(chains) -> dict:
    """one overlap per read pair: chains (t, q, rel, score, ts, te, qs, qe, count) in ascending (t, q, rel) ->
    {(t, q): (score, rel, ts, te, qs, qe, count)}, the better-scoring strand, strand 0 on a tie"""
    best = {}
    for t, q, rel, sc, ts, te, qs, qe, cnt in chains:
        cur = best.get((t, q))
        if cur is None or sc > cur[0]:
            best[(t, q)] = (sc, rel, ts, te, qs, qe, cnt)
    return best


def find_overlaps(read_codes, lookback: int | None = LOOKBACK, stats: dict | None = None, **kw):
    """The whole specification.  Returns (rids u32 [n_targets], rows u32 [n, 10], aln_off u64 [n_targets + 1], scores i32 [n]):
    rows in create_job's layout (qid, qlen, qstart, qend, strand, tid, tlen, tstart, tend, 0), grouped by target in ascending
    read id, each target's records in ascending qid."""
    P = params(**kw)
    k = P["k"]
    lens = np.array([len(c) for c in read_codes], np.int64)
    h, rid, pos, st = sketch_store(read_codes, k, P["w"])
    a = anchors(h, rid, pos, st, lens, k, P["max_occ"])
    if stats is not None:
        stats["minimizers"], stats["anchors"] = len(h), len(a)
    kept = []
    if len(a):
        key = a[:, :3]
        b = np.flatnonzero(np.concatenate([[True], (key[1:] != key[:-1]).any(axis=1), [True]]))
        spans = [(g0, g1) for g0, g1 in zip(b[:-1], b[1:]) if g1 - g0 >= P["min_anchors"]]
        tps, qps = [a[g0:g1, 3] for g0, g1 in spans], [a[g0:g1, 4] for g0, g1 in spans]
        if lookback is None:
            chains = [chain(tp, qp, k, P["bandwidth"], P["max_gap"], None) for tp, qp in zip(tps, qps)]
        else:
            chains = chain_many(tps, qps, k, P["bandwidth"], P["max_gap"], lookback)
        for (g0, g1), tp, qp, (sc, s0, e0, cnt) in zip(spans, tps, qps, chains):
            t, q, rel = (int(x) for x in a[g0, :3])
            if sc < P["min_score"] or cnt < P["min_anchors"]:
                continue
            ts, te = int(tp[s0]) - k + 1, int(tp[e0]) + 1
            qs, qe = int(qp[s0]) - k + 1, int(qp[e0]) + 1
            if rel:
                qs, qe = int(lens[q]) - qe, int(lens[q]) - qs
            kept.append((t, q, rel, sc, ts, te, qs, qe, cnt))
    best = pick_strands(kept)
    if stats is not None:
        stats["pairs"] = dict(best)
    recs = []
    for (t, q), (sc, rel, ts, te, qs, qe, cnt) in best.items():
        recs.append((t, q, int(lens[q]), qs, qe, rel, t, int(lens[t]), ts, te, 0, sc))
        recs.append((q, t, int(lens[t]), ts, te, rel, q, int(lens[q]), qs, qe, 0, sc))
    recs.sort(key=lambda r: (r[0], r[1]))
    arr = np.array(recs, np.int64).reshape(-1, 12)
    rows = arr[:, 1:11].astype(np.uint32)
    scores = arr[:, 11].astype(np.int32)
    rids, counts = np.unique(arr[:, 0], return_counts=True)
    aln_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    return rids.astype(np.uint32), rows, aln_off, scores
