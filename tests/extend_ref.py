"""numpy restatement of the end extension herro_extend_overlaps runs on the GPU (k_extend in csrc/align_dev.hip).

This file is the reference the kernel is held to, bit for bit.  A record has two independent sides.  The right side sweeps
Q' x T', the oriented query's and the target's bases behind the aligned span; the left side the bases in front of it, read away
from the span.  Each of the four sequences is cut to max_ext bases.  The sweep is §9's (tests/align_ref.py): banded Gotoh, +2 / -4,
a gap of k costs 4 + 2k, W = 128 cells per anti-diagonal d = i + j, lo_0 = -64, the band moving up one cell after d when
H(top) > H(bot), H(0, 0) = 0.  Nothing is traced back: the result is the best cell.

  best cell   starts as (score 0, i 0, j 0); after diagonal d every band cell with 1 <= i <= n, 1 <= j <= m and finite H is a
              candidate and replaces the result only if its H is strictly greater; among equal H on one diagonal the smallest i.
  stop rule   M_d = the maximum finite H over the band's in-matrix cells (0 <= i <= n, 0 <= j <= m) of diagonal d, -inf if none;
              after every diagonal with d % 16 == 0 the sweep stops if max(M_d, M_{d-1}) < best - zdrop; it ends at d = n + m.

Written from the specification, not from the kernel: cells are addressed by their i, the matrix edges are explicit masks and
-inf is exact.  Sides of similar size run together (arrays sides x band), as align_ref._band_group runs records."""
from __future__ import annotations

import numpy as np

import align_ref
from align_ref import FIN, GAP_EXT, GAP_OPEN, MATCH, MISMATCH, NEG, W, store_codes  # noqa: F401  (store_codes: re-exported)

ZDROP = 400          # zdrop = 0
MAX_EXT = 2048       # max_ext = 0
MAX_EXT_LIMIT = 1 << 20
CHECK = 16           # the stop rule is evaluated after every diagonal d with d % CHECK == 0
NINF = -(1 << 62)


def params(zdrop: int = 0, max_ext: int = 0):
    if max_ext > MAX_EXT_LIMIT:
        raise ValueError("max_ext above 2^20")
    return (zdrop or ZDROP), (max_ext or MAX_EXT)


def side_seqs(read_codes, row, max_ext: int):
    """((T_left, Q_left), (T_right, Q_right)) of a record row (qid, qlen, qstart, qend, strand, tid, tlen, tstart, tend): the bases
    in front of / behind the span, read away from it, the query in its orientation (strand 1: reversed and complemented)."""
    qid, _, qs, qe, strand, tid, _, ts, te = (int(x) for x in row[:9])
    t, q = read_codes[tid], read_codes[qid]
    oq = (3 - q[::-1]).astype(np.uint8) if strand else q               # the oriented query ...
    os_, oe = (len(q) - qe, len(q) - qs) if strand else (qs, qe)        # ... and the span on it
    left = (t[:ts][::-1][:max_ext], oq[:os_][::-1][:max_ext])
    right = (t[te:][:max_ext], oq[oe:][:max_ext])
    return tuple((np.ascontiguousarray(a), np.ascontiguousarray(b)) for a, b in (left, right))


def _norm(x):
    return np.where(x < FIN, np.int32(NEG), x)


def _ext_group(Ts, Qs, zdrop: int):
    """the sweep for sides of similar size, every side with n, m >= 1; returns int64 [R, 4]: score, i, j, the last diagonal computed"""
    R = len(Ts)
    n = np.array([len(q) for q in Qs], np.int64)
    m = np.array([len(t) for t in Ts], np.int64)
    D = n + m
    Dmax = int(D.max())
    P = W + 2
    Qp = np.full((R, Dmax + 2 * P), 4, np.int8)
    Tp = np.full((R, Dmax + 2 * P), 5, np.int8)
    for r in range(R):
        Qp[r, P:P + n[r]] = Qs[r]
        Tp[r, P:P + m[r]] = Ts[r]
    k = np.arange(W, dtype=np.int64)[None, :]
    rr = np.arange(R)[:, None]
    lo1 = np.full(R, -W // 2, np.int64)   # lo of diagonal d - 1
    lo2 = lo1 - 1                         # lo of diagonal d - 2 (diagonal -1 is all -inf anyway)
    H1 = np.where(lo1[:, None] + k == 0, 0, NEG).astype(np.int32)
    I1 = np.full((R, W), NEG, np.int32)
    D1 = np.full((R, W), NEG, np.int32)
    H2 = np.full((R, W), NEG, np.int32)
    best = np.zeros(R, np.int64)
    bi = np.zeros(R, np.int64)
    bj = np.zeros(R, np.int64)
    last = np.zeros(R, np.int64)
    Mprev = np.full(R, NINF, np.int64)
    live = np.ones(R, bool)

    def take(A, idx):
        ok = (idx >= 0) & (idx < W)
        return np.where(ok, np.take_along_axis(A, np.clip(idx, 0, W - 1), axis=1), np.int32(NEG))

    res = np.zeros((R, 4), np.int64)
    rows = np.arange(R)                    # the sides still in the arrays

    for d in range(1, Dmax + 1):
        if d % 32 == 1 and live.sum() < 0.75 * len(live):     # sides that have ended leave the arrays
            res[rows[~live]] = np.stack([best, bi, bj, last], 1)[~live]
            rows, n, m, D, Qp, Tp = rows[live], n[live], m[live], D[live], Qp[live], Tp[live]
            lo1, lo2, H1, I1, D1, H2 = lo1[live], lo2[live], H1[live], I1[live], D1[live], H2[live]
            best, bi, bj, last, Mprev = best[live], bi[live], bj[live], last[live], Mprev[live]
            R = len(rows)
            rr = np.arange(R)[:, None]
            live = np.ones(R, bool)
        if R == 0:
            break
        lo = lo1 + (H1[:, W - 1] > H1[:, 0]) if d >= 2 else lo1.copy()   # decided after d - 1; cells outside the matrix are -inf
        i = lo[:, None] + k
        j = d - i
        valid = (i >= 0) & (i <= n[:, None]) & (j >= 0) & (j <= m[:, None])
        upH = take(H1, i - 1 - lo1[:, None])
        upI = take(I1, i - 1 - lo1[:, None])
        lfH = take(H1, i - lo1[:, None])
        lfD = take(D1, i - lo1[:, None])
        dgH = take(H2, i - 1 - lo2[:, None])
        if align_ref.BOTTOM_CELL_FORGETS:
            upH[:, 0] = NEG; upI[:, 0] = NEG; dgH[:, 0] = NEG
        Iv = np.maximum(_norm(upH - GAP_OPEN - GAP_EXT), _norm(upI - GAP_EXT))
        Dv = np.maximum(_norm(lfH - GAP_OPEN - GAP_EXT), _norm(lfD - GAP_EXT))
        qc = Qp[rr, np.clip(i - 1 + P, 0, Qp.shape[1] - 1)]
        tc = Tp[rr, np.clip(j - 1 + P, 0, Tp.shape[1] - 1)]
        sd = np.where(dgH == NEG, np.int32(NEG), dgH + np.where(qc == tc, np.int32(MATCH), np.int32(MISMATCH)))
        Hv = np.where(valid, np.maximum(sd, np.maximum(Iv, Dv)), np.int32(NEG))
        Iv = np.where(valid, Iv, np.int32(NEG))
        Dv = np.where(valid, Dv, np.int32(NEG))
        # the best cell: candidates of this diagonal, the smallest i among equal H (argmax takes the first)
        cand = np.where(valid & (i >= 1) & (j >= 1) & (Hv > FIN), Hv.astype(np.int64), NINF)
        ck = np.argmax(cand, axis=1)
        ch = cand[np.arange(R), ck]
        up = live & (ch > best)
        best = np.where(up, ch, best)
        bi = np.where(up, lo + ck, bi)
        bj = np.where(up, d - (lo + ck), bj)
        last = np.where(live, d, last)
        # the stop rule
        Md = np.where(Hv > FIN, Hv.astype(np.int64), NINF).max(axis=1)
        stop = (np.maximum(Md, Mprev) < best - zdrop) if d % CHECK == 0 else np.zeros(R, bool)
        Mprev = Md
        go = live & ~stop & (d < D)        # sides that go on to diagonal d + 1
        H2, lo2 = np.where(go[:, None], H1, H2), np.where(go, lo1, lo2)
        H1 = np.where(go[:, None], Hv, H1)
        I1 = np.where(go[:, None], Iv, I1)
        D1 = np.where(go[:, None], Dv, D1)
        lo1 = np.where(go, lo, lo1)
        live = go
    res[rows] = np.stack([best, bi, bj, last], 1)
    return res


def extend_sides(sides, zdrop: int, group_cells: int = 1 << 22):
    """[(T', Q')] -> int64 [len, 4] (score, i, j, last diagonal); a side with n = 0 or m = 0 gives zeros"""
    res = np.zeros((len(sides), 4), np.int64)
    idx = [s for s in range(len(sides)) if len(sides[s][0]) and len(sides[s][1])]
    idx.sort(key=lambda s: len(sides[s][0]) + len(sides[s][1]))
    cap = max(1, group_cells // W)
    for g in range(0, len(idx), cap):
        part = idx[g:g + cap]
        res[part] = _ext_group([sides[s][0] for s in part], [sides[s][1] for s in part], zdrop)
    return res


def extend_records(read_codes, rows, zdrop: int = 0, max_ext: int = 0, stats: dict | None = None):
    """The full specification for record rows u32 [n, >=9].  Returns (rows_out u32 [n, 10] with the extended coordinates and
    cigar_len 0, ext u32 [n, 4]: t_left, q_left, t_right, q_right — the q lengths on the oriented query —, scores i32 [n, 2]: left,
    right) — what herro_extend_overlaps returns."""  # (stats["last"]: int64 [n, 2], for the tests of the stop rule)
    zdrop, max_ext = params(zdrop, max_ext)
    rows = np.asarray(rows)
    N = len(rows)
    sides = []
    for r in range(N):
        sides.extend(side_seqs(read_codes, rows[r], max_ext))
    res = extend_sides(sides, zdrop).reshape(N, 2, 4)
    if stats is not None:
        stats["last"] = res[:, :, 3].copy()      # the last anti-diagonal each side computed
    out = np.zeros((N, 10), np.uint32)
    out[:, :9] = rows[:, :9]
    o = out.astype(np.int64)
    il, jl, ir, jr = res[:, 0, 1], res[:, 0, 2], res[:, 1, 1], res[:, 1, 2]
    fwd = o[:, 4] == 0
    o[:, 7] -= jl
    o[:, 8] += jr
    o[:, 2] -= np.where(fwd, il, ir)
    o[:, 3] += np.where(fwd, ir, il)
    ext = np.stack([jl, il, jr, ir], 1).astype(np.uint32)
    scores = np.stack([res[:, 0, 0], res[:, 1, 0]], 1).astype(np.int32)
    return o.astype(np.uint32), ext, scores


def extend_unbanded(T, Q):
    """(score, i, j) of the same best-cell rule over the whole matrix, without band and without stop rule (row by row; short flanks)"""
    n, m = len(Q), len(T)
    T = np.asarray(T, np.int64)
    H = np.array([0] + [-(GAP_OPEN + GAP_EXT * j) for j in range(1, m + 1)], np.int64)
    I = np.full(m + 1, NINF // 2, np.int64)
    cells = []
    for i in range(1, n + 1):
        In = np.maximum(H - GAP_OPEN - GAP_EXT, I - GAP_EXT)
        diag = H[:-1] + np.where(T == Q[i - 1], MATCH, MISMATCH)
        Hn = np.empty(m + 1, np.int64)
        Hn[0] = -(GAP_OPEN + GAP_EXT * i)
        Hn[1:] = np.maximum(diag, In[1:])
        Dp = NINF // 2
        for j in range(1, m + 1):
            Dp = max(Hn[j - 1] - GAP_OPEN - GAP_EXT, Dp - GAP_EXT)
            if Dp > Hn[j]:
                Hn[j] = Dp
        cells.extend((int(Hn[j]), i + j, i, j) for j in range(1, m + 1))
        H, I = Hn, In
    best = (0, 0, 0)
    for h, d, i, j in sorted(cells, key=lambda c: (c[1], c[2])):     # diagonal by diagonal, ascending i
        if h > best[0]:
            best = (h, i, j)
    return best
