"""numpy restatement of the aligner herro_align_overlaps runs on the GPU (csrc/align_dev.hip).

This file is the reference the kernel is held to, bit for bit: banded Gotoh (+2 / -4, a gap of k costs 4 + 2k), W = 128 cells
per anti-diagonal d = i + j starting at lo_0 = -64, the band moving up one cell after d when H(top) > H(bot) (-inf == -inf),
traceback from (n, m) with ties diagonal > I > D in H and "open" on ties in I / D, then the reference's fix_cigar
(aligners.rs:138-250) and one trailing indel dropped.  A record fails when (n, m) leaves the band, when H(n, m) is -inf, or
when the final CIGAR is empty or does not start and end with M.

The DP runs along anti-diagonals for a group of records at once (arrays records x band).  It is written from the
specification, not from the kernel: cells are addressed by their i on every diagonal (no shifting of register arrays), the
matrix edges are explicit masks and -inf is exact (normalised after every step)."""
from __future__ import annotations

import numpy as np

W = 128
NEG = -(1 << 30)
FIN = -(1 << 29)
MATCH, MISMATCH, GAP_OPEN, GAP_EXT = 2, -4, 4, 2
M_, I_, D_ = 0, 1, 2
# A test hook, never set by the specification: True makes the band's bottom cell (k = 0) read -inf above it and diagonally below it,
# as k_align and k_extend once did after the band had moved.  tests/extend_ref.py reads it too.
BOTTOM_CELL_FORGETS = False
LETTER = "MID"


# ---- the read store's 2-bit codes (haec_io.rs:121-136, the non-ACGT quirk included) ---------------------------------------
def store_codes(seq: bytes) -> np.ndarray:
    """codes 0..3 of every base of one read as the read store holds them: a non-ACGT byte ORs 255 unmasked into its word."""
    b = np.frombuffer(seq, np.uint8)
    n = len(b)
    if n == 0:
        return np.zeros(0, np.uint8)
    tab = np.full(256, 255, np.uint64)
    for ch, c in zip(b"ACGTacgt", (0, 1, 2, 3, 0, 1, 2, 3)):
        tab[ch] = c
    nw = (n + 31) // 32
    pad = np.zeros(nw * 32, np.uint64)
    pad[:n] = tab[b]
    words = np.zeros(nw, np.uint64)
    for j in range(32):
        words |= (pad[j::32] << np.uint64(2 * j)) & np.uint64(0xFFFFFFFFFFFFFFFF)
    pos = np.arange(n, dtype=np.uint64)
    return ((words[pos >> np.uint64(5)] >> ((pos & np.uint64(31)) * np.uint64(2))) & np.uint64(3)).astype(np.uint8)


def record_seqs(read_codes, row):
    """(T, Q) codes of a record row (qid, qlen, qstart, qend, strand, tid, tlen, tstart, tend): strand 1 reads the query
    region reversed and complemented (features.rs:128-153)."""
    qid, _, qs, qe, strand, tid, _, ts, te = (int(x) for x in row[:9])
    T = read_codes[tid][ts:te]
    Q = read_codes[qid][qs:qe]
    if strand:
        Q = (3 - Q[::-1]).astype(np.uint8)
    return np.ascontiguousarray(T), np.ascontiguousarray(Q)


# ---- banded DP over a group of records ------------------------------------------------------------------------------------
def _norm(x):
    return np.where(x < FIN, np.int32(NEG), x)


def _band_group(Ts, Qs):
    """DP + traceback for records of similar size; returns per record (hend or None, step types from the END of the path)."""
    R = len(Ts)
    n = np.array([len(q) for q in Qs], np.int64)
    m = np.array([len(t) for t in Ts], np.int64)
    D = n + m
    Dmax = int(D.max())
    P = W + 2
    # padded codes: Qp[r, P + x] = Q[x]; out-of-range codes are 4 (never read for a valid cell)
    Qp = np.full((R, Dmax + 2 * P), 4, np.int8)
    Tp = np.full((R, Dmax + 2 * P), 5, np.int8)
    for r in range(R):
        Qp[r, P:P + n[r]] = Qs[r]
        Tp[r, P:P + m[r]] = Ts[r]
    k = np.arange(W, dtype=np.int64)[None, :]
    rr = np.arange(R)[:, None]
    lo_hist = np.zeros((R, Dmax + 1), np.int64)
    tb = np.zeros((R, Dmax + 1, W), np.uint8)
    lo = np.full(R, -W // 2, np.int64)
    # diagonal 0
    i0 = lo[:, None] + k
    H1 = np.where(i0 == 0, 0, NEG).astype(np.int32)
    I1 = np.full((R, W), NEG, np.int32)
    D1 = np.full((R, W), NEG, np.int32)
    H2 = np.full((R, W), NEG, np.int32)
    lo1 = lo.copy()       # lo of diagonal d - 1
    lo2 = lo.copy() - 1   # lo of diagonal d - 2 (diagonal -1 is all -inf anyway)
    lo_hist[:, 0] = lo
    hend = np.full(R, NEG, np.int64)
    endk = np.full(R, -1, np.int64)

    def take(A, idx):
        ok = (idx >= 0) & (idx < W)
        return np.where(ok, np.take_along_axis(A, np.clip(idx, 0, W - 1), axis=1), np.int32(NEG))

    for d in range(1, Dmax + 1):
        # the band of diagonal d: decided after d - 1 (d - 1 = 0: both edge cells lie outside the matrix)
        if d >= 2:
            tH = H1[:, W - 1]
            bH = H1[:, 0]
            lo = lo1 + (tH > bH)
        else:
            lo = lo1.copy()
        i = lo[:, None] + k
        j = d - i
        valid = (i >= 0) & (i <= n[:, None]) & (j >= 0) & (j <= m[:, None])
        upH = take(H1, i - 1 - lo1[:, None])
        upI = take(I1, i - 1 - lo1[:, None])
        lfH = take(H1, i - lo1[:, None])
        lfD = take(D1, i - lo1[:, None])
        dgH = take(H2, i - 1 - lo2[:, None])
        if BOTTOM_CELL_FORGETS:
            upH[:, 0] = NEG; upI[:, 0] = NEG; dgH[:, 0] = NEG
        io, ie = _norm(upH - GAP_OPEN - GAP_EXT), _norm(upI - GAP_EXT)
        dop, de = _norm(lfH - GAP_OPEN - GAP_EXT), _norm(lfD - GAP_EXT)
        Iv = np.maximum(io, ie)
        Dv = np.maximum(dop, de)
        qc = Qp[rr, np.clip(i - 1 + P, 0, Qp.shape[1] - 1)]
        tc = Tp[rr, np.clip(j - 1 + P, 0, Tp.shape[1] - 1)]
        sd = np.where(dgH == NEG, np.int32(NEG), dgH + np.where(qc == tc, np.int32(MATCH), np.int32(MISMATCH)))
        Hv = np.maximum(sd, np.maximum(Iv, Dv))
        src = np.where(Hv == sd, 0, np.where(Hv == Iv, 1, 2))
        nib = src | np.where(io >= ie, 4, 0) | np.where(dop >= de, 8, 0)
        Hv = np.where(valid, Hv, np.int32(NEG))
        Iv = np.where(valid, Iv, np.int32(NEG))
        Dv = np.where(valid, Dv, np.int32(NEG))
        live = d <= D
        tb[:, d, :] = nib.astype(np.uint8)
        lo_hist[:, d] = lo
        fin = D == d
        if fin.any():
            kk = n - lo
            inb = fin & (kk >= 0) & (kk < W)
            endk[inb] = kk[inb]
            hend[inb] = Hv[inb, kk[inb]]
        H2, lo2 = np.where(live[:, None], H1, H2), np.where(live, lo1, lo2)
        H1 = np.where(live[:, None], Hv, H1)
        I1 = np.where(live[:, None], Iv, I1)
        D1 = np.where(live[:, None], Dv, D1)
        lo1 = np.where(live, lo, lo1)

    # traceback, every record at once
    ok = (D > 0) & (endk >= 0) & (hend > FIN)
    steps = np.full((R, Dmax + 1), -1, np.int8)
    ns = np.zeros(R, np.int64)
    dd = np.where(ok, D, 0)
    ii = n.copy()
    mat = np.zeros(R, np.int64)
    act = ok & (dd > 0)
    while act.any():
        a = np.nonzero(act)[0]
        kk = ii[a] - lo_hist[a, dd[a]]
        bad = (kk < 0) | (kk >= W)
        if bad.any():
            ok[a[bad]] = False
            act[a[bad]] = False
            a, kk = a[~bad], kk[~bad]
        nb = tb[a, dd[a], kk].astype(np.int64)
        mt = mat[a]
        h_sw = (mt == 0) & ((nb & 3) != 0)
        mat[a[h_sw]] = (nb & 3)[h_sw]
        stp = ~h_sw
        a, nb, mt = a[stp], nb[stp], mt[stp]
        steps[a, ns[a]] = mt
        ns[a] += 1
        ii[a] -= (mt != D_)
        dd[a] -= np.where(mt == M_, 2, 1)
        nm = np.where(mt == I_, np.where(nb & 4, 0, 1), np.where(mt == D_, np.where(nb & 8, 0, 2), 0))
        mat[a] = nm
        act = ok & (dd > 0)
    ok &= (dd == 0) & (ii == 0) & (mat == 0)
    return [(int(hend[r]) if ok[r] else None, steps[r, :ns[r]][::-1] if ok[r] else None) for r in range(R)]


def runs(step_types: np.ndarray):
    """step types (path order) -> [(len, type)]"""
    if len(step_types) == 0:
        return []
    cut = np.nonzero(np.diff(step_types))[0] + 1
    starts = np.concatenate([[0], cut])
    ends = np.concatenate([cut, [len(step_types)]])
    return [(int(e - s), int(step_types[s])) for s, e in zip(starts, ends)]


# ---- fix_cigar (aligners.rs:138-250) ------------------------------------------------------------------------------------
def fix_cigar(cigar, target, query):
    """cigar: list of (len, type) with type 0 M, 1 I, 2 D; target / query: indexable sequences.  Returns (cigar, tshift, qshift)
    exactly as the reference: indels between two M left-shifted while the bases repeat, zero-length M dropped, a leading
    indel dropped (its length reported), adjacent equal ops merged."""
    cig = [list(op) for op in cigar]
    tpos = qpos = 0
    for i in range(len(cig)):
        ln, t = cig[i]
        if t == M_:
            tpos += ln
            qpos += ln
            continue
        if 0 < i < len(cig) - 1 and cig[i - 1][1] == M_ and cig[i + 1][1] == M_:
            prev_len = cig[i - 1][0]
            l = 0
            if t == I_:
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
        if t == I_:
            qpos += ln
        else:
            tpos += ln
    out, is_start, tshift, qshift = [], True, 0, 0
    for ln, t in cig:
        if is_start:
            if t == M_:
                if ln > 0:
                    is_start = False
                    out.append([ln, t])
                continue
            is_start = False
            if t == I_:
                qshift = ln
            else:
                tshift = ln
            continue
        if ln > 0:
            out.append([ln, t])
    merged = []
    for ln, t in out:
        if merged and merged[-1][1] == t:
            merged[-1][0] += ln
        else:
            merged.append([ln, t])
    return [tuple(x) for x in merged], tshift, qshift


def cigar_text(cig) -> bytes:
    return "".join(f"{ln}{LETTER[t]}" for ln, t in cig).encode()


def parse_cigar(text: bytes):
    out, num = [], 0
    for ch in text.decode():
        if ch.isdigit():
            num = num * 10 + int(ch)
        else:
            out.append((num, "MID".index(ch)))
            num = 0
    return out


def score_cigar(cig, T, Q):
    """score of a CIGAR against (T, Q) from their starts; raises if it does not consume both exactly"""
    t = q = s = 0
    for ln, ty in cig:
        if ty == M_:
            eq = int(np.count_nonzero(np.asarray(T[t:t + ln]) == np.asarray(Q[q:q + ln])))
            if t + ln > len(T) or q + ln > len(Q):
                raise ValueError("CIGAR runs past the sequences")
            s += MATCH * eq + MISMATCH * (ln - eq)
            t += ln
            q += ln
        elif ty == I_:
            s -= GAP_OPEN + GAP_EXT * ln
            q += ln
        else:
            s -= GAP_OPEN + GAP_EXT * ln
            t += ln
    if t != len(T) or q != len(Q):
        raise ValueError(f"CIGAR consumes ({t}, {q}) of ({len(T)}, {len(Q)})")
    return s


# ---- whole records ------------------------------------------------------------------------------------------------------
INT32_MIN = -(1 << 31)


def align_records(read_codes, rows, group_bytes: int = 96 << 20, threads: int = 8):
    """The full specification for record rows u32 [n, >=9].  Returns (rows_out u32 [n, 10], cigars list of bytes, scores i64 [n],
    ok bool [n], hend list: the DP optimum H(n, m) before normalisation, None when failed) — what herro_align_overlaps returns."""
    rows = np.asarray(rows)
    N = len(rows)
    seqs = [record_seqs(read_codes, rows[r]) for r in range(N)]
    Dv = np.array([len(t) + len(q) for t, q in seqs], np.int64)
    order = np.argsort(Dv, kind="stable")
    groups, g = [], 0
    while g < N:                       # records of similar size together; the traceback bits of a group stay within group_bytes
        cap = max(1, group_bytes // ((int(Dv[order[g]]) + 1) * W + 1))
        idx = order[g:g + cap]
        cap = max(1, group_bytes // ((int(Dv[idx].max()) + 1) * W + 1))
        idx = order[g:g + cap]
        groups.append(idx)
        g += len(idx)
    res = [None] * N

    def run(idx):
        for r, o in zip(idx, _band_group([seqs[r][0] for r in idx], [seqs[r][1] for r in idx])):
            res[r] = o
    import concurrent.futures as cf
    with cf.ThreadPoolExecutor(max(1, min(threads, len(groups)))) as ex:   # numpy drops the GIL inside the large array operations
        list(ex.map(run, groups))
    rows_out = np.zeros((N, 10), np.uint32)
    rows_out[:, :9] = rows[:, :9]
    cigars, scores, ok, hends = [], np.full(N, INT32_MIN, np.int64), np.zeros(N, bool), []
    for r in range(N):
        hend, st = res[r]
        T, Q = seqs[r]
        if hend is None:
            cigars.append(b"")
            hends.append(None)
            continue
        cig, tsh0, qsh0 = fix_cigar(runs(st), T, Q)
        tsh1 = qsh1 = 0
        if cig and cig[-1][1] != M_:
            if cig[-1][1] == I_:
                qsh1 = cig[-1][0]
            else:
                tsh1 = cig[-1][0]
            cig = cig[:-1]
        if not cig or cig[0][1] != M_ or cig[-1][1] != M_:
            cigars.append(b"")
            hends.append(hend)
            continue
        row = rows_out[r]
        row[7] += tsh0
        row[8] -= tsh1
        if row[4] == 0:
            row[2] += qsh0
            row[3] -= qsh1
        else:
            row[3] -= qsh0
            row[2] += qsh1
        scores[r] = score_cigar(cig, T[tsh0:len(T) - tsh1], Q[qsh0:len(Q) - qsh1])
        txt = cigar_text(cig)
        row[9] = len(txt)
        cigars.append(txt)
        ok[r] = True
        hends.append(hend)
    return rows_out, cigars, scores, ok, hends


def gotoh_unbanded(T, Q) -> int:
    """global Gotoh optimum of the same scores over the whole matrix (row by row)"""
    n, m = len(Q), len(T)
    T = np.asarray(T, np.int64)
    H = np.array([0] + [-(GAP_OPEN + GAP_EXT * j) for j in range(1, m + 1)], np.int64)
    I = np.full(m + 1, NEG, np.int64)
    for i in range(1, n + 1):
        In = np.maximum(H - GAP_OPEN - GAP_EXT, I - GAP_EXT)
        diag = H[:-1] + np.where(T == Q[i - 1], MATCH, MISMATCH)
        Hn = np.empty(m + 1, np.int64)
        Hn[0] = -(GAP_OPEN + GAP_EXT * i)
        Hn[1:] = np.maximum(diag, In[1:])
        # D runs along the row: D(j) = max(H(j-1) - 6, D(j-1) - 2), H(j) = max(Hn(j), D(j))
        Dp = NEG
        for j in range(1, m + 1):
            Dp = max(Hn[j - 1] - GAP_OPEN - GAP_EXT, Dp - GAP_EXT)
            if Dp > Hn[j]:
                Hn[j] = Dp
        H, I = Hn, In
    return int(H[m])
