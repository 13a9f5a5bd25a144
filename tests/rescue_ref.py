"""numpy restatement of the rescue of high-frequency minimizers (herro_set_seed_rescue; csrc/overlap_dev.hip: k_occ_place, k_rescue, k_resc_kind,
the RESCUE side of k_runs / k_expand; DESIGN.md §10, "Rescue of high-frequency minimizers"), on top of overlap_ref.  All integer; the kernels
equal it bit for bit.

  occ      occ(x) = occurrences of x's hash in the whole store; cut = the frequency cut the call uses anyway (max_occ, or occ_ref's).
  classes  U: 2 <= occ <= cut.  H: cut < occ <= rescue_max_occ.  Transparent: everything else (singletons, hashes above rescue_max_occ) —
           such a minimizer neither ends a streak nor is rescued.
  streaks  per read, over its U and H minimizers in ascending pos: a streak is a maximal run of H.  ps = pos of the U in front of it (0: none),
           pe = pos of the U behind it (the read's length: none), m = (2 (pe - ps) + occ_dist) // (2 occ_dist).  The m members with the least
           (occ, pos) are rescued; all of them if m >= the streak's size.
  anchors  two occurrences of one hash in reads t < q give an anchor iff 2 <= occ <= cut, or cut < occ <= rescue_max_occ and one of the two is
           rescued.  Everything behind the anchors is overlap_ref's.

The underscored arguments are not part of the specification: they make the mutants the tests hold it against."""
from __future__ import annotations

import numpy as np

import overlap_ref as R

RESCUE_MAX_OCC = 4095        # rescue_max_occ 0 / None
OCC_DIST_MAX = 1 << 20
OCC_CAP = 65535              # what herro_debug_seed_rescue reports: min(occ, 65535)
_PLAIN_ANCHORS = R.anchors   # (find_overlaps_rescue puts anchors_rescue in its place for the length of a call)


def check(occ_dist: int, rescue_max_occ: int | None = None) -> tuple[int, int]:
    """(occ_dist, rescue_max_occ) filled in; ValueError where herro_set_seed_rescue returns HERRO_E_INVALID.  occ_dist 0 is off, not an error."""
    d, m = int(occ_dist or 0), int(rescue_max_occ or 0)
    if not 0 <= d <= OCC_DIST_MAX or not 0 <= m <= 65534:
        raise ValueError("occ_dist <= 2^20, rescue_max_occ <= 65534")
    return d, m or RESCUE_MAX_OCC


def occurrences(h) -> np.ndarray:
    """occ of every minimizer, int64 [n]"""
    h = np.asarray(h, np.uint64)
    if not len(h):
        return np.zeros(0, np.int64)
    _, inv, cnt = np.unique(h, return_inverse=True, return_counts=True)
    return cnt[inv].astype(np.int64)


def streak_quota(ps: int, pe: int, occ_dist: int, _round_down: bool = False) -> int:
    return (pe - ps) // occ_dist if _round_down else (2 * (pe - ps) + occ_dist) // (2 * occ_dist)


def streaks(occ, pos, length: int, cut: int, rmax: int, _band: int | None = None):
    """the streaks of one read (occ, pos in ascending pos): a list of (member indices int64, ps, pe)"""
    out, cur, ps = [], [], 0
    lo = cut if _band is None else _band         # (the mutant's H begins above _band, not above the cut)
    for i, (c, p) in enumerate(zip(occ, pos)):
        if 2 <= c <= cut:
            if cur:
                out.append((np.array(cur, np.int64), ps, int(p)))
                cur = []
            ps = int(p)
        elif lo < c <= rmax:
            cur.append(i)
    if cur:
        out.append((np.array(cur, np.int64), ps, int(length)))
    return out


def rescue_flags(h, rid, pos, lens, cut: int, occ_dist: int, rescue_max_occ: int | None = None, _larger_pos: bool = False, _round_down: bool = False,
                 _band: int | None = None):
    """(occ int64 [n], rescued u8 [n]) for minimizers sorted by (rid, pos), as overlap_ref.sketch_store returns them"""
    d, rmax = check(occ_dist, rescue_max_occ)
    occ = occurrences(h)
    flag = np.zeros(len(occ), np.uint8)
    if not d:
        return occ, flag
    rid, pos = np.asarray(rid, np.int64), np.asarray(pos, np.int64)
    bounds = np.searchsorted(rid, np.arange(len(lens) + 1))
    for r in range(len(lens)):
        b, e = int(bounds[r]), int(bounds[r + 1])
        for idx, ps, pe in streaks(occ[b:e], pos[b:e], int(lens[r]), cut, rmax, _band):
            m = streak_quota(ps, pe, d, _round_down)
            if m >= len(idx):
                take = idx
            else:
                p = pos[b:e][idx]
                take = idx[np.lexsort((-p if _larger_pos else p, occ[b:e][idx]))[:m]]
            flag[b + take] = 1
    return occ, flag


def anchors_rescue(h, rid, pos, st, lens, k: int, cut: int, flag, rescue_max_occ: int | None = None, _both: bool = False, _band: int | None = None):
    """overlap_ref.anchors plus the anchors of the hashes above the cut: (t, q, rel, tpos, qpos) int64 rows sorted by that tuple"""
    rmax = check(1, rescue_max_occ)[1]
    a = [_PLAIN_ANCHORS(h, rid, pos, st, lens, k, cut)]
    occ = occurrences(h)
    high = np.flatnonzero((occ > (cut if _band is None else _band)) & (occ <= rmax))
    if len(high):
        o = high[np.lexsort((pos[high], rid[high], h[high]))]
        hh, rr, pp, ss, ff = h[o], rid[o], pos[o], st[o].astype(np.int64), np.asarray(flag)[o].astype(bool)
        b = np.flatnonzero(np.concatenate([[True], hh[1:] != hh[:-1], [True]]))
        for s0, s1 in zip(b[:-1], b[1:]):
            x, y = np.triu_indices(int(s1 - s0), 1)
            x, y = x + s0, y + s0
            keep = (rr[x] != rr[y]) & ((ff[x] & ff[y]) if _both else (ff[x] | ff[y]))
            x, y = x[keep], y[keep]
            rel = ss[x] ^ ss[y]
            qpos = np.where(rel == 0, pp[y], lens[rr[y]] - pp[y] + k - 2)
            a.append(np.stack([rr[x], rr[y], rel, pp[x], qpos], axis=1).astype(np.int64).reshape(-1, 5))
    a = np.concatenate(a)
    return a[np.lexsort((a[:, 4], a[:, 3], a[:, 2], a[:, 1], a[:, 0]))]


def find_overlaps_rescue(read_codes, occ_dist: int, rescue_max_occ: int | None = None, occ_frac_ppm: int = 0, stats: dict | None = None,
                         lookback: int | None = R.LOOKBACK, _larger_pos: bool = False, _round_down: bool = False, _both: bool = False,
                         _lookback_64: bool = False, _band_from_max_occ: bool = False, **kw):
    """overlap_ref.find_overlaps with the rescue: (rids, rows, aln_off, scores).  occ_frac_ppm != 0: the cut is occ_ref's, max_occ its ceiling.
    lookback: overlap_ref.find_overlaps' own, handed on as it is.  stats gains cut, occ, rescued (the flags) and high (the H minimizers).
    _lookback_64: with the rescue on, the chains look back 64 whatever was asked; _band_from_max_occ: under occ_frac_ppm, H begins above
    max_occ instead of above the cut (what lies between is neither used nor rescued)."""
    P = R.params(**{n: v for n, v in kw.items() if not (occ_frac_ppm and n == "max_occ")})
    lens = np.array([len(c) for c in read_codes], np.int64)
    h, rid, pos, st = R.sketch_store(read_codes, P["k"], P["w"])
    cut = P["max_occ"]
    if occ_frac_ppm:
        import occ_ref as OR
        cut = OR.occ_cut(OR.run_counts(h), occ_frac_ppm, int(kw.get("max_occ") or 0))
    band = int(kw["max_occ"]) if _band_from_max_occ and occ_frac_ppm and kw.get("max_occ") else None
    occ, flag = rescue_flags(h, rid, pos, lens, cut, occ_dist, rescue_max_occ, _larger_pos, _round_down, band)
    if stats is not None:
        rmax = check(occ_dist, rescue_max_occ)[1]
        stats.update(cut=cut, occ=occ, rescued=flag, high=int(((occ > cut) & (occ <= rmax)).sum()))
    if not check(occ_dist, rescue_max_occ)[0]:
        return R.find_overlaps(read_codes, lookback=lookback, stats=stats, **dict(kw, max_occ=cut))

    def with_rescue(h_, rid_, pos_, st_, lens_, k_, max_occ_):
        return anchors_rescue(h_, rid_, pos_, st_, lens_, k_, max_occ_, flag, rescue_max_occ, _both, band)
    R.anchors = with_rescue              # everything behind the anchors is overlap_ref.find_overlaps itself, not a copy of it
    try:
        return R.find_overlaps(read_codes, lookback=R.LOOKBACK if _lookback_64 else lookback, stats=stats, **dict(kw, max_occ=cut))
    finally:
        R.anchors = _PLAIN_ANCHORS
