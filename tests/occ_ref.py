"""numpy restatement of the frequency cut taken from the index (occ_frac_ppm of herro_overlap_params; csrc/overlap_dev.hip: k_occ_census,
k_occ_pick; DESIGN.md §10, "The cut as a fraction"), on top of overlap_ref.  All integer; the kernels equal it bit for bit.

  census   over the index of the whole store: one count per distinct minimizer hash (singletons included), c' = min(c, 65535); the
           histogram has 65 536 bins, the last one collects every longer run.
  pick     D = distinct hashes; drop = floor(D * ppm / 10^6); q = min{v : #(c' > v) <= drop} — the (D - drop)-th smallest c', every run
           tied with it kept; cut = max(q, 10); min(cut, max_occ) if max_occ is not 0; min(cut, 65534).
  use      a run is used iff 2 <= c <= cut: everything behind is overlap_ref.find_overlaps(..., max_occ=cut)."""
from __future__ import annotations

import numpy as np

import overlap_ref as R

BINS = 65536
FLOOR = 10          # the least cut (minimap2's min_mid_occ)
PPM_MAX = 999_999


def check_ppm(ppm: int) -> int:
    """ValueError where the library returns HERRO_E_INVALID (0, the fixed cut, is not a fraction)"""
    ppm = int(ppm)
    if not 1 <= ppm <= PPM_MAX:
        raise ValueError("1 <= occ_frac_ppm <= 999999")
    return ppm


def run_counts(h) -> np.ndarray:
    """occurrences of every distinct hash, int64 [D]"""
    h = np.asarray(h, np.uint64)
    return np.unique(h, return_counts=True)[1].astype(np.int64) if len(h) else np.zeros(0, np.int64)


def histogram(counts) -> np.ndarray:
    """u32 [65536]: bin min(c, 65535) per run"""
    c = np.minimum(np.asarray(counts, np.int64), BINS - 1)
    return np.bincount(c, minlength=BINS).astype(np.uint32)


def occ_cut(counts, ppm: int, max_occ: int = 0, _rank: int = 0, _floor: int = FLOOR, _last: int = BINS - 2) -> int:
    """the cut for a multiset of run lengths.  The underscored arguments are not part of the specification: they make the mutants the
    tests hold it against (the pick one rank higher, no floor, the last bin usable)."""
    ppm = check_ppm(ppm)
    hist = histogram(counts).astype(np.int64)
    D = int(hist.sum())
    drop = D * ppm // 10**6
    above = hist[::-1].cumsum()[::-1] - hist                 # above[v] = runs with c' > v
    q = int(np.flatnonzero(above <= drop - _rank)[0]) if drop - _rank >= 0 else BINS - 1
    cut = max(q, _floor)
    if max_occ:
        cut = min(cut, int(max_occ))
    return min(cut, _last)


def figures(counts, ppm: int, max_occ: int = 0) -> dict:
    """what herro_debug_occ_census returns besides the histogram: the cut, the distinct hashes, the runs above the cut, their minimizers"""
    c = np.asarray(counts, np.int64)
    cut = occ_cut(c, ppm, max_occ)
    return dict(cut=cut, distinct=len(c), cut_runs=int((c > cut).sum()), cut_minimizers=int(c[c > cut].sum()))


def census(read_codes, occ_frac_ppm: int, **kw):
    """(hist u32 [65536], figures) of a read store; kw: the finder's parameters (k, w; max_occ: the ceiling, 0 or missing = none)"""
    P = R.params(**{n: v for n, v in kw.items() if n != "max_occ"})
    h, _, _, _ = R.sketch_store(read_codes, P["k"], P["w"])
    counts = run_counts(h)
    return histogram(counts), figures(counts, occ_frac_ppm, int(kw.get("max_occ") or 0))


def find_overlaps(read_codes, occ_frac_ppm: int, stats: dict | None = None, lookback: int | None = R.LOOKBACK, **kw):
    """overlap_ref.find_overlaps with the cut taken from the index: (rids, rows, aln_off, scores), cut.  lookback: overlap_ref.find_overlaps'
    own, handed on as it is (the census does not see it)."""
    _, fig = census(read_codes, occ_frac_ppm, **kw)
    if stats is not None:
        stats["occ"] = fig
    return R.find_overlaps(read_codes, lookback=lookback, stats=stats, **dict(kw, max_occ=fig["cut"])), fig["cut"]
