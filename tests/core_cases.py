"""The core masks of the core-set tests (tests/test_core_host.py, tests/test_gpu_core.py), the filter that specifies what a masked finder
returns, and the counts the read sets of tests/pair_cases.py have under those masks.

A core mask has one byte per read, non-zero = the read is a target (include/herro_amd.h, "a core set of targets").  A read pair is wanted
iff one of its reads is core, a row (target, query) iff its target is core.  Chains are independent per (t, q, strand) and max_occ is the
cut of the whole store's index, so the masked result is a selection of the unmasked one: filter_pairs / filter_rows below ARE the
specification, applied to the unmasked result of the same reads and parameters."""
import numpy as np

import overlap_ref as R
import pair_cases as PC
from herro_amd import api


# ---- masks ----------------------------------------------------------------------------------------------------------------------------------
def masks(n: int) -> dict:
    i = np.arange(n)
    one, last = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    one[n // 2] = 1
    last[n - 1] = 1
    return dict(none=np.zeros(n, np.uint8), all=np.ones(n, np.uint8), one=one, last=last, every3rd=(i % 3 == 0).astype(np.uint8),
                first_half=(i < n // 2).astype(np.uint8))


def odd_bytes(mask) -> np.ndarray:
    """the same mask with the byte values 2 and 255, alternating, in place of 1"""
    m = np.asarray(mask, np.uint8).copy()
    at = np.flatnonzero(m)
    m[at[0::2]] = 2
    m[at[1::2]] = 255
    return m


# ---- the specification ------------------------------------------------------------------------------------------------------------------
def filter_pairs(fields: dict, core, _targets_only: bool = False) -> dict:
    """the fields of an OverlapPairs handle (pair_cases.pairs_fields / stepwise) under a core mask.  _targets_only is not part of the
    specification: the mutant that wants a pair only where its primary's target is core (tests/test_combo_host.py)."""
    c = np.asarray(core) != 0
    pr = np.asarray(fields["primaries"])
    P = len(pr)
    keep = (c[pr[:, 5]] if _targets_only else c[pr[:, 5]] | c[pr[:, 0]]) if P else np.zeros(0, bool)
    new = np.cumsum(keep) - 1                                      # the new index of a kept primary
    Pn = int(keep.sum())
    rids, aln_off, rec = np.asarray(fields["rids"]), np.asarray(fields["aln_off"]), np.asarray(fields["rec_of_row"])
    row_t = np.repeat(rids, np.diff(aln_off.astype(np.int64)))     # the target of every row
    keep_row = c[row_t] if len(row_t) else np.zeros(0, bool)
    if _targets_only and len(row_t):
        keep_row = keep_row & keep[rec.astype(np.int64) % P]
    r = rec[keep_row].astype(np.int64)
    assert keep[r % P].all() if len(r) else True                   # a row with a core target belongs to a kept pair
    new_rec = np.where(r < P, new[r % P], Pn + new[r % P]) if len(r) else np.zeros(0, np.int64)
    keep_t = c[rids] if len(rids) else np.zeros(0, bool)
    per_t = np.add.reduceat(keep_row.astype(np.int64), aln_off[:-1].astype(np.int64))[keep_t] if len(rids) else np.zeros(0, np.int64)
    return dict(primaries=pr[keep], chain_scores=np.asarray(fields["chain_scores"])[keep], ext=np.asarray(fields["ext"])[keep],
                ext_scores=np.asarray(fields["ext_scores"])[keep], rids=rids[keep_t],
                aln_off=np.concatenate([[0], np.cumsum(per_t)]).astype(aln_off.dtype), rec_of_row=new_rec.astype(rec.dtype))


def filter_rows(rids, rows, aln_off, scores, core):
    """find_overlaps' result under a core mask: the records whose tid is core, in the same order, with the same scores"""
    c = np.asarray(core) != 0
    rids, rows, aln_off, scores = np.asarray(rids), np.asarray(rows), np.asarray(aln_off), np.asarray(scores)
    keep = c[rows[:, 5]] if len(rows) else np.zeros(0, bool)
    keep_t = c[rids] if len(rids) else np.zeros(0, bool)
    per_t = np.diff(aln_off.astype(np.int64))[keep_t]              # a core target keeps all its rows
    return rids[keep_t], rows[keep], np.concatenate([[0], np.cumsum(per_t)]).astype(aln_off.dtype), scores[keep]


# ---- counts from the numpy reference ------------------------------------------------------------------------------------------------
_REF = {}


def reference(name: str, kw: dict):
    """(codes, anchors [n, 5], the stepwise fields without extension) of a read set of pair_cases at parameters kw, on the CPU"""
    key = (name, tuple(sorted(kw.items())))
    if key not in _REF:
        rs = dict((n, m) for n, m, _ in PC.SETS)[name]()
        off = np.asarray(rs.off).astype(np.int64)
        codes = [R.store_codes(bytes(np.asarray(rs.seq[off[i]:off[i + 1]]))) for i in range(len(off) - 1)]
        P = R.params(**kw)
        lens = np.array([len(x) for x in codes], np.int64)
        a = R.anchors(*R.sketch_store(codes, P["k"], P["w"]), lens, P["k"], P["max_occ"])
        rids, rows, aln_off, scores = R.find_overlaps(codes, **kw)
        prim, rec = api.pair_rows(rows, exact_ids=True) if len(rows) else (np.zeros(0, np.int64), np.zeros(0, np.uint32))
        n = len(prim)
        fields = dict(primaries=rows[prim].reshape(n, 10), chain_scores=scores[prim], ext=np.zeros((n, 4), np.uint32),
                      ext_scores=np.zeros((n, 2), np.int32), rids=rids, aln_off=aln_off, rec_of_row=rec)
        _REF[key] = (codes, a, fields)
    return _REF[key]


def counts(name: str, kw: dict, core):
    """(anchors, pairs, rows) under the mask"""
    _, a, fields = reference(name, kw)
    c = np.asarray(core) != 0
    f = filter_pairs(fields, core)
    return int((c[a[:, 0]] | c[a[:, 1]]).sum()) if len(a) else 0, len(f["primaries"]), len(f["rec_of_row"])


# (set, parameters) -> the unmasked (anchors, pairs) and {mask: (anchors, pairs, rows)}
EXPECTED = {
    ("B", "DEFAULTS"): ((6838, 75), dict(every3rd=(4233, 42, 48), first_half=(4216, 43, 70), one=(744, 7, 7), last=(762, 7, 7))),
    ("B", "SMALL_K"): ((35654, 78), dict(every3rd=(20615, 44, 50), first_half=(19824, 44, 72), one=(3928, 7, 7))),
    ("D", "DEFAULTS"): ((943, 4), dict(first_half=(733, 3, 5), every3rd=(728, 3, 3), last=(0, 0, 0))),
}
PARAMS = dict(DEFAULTS=PC.DEFAULTS, SMALL_K=PC.SMALL_K)
C_ANCHORS = 660          # set C at the defaults: one pair; any one-read mask keeps every anchor, the pair and one row
