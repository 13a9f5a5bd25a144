"""The trials of the combination tests (tests/test_combo_host.py, tests/test_gpu_combo.py): the overlap finder's four options — the occurrence
cut as a fraction (occ_frac_ppm), the rescue (herro_set_seed_rescue), the core mask (herro_find_overlaps_core / herro_find_overlap_pairs_core)
and the chain look-back (herro_set_chain_params) — set together, on small repeat-bearing read sets, and the composition of the references that
states what the finder must return then.

A trial is (read set, finder keywords, rescue, occ_frac_ppm, look-back, core mask, extension keywords, scratch budget), row `number` of a
table of N_TRIALS rows.  Every column of the table is a pool of values, each about equally often, in an order shuffled under a seed of the
column's own; a trial is reproduced by its number.

The composition: the cut is max_occ, or occ_ref's with max_occ as its ceiling; the rescue classifies against that cut
(rescue_ref); the anchors of both are chained at the look-back asked for (overlap_ref); the core mask selects from the unmasked result
(core_cases.filter_rows / filter_pairs); find_overlap_pairs pairs the unmasked rows (api.pair_rows), extends the primaries (extend_ref) and is
masked last.  The underscored switches of reference() / expected_pairs() are not part of it: they make the wrong compositions the host test
holds it against."""
from __future__ import annotations

import functools

import numpy as np

import core_cases as CC
import extend_ref as E
import lookback_cases as L
import lowcomplexity as LC
import overlap_ref as R
import pair_cases as PC
import rescue_cases as RC
import rescue_ref as RR
from herro_amd import api

N_TRIALS = 48
SEED = 220                                          # (a seed at which the table meets every condition of tests/test_combo_host.py with a margin)
PPM = 100_000
MIN_SCORE = {15: 60, 25: 100}                       # by k: low enough for chains inside a repeat of a kilobase

# ---- the pools: a value occurs as often as it is listed, the pool is repeated to N_TRIALS ---------------------------------------------------
GENERATED = {"G7": (7, 120, 31), "G20": (20, 30, 32), "G40": (40, 30, 33), "G150": (150, 8, 34)}      # name -> (unit, copies, seed)
SETS = (["T1"] * 3 + ["T0+T2"] * 4 + ["T3"] * 4 + ["T2+T3"] * 3 + ["streaks"] * 3 + ["set_a"] * 3 + ["set_b"] * 3 + ["B"] * 3 + ["C"] * 2 + ["D"] * 3
        + ["G7"] * 5 + ["G20"] * 4 + ["G40"] * 4 + ["G150"] * 4)
KW = [(15, 5), (25, 17)]
MAX_OCC = [8, 20, 64]
FRAC = [0, PPM]
RESCUE = [None, (100, None), (50, 200)]             # (occ_dist, rescue_max_occ); None: off
LOOKBACK = [64, 128, 256, 1024]
CORE = [None, "alternate", "one", None, "alternate", "empty"]       # every other read, read n // 2, no read
NARROW = [None, None, dict(bandwidth=40, max_gap=300)]
EXTEND = list(PC.EXTENDS)
BUDGET = [None, 1]                                  # HERRO_OVL_SCRATCH_MB
COLUMNS = dict(set=SETS, kw=KW, max_occ=MAX_OCC, ppm=FRAC, rescue=RESCUE, lookback=LOOKBACK, core=CORE, narrow=NARROW, extend=EXTEND, budget=BUDGET)


@functools.lru_cache(maxsize=None)
def _table() -> dict:
    out = {}
    for i, (name, pool) in enumerate(COLUMNS.items()):
        col = [pool[j % len(pool)] for j in range(N_TRIALS)]
        order = np.random.default_rng([SEED, i]).permutation(N_TRIALS)
        out[name] = [col[j] for j in order]
    return out


def trial(number: int) -> dict:
    """the trial of a number in 0 .. N_TRIALS - 1: set, fkw (the finder's keywords without occ_frac_ppm), ppm, rescue, lookback, core (a
    name of CORE), extend (a member of pair_cases.EXTENDS), budget (HERRO_OVL_SCRATCH_MB or None)"""
    t = {name: col[number] for name, col in _table().items()}
    k, w = t["kw"]
    if t["set"] == "set_a" and t["max_occ"] == 64:
        t["max_occ"] = 16                           # 40 reads of one genome: at 64 nothing is cut and the reference chains 389 000 anchors
    if t["set"] in ("set_a", "set_b") and t["extend"] == {}:
        t["extend"] = EXTEND[1]                     # hundreds of pairs: the full extension costs the numpy reference seconds
    fkw = dict(k=k, w=w, max_occ=t["max_occ"], min_score=MIN_SCORE[k], **(t["narrow"] or {}))
    return dict(number=number, set=t["set"], fkw=fkw, ppm=t["ppm"], rescue=t["rescue"], lookback=t["lookback"], core=t["core"], narrow=t["narrow"] is not None,
                extend=t["extend"], budget=t["budget"])


def trials() -> list:
    return [trial(n) for n in range(N_TRIALS)]


def tag(t: dict) -> str:
    return (f"trial {t['number']}: {t['set']} k={t['fkw']['k']} max_occ={t['fkw']['max_occ']} ppm={t['ppm']} rescue={t['rescue']} lookback={t['lookback']} "
            f"core={t['core']} narrow={t['narrow']} extend={t['extend']} budget={t['budget']}")


# the option kinds a trial has switched on (every pair of them meets in at least four trials: tests/test_combo_host.py)
KINDS = dict(k25=lambda t: t["fkw"]["k"] == 25, frac=lambda t: t["ppm"] != 0, rescue=lambda t: t["rescue"] is not None, far=lambda t: t["lookback"] > 64,
             core=lambda t: t["core"] is not None, narrow=lambda t: t["narrow"], extend=lambda t: t["extend"] != {}, budget=lambda t: t["budget"] is not None)


# ---- the read sets ----------------------------------------------------------------------------------------------------------------------------
def generated(unit: int, copies: int, seed: int) -> PC.Reads:
    """two genomes of 700 random bp + a unit of its own x copies + 700 random bp, five reads of each on alternating strands with 3 %
    substitutions; then a read too short to sketch and a read of the first genome with non-ACGT bytes"""
    rng = np.random.default_rng(seed)
    rd = []
    for gi in range(2):
        g = LC._rand(rng, 700) + LC._rand(rng, unit) * copies + LC._rand(rng, 700)
        for i in range(5):
            r = RC._mutate(rng, g, 0.03)
            rd.append(LC.rc(r) if i % 2 else r)
        if gi == 0:
            first = g
    n = bytearray(RC._mutate(rng, first, 0.03))
    for at in (5, 640, 641, 642, 900, len(n) - 3):
        n[at] = ord("N")
    n[1300] = ord("R")
    return PC.Reads(rd + [LC._rand(rng, 17), bytes(n)])


@functools.lru_cache(maxsize=None)
def reads(name: str):
    """(seq u8, qual u8, off u64, codes) of a set: Context.set_reads' arguments and the references'"""
    if name in GENERATED:
        rs = generated(*GENERATED[name])
    elif name in RC.SETS:
        rs = RC.get(name)[0]
    elif name in ("B", "C", "D"):
        rs = dict((n, m) for n, m, _ in PC.SETS)[name]()
    else:
        return L.store(tuple(name.split("+")))
    return rs.seq, rs.qual, rs.off, [R.store_codes(bytes(r)) for r in rs.reads]


def mask(name: str | None, n: int):
    """the core mask of a name of CORE for a store of n reads (None: no mask)"""
    if name is None:
        return None
    m = np.zeros(n, np.uint8)
    if name == "alternate":
        m[0::2] = 1
    elif name == "one":
        m[n // 2] = 1
    return m


# ---- the composed reference -------------------------------------------------------------------------------------------------------------------
_REF = {}


def reference(t: dict, lookback: int | None = None, rescue="asked", _lookback_64: bool = False, _band_from_max_occ: bool = False):
    """the unmasked result of a trial's finder call: ((rids, rows, aln_off, scores), stats) of rescue_ref.find_overlaps_rescue — which is
    occ_ref's and overlap_ref's where the rescue is off.  lookback / rescue: the same trial at another look-back, or with another rescue
    (None: off).  Computed once per process and argument set; nobody writes into the result."""
    H = t["lookback"] if lookback is None else lookback
    resc = t["rescue"] if rescue == "asked" else rescue
    key = (t["set"], tuple(sorted(t["fkw"].items())), t["ppm"], resc, H, _lookback_64, _band_from_max_occ)
    if key not in _REF:
        st = {}
        d, rmax = resc or (0, None)
        got = RR.find_overlaps_rescue(reads(t["set"])[3], d, rmax, t["ppm"], stats=st, lookback=H, _lookback_64=_lookback_64,
                                      _band_from_max_occ=_band_from_max_occ, **t["fkw"])
        _REF[key] = (got, st)
    return _REF[key]


_ANCHORS = {}


def anchors(t: dict):
    """(the reference's anchors of a trial, int64 [n, 5] as overlap_ref.anchors sorts them — the rescue's included —, cut, rescued minimizers)"""
    k, w = t["fkw"]["k"], t["fkw"]["w"]
    key = (t["set"], k, w, t["fkw"]["max_occ"], t["ppm"], t["rescue"])
    if key not in _ANCHORS:
        codes = reads(t["set"])[3]
        lens = np.array([len(c) for c in codes], np.int64)
        h, rid, pos, strand = R.sketch_store(codes, k, w)
        cut = t["fkw"]["max_occ"]
        if t["ppm"]:
            import occ_ref as OR
            cut = OR.occ_cut(OR.run_counts(h), t["ppm"], cut)
        if t["rescue"] is None:
            a, n = R.anchors(h, rid, pos, strand, lens, k, cut), 0
        else:
            flag = RR.rescue_flags(h, rid, pos, lens, cut, *t["rescue"])[1]
            a, n = RR.anchors_rescue(h, rid, pos, strand, lens, k, cut, flag, t["rescue"][1]), int(flag.sum())
        _ANCHORS[key] = (a, cut, n)
    return _ANCHORS[key]


def group_sizes(t: dict) -> np.ndarray:
    """anchors of every (t, q, rel) chain group of a trial"""
    a = anchors(t)[0]
    if not len(a):
        return np.zeros(0, np.int64)
    return np.diff(np.flatnonzero(np.concatenate([[True], (a[1:, :3] != a[:-1, :3]).any(axis=1), [True]])))


ANCHOR_BYTES = 128          # the finder's scratch per anchor (include/herro_amd.h, "Scratch"); one byte more past look-back 64


def chunks(t: dict, budget_mb: int = 1) -> int:
    """the chunks the finder cuts a trial's call into under a scratch budget: consecutive targets whose anchors fit it, a target with more
    alone; under a mask only the anchors of pairs with a core read count"""
    a = anchors(t)[0]
    n = len(reads(t["set"])[3])
    m = mask(t["core"], n)
    if m is not None and len(a):
        a = a[(m[a[:, 0]] != 0) | (m[a[:, 1]] != 0)]
    per = np.bincount(a[:, 0], minlength=n) if len(a) else np.zeros(n, np.int64)
    want = max((budget_mb << 20) // (ANCHOR_BYTES + (t["lookback"] != 64)), 1)
    acc = out = 0
    for c in per:
        if acc and acc + c > want:
            out, acc = out + 1, 0
        acc += int(c)
    return out + (acc > 0)


def expected_rows(t: dict, ref=None):
    """find_overlaps' (rids, rows, aln_off, scores) of a trial: the unmasked reference under the trial's mask"""
    got = (ref or reference(t))[0]
    m = mask(t["core"], len(reads(t["set"])[3]))
    return got if m is None else CC.filter_rows(*got, m)


_PAIRS = {}


def unmasked_pairs(t: dict, ref=None) -> dict:
    """the fields of the unmasked OverlapPairs handle: the reference's rows paired, the primaries extended by extend_ref"""
    rids, rows, aln_off, scores = (ref or reference(t))[0]
    key = None if ref is not None else (t["set"], tuple(sorted(t["fkw"].items())), t["ppm"], t["rescue"], t["lookback"], repr(t["extend"]))
    if key is not None and key in _PAIRS:
        return _PAIRS[key]
    prim, rec = api.pair_rows(rows, exact_ids=True) if len(rows) else (np.zeros(0, np.int64), np.zeros(0, np.uint32))
    n = len(prim)
    assert 2 * n == len(rows)
    pr = rows[prim].reshape(n, 10)
    if t["extend"] is None or not n:
        ext, ext_sc = np.zeros((n, 4), np.uint32), np.zeros((n, 2), np.int32)
    else:
        pr, ext, ext_sc = E.extend_records(reads(t["set"])[3], pr, **t["extend"])
    f = dict(primaries=pr, chain_scores=scores[prim], ext=ext, ext_scores=ext_sc, rids=rids, aln_off=aln_off, rec_of_row=rec)
    if key is not None:
        _PAIRS[key] = f
    return f


def expected_pairs(t: dict, ref=None, _targets_only: bool = False) -> dict:
    """find_overlap_pairs' fields of a trial: unmasked_pairs under the trial's mask"""
    f = unmasked_pairs(t, ref)
    m = mask(t["core"], len(reads(t["set"])[3]))
    return f if m is None else CC.filter_pairs(f, m, _targets_only)


def same_rows(a, b) -> bool:
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def same_pairs(a: dict, b: dict) -> bool:
    return all(np.asarray(a[f]).shape == np.asarray(b[f]).shape and np.array_equal(a[f], b[f]) for f in PC.FIELDS)
