"""The read sets of the pair-overlap tests (tests/test_pairs_host.py, tests/test_gpu_pairs.py) and the stepwise chain their results are
held to.  All sets are seeded and small.

A  synth.generate(2, 3000, 5, ...): 12 reads, every read of a genome overlaps the others.
B  lowcomplexity.working_set(): 24 low-complexity reads; at k = 15, w = 5 the finder has 35 654 anchors (several chunks at 1 MiB).
C  lowcomplexity.palindromic_pair: the two strands of the one pair tie exactly.
D  pairs that chain on BOTH strands with unequal scores (neither A nor B has one), a plain forward and a plain reverse pair, a read
   too short to sketch and an unrelated read.
E  three reads that share nothing: no pair at all."""
import numpy as np

import lowcomplexity as LC
import overlap_ref as R
from herro_amd import api, synth

DEFAULTS = dict(max_occ=64, min_score=100)
SMALL_K = dict(k=15, w=5, max_occ=64, min_score=60)
HIGH_SCORE = dict(max_occ=64, min_score=1000)
EXTENDS = (dict(), dict(zdrop=30, max_ext=50), None)        # extend_overlaps' keywords; None: HERRO_PAIRS_NO_EXTEND

# what set D's chains are at the seed below: (t, q, rel) -> score
D_CHAINS_DEFAULTS = {(0, 1, 0): 1477, (0, 1, 1): 891, (2, 3, 0): 883, (2, 3, 1): 1487, (4, 5, 0): 1890, (6, 7, 1): 1889}
D_BOTH_SMALL_K = {(0, 1, 0): 1499, (0, 1, 1): 895, (2, 3, 0): 897, (2, 3, 1): 1497}


class Reads:
    """ASCII reads as Context.set_reads takes them"""

    def __init__(self, reads):
        self.reads = list(reads)
        self.seq = np.frombuffer(b"".join(self.reads), np.uint8)
        self.qual = np.full(len(self.seq), 40 + 33, np.uint8)
        self.off = np.concatenate([[0], np.cumsum([len(r) for r in self.reads])]).astype(np.uint64)
        self.lens = np.array([len(r) for r in self.reads], np.uint32)

    def codes(self):
        return [R.store_codes(r) for r in self.reads]


def set_a(W=256):
    sb = synth.generate(2, 3000, 5, seed=231 + W, flank_min=100, flank_max=300)
    assert sb.n_reads == 12
    return sb


def set_b():
    return LC.working_set()


def set_c():
    return Reads(LC.palindromic_pair(np.random.default_rng(13)))


def set_d():
    rng = np.random.default_rng(5)
    rd = []
    for xl, yl in ((1500, 900), (900, 1500)):               # a forward stretch of xl and a reverse stretch of yl bases of the same target
        t = LC._rand(rng, 3000)
        rd += [t, t[200:200 + xl] + LC._rand(rng, 60) + LC.rc(t[300 + xl:300 + xl + yl])]
    t = LC._rand(rng, 2500)
    rd += [t, t[300:2200]]
    t = LC._rand(rng, 2500)
    rd += [t, LC.rc(t[300:2200])]
    rd += [LC._rand(rng, 30), LC._rand(rng, 2000)]
    return Reads(rd)


def set_e():
    rng = np.random.default_rng(6)
    return Reads([LC._rand(rng, 30), LC._rand(rng, 2000), LC._rand(rng, 2000)])


# (name, maker, the finder's parameter sets it runs with)
SETS = [
    ("A", set_a, (DEFAULTS, SMALL_K, dict(max_occ=64, min_score=200))),
    ("B", set_b, (DEFAULTS, SMALL_K)),
    ("C", set_c, (DEFAULTS, SMALL_K)),
    ("D", set_d, (DEFAULTS, SMALL_K, HIGH_SCORE)),
    ("E", set_e, (DEFAULTS, SMALL_K)),
]


def load(c, rs):
    c.set_reads(rs.seq, rs.qual, rs.off)


def stepwise(c, ext, **kw):
    """find_overlaps -> pair_rows -> extend_overlaps(rows[prim]): the fields an OverlapPairs handle must equal, by name"""
    rids, rows, aln_off, scores = c.find_overlaps(**kw)
    prim, rec_of_row = api.pair_rows(rows, exact_ids=True)
    assert 2 * len(prim) == len(rows)
    n = len(prim)
    if ext is None:
        rows_e, ex, ex_sc = rows[prim].reshape(n, 10), np.zeros((n, 4), np.uint32), np.zeros((n, 2), np.int32)
    else:
        rows_e, ex, ex_sc = c.extend_overlaps(rows[prim].reshape(n, 10), **ext)
    return dict(primaries=rows_e, chain_scores=scores[prim], ext=ex, ext_scores=ex_sc, rids=rids, aln_off=aln_off, rec_of_row=rec_of_row)


FIELDS = ("primaries", "chain_scores", "ext", "ext_scores", "rids", "aln_off", "rec_of_row")


def pairs_fields(p):
    return {f: getattr(p, f) for f in FIELDS}


def pairs_bytes(p):
    return b"|".join(np.ascontiguousarray(getattr(p, f)).tobytes() for f in FIELDS)


def assert_same_fields(got, want, tag):
    for f in FIELDS:
        g, w = np.asarray(got[f]), np.asarray(want[f])
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (tag, f, g.shape, w.shape)
