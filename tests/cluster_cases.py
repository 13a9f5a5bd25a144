"""Graphs for the cluster tests (tests/cluster_ref.py is the specification): the hand graphs with answers that can be derived on paper, and a
seeded generator of read-overlap graphs that needs no reads.  A case is a dict of cluster_ref.cluster's keywords."""
from __future__ import annotations

import numpy as np

from scan_sort_cases import SCAN_SEAM     # elements above which the scan under cl_build (scan_sort_dev.hip: k_scan_top) runs a second round


def case(n, edges, k, w=None, span=None, min_span=0):
    e = np.asarray(edges, np.uint32).reshape(-1, 2)
    return dict(n=n, w=None if w is None else np.asarray(w, np.uint32), a=e[:, 0].copy(), b=e[:, 1].copy(),
                span=None if span is None else np.asarray(span, np.uint32), n_parts=k, min_span=min_span)


# a path of 7 with shuffled ids: 3 - 5 - 0 - 6 - 2 - 4 - 1.  comp = 0 everywhere; d1 from 0: 3:2 5:1 0:0 6:1 2:2 4:3 1:4, so far = 1 and the order is
# the path from that end: 1 4 2 6 0 5 3.
PATH7 = [3, 5, 0, 6, 2, 4, 1]
PATH7_ORDER = [1, 4, 2, 6, 0, 5, 3]


def hand_graphs() -> dict:
    g = {}
    g["path7"] = case(7, [(PATH7[i], PATH7[i + 1]) for i in range(6)], 3)
    # 0 in the middle of 2 - 1 - 0 - 3 - 4 ... both ends (2 and 4) at distance 2: far = 2, the least id
    g["tie_far"] = case(5, [(2, 1), (1, 0), (0, 3), (3, 4)], 2)
    g["single"] = case(1, [], 1)
    g["single_k4"] = case(1, [], 4)
    g["no_edges"] = case(5, [], 2)
    g["two_components"] = case(7, [(0, 2), (2, 4), (4, 6), (1, 3), (3, 5)], 2)
    g["k1"] = case(6, [(0, 1), (1, 2), (3, 4)], 1)
    g["k_gt_n"] = case(3, [(0, 1), (1, 2)], 7)
    g["weights"] = case(6, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)], 3, w=[0, 4000000000, 0, 5, 0, 294967290])   # T = 2^32 - 1
    g["t_zero"] = case(4, [(0, 1), (2, 3)], 3, w=[0, 0, 0, 0])
    # span == min_span is strong, min_span - 1 is weak: 0 - 1 strong, 1 - 2 weak, 2 - 3 strong
    g["span_boundary"] = case(4, [(0, 1), (1, 2), (2, 3)], 2, span=[500, 499, 500], min_span=500)
    # the weak edge 1 - 4 joins two strong paths: it shows in the masks and in edge_cut, not in comp or level
    g["weak_edge"] = case(6, [(0, 1), (1, 2), (3, 4), (4, 5), (1, 4)], 2, span=[9, 9, 9, 9, 1], min_span=5)
    g["dup_reversed"] = case(5, [(0, 1), (1, 0), (0, 1), (3, 2), (2, 3), (4, 3), (1, 2)], 2)
    # components whose root is their far vertex: the isolated reads 0, 3, 7 among two paths
    g["root_is_far"] = case(8, [(1, 2), (4, 5), (5, 6)], 3)
    g["min_span_zero"] = case(3, [(0, 1), (1, 2)], 2, span=[0, 7], min_span=0)
    # read 255 = n - 1 is the far vertex of component 0 and alone in part 0 (the only weight), every other read is in part 255 = k - 1: the pair
    # (part 255, neighbour 255) is all ones in every byte a sort over 8 bits of id and 8 bits of part looks at, and it occurs twice with an arc
    # inside part 255 between its occurrences.  Read 255 is one neighbour of part 255, and read 0 the one neighbour of part 0.
    w = np.zeros(256, np.uint32)
    w[255] = 1
    g["all_ones_key"] = case(256, [(0, 255), (1, 2), (0, 255)], 256, w=w)
    return g


def all_ones_key_graph():
    """the same at 16 bits of id: 65 536 reads of weight 1 in 256 parts.  The strong edge 0 - 65535 makes read 65535 the first of the order (part 0);
    its weak edges to 65400 and 65401 (part 255) make it a neighbour of part 255 twice over, with an edge inside part 255 between them."""
    return case(65536, [(0, 65535), (65535, 65400), (65300, 65301), (65401, 65535), (65500, 65501)], 256, span=[9, 1, 9, 1, 1], min_span=5)


def path_graph(n: int, k: int, seed: int = 5):
    """a path of n vertices with shuffled ids: n - 1 levels"""
    ids = np.random.default_rng(seed).permutation(n)
    return case(n, np.stack([ids[:-1], ids[1:]], 1), k)


def star_graph(leaves: int, k: int):
    """hub `leaves` // 2 with `leaves` neighbours"""
    hub = leaves // 2
    others = np.array([v for v in range(leaves + 1) if v != hub])
    return case(leaves + 1, np.stack([np.full(leaves, hub), others], 1), k)


def edge_free_graph(n: int = SCAN_SEAM + 1, k: int = 7, seed: int = 14):
    """n reads without an edge, weights 0 .. 4095 (T below 2^32 up to a million reads): the sort of the n order keys and the scan of the n weights
    are the only work, and at the default n both pass the seam of the scan.  (cluster_ref.cluster takes two seconds for it: no closed form is needed.)"""
    return case(n, [], k, w=np.random.default_rng(seed).integers(0, 4096, n))


def genome_graph(seed: int, n: int, chromosomes: int, shortcuts: int, chrom_len: int = 1_000_000, min_overlap: int = 2000):
    """n reads of 10 - 40 kb placed uniformly on `chromosomes` chromosomes of chrom_len bases, in random id order; an edge wherever two reads of
    one chromosome share at least min_overlap bases, its span the shared length; weights ceil(len / 4096) (windows per read).  shortcuts: that
    many more edges between random reads, spans of 3 - 6 kb: what a repeat that survives min_span looks like.  Returns (case without n_parts,
    read start positions on the concatenated genome)."""
    rng = np.random.default_rng(seed)
    length = rng.integers(10_000, 40_001, n)
    chrom = rng.integers(0, chromosomes, n)
    start = rng.integers(0, chrom_len - length + 1)
    edges, spans = [], []
    for c in range(chromosomes):
        ids = np.flatnonzero(chrom == c)
        ids = ids[np.argsort(start[ids], kind="stable")]
        s, e = start[ids], start[ids] + length[ids]
        for i in range(len(ids)):
            j = i + 1
            while j < len(ids) and s[j] + min_overlap <= e[i]:
                ov = min(e[i], e[j]) - s[j]
                if ov >= min_overlap:
                    edges.append((ids[i], ids[j]))
                    spans.append(ov)
                j += 1
    for _ in range(shortcuts):
        x, y = rng.choice(n, 2, replace=False)
        edges.append((x, y))
        spans.append(int(rng.integers(3000, 6001)))
    g = case(n, edges, 1, w=(length + 4095) // 4096, span=spans, min_span=min_overlap)
    return g, chrom * chrom_len + start
