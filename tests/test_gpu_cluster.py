"""gpu: the clusters of the overlap graph on the device (herro_cluster_graph, herro_pairs_cluster; csrc/cluster_dev.hip).  Every handle is
compared field for field with tests/cluster_ref.py — comp, level, rank, part, every part's mask, all statistics — on the hand graphs and the seeded
graphs of tests/cluster_cases.py, on the shapes where the kernels take another path (more levels than one batch between two reads of the frontier
counter, a hub above the wave threshold, the sort's tile of 2 048), and from reads: the handle of a finder call equals the one over its primaries
read back, and the shards of shard.cluster_masks correct the same records as those of shard.core_masks and as one unsharded pass."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cluster_cases as CC  # noqa: E402
import cluster_ref as CR  # noqa: E402
import gpu_common as G  # noqa: E402
import pair_cases as PC  # noqa: E402
from herro_amd import api, shard  # noqa: E402

pytestmark = pytest.mark.gpu

FIELDS = ("comp", "level", "rank", "part")
_GENOME = {}


def _run(c, g):
    return c.cluster_graph(g["n"], g["a"], g["b"], g["n_parts"], weights=g["w"], span=g["span"], min_span=g["min_span"])


def _same_as_ref(cl, want, tag):
    assert (cl.n_parts, cl.n_reads) == (want.n_parts, len(want.part)), tag
    for f in FIELDS:
        got = getattr(cl, f)
        assert got.dtype == np.uint32 and np.array_equal(got, getattr(want, f)), (tag, f)
    assert cl.stats == want.stats, (tag, cl.stats, want.stats)
    assert np.array_equal(cl.part_stats, want.part_stats), (tag, cl.part_stats[:8], want.part_stats[:8])
    for p in range(cl.n_parts):
        assert np.array_equal(cl.mask(p), want.masks[p]), (tag, p)


def _bytes(cl):
    return b"".join(getattr(cl, f).tobytes() for f in FIELDS) + cl.part_stats.tobytes() + repr(cl.stats).encode() + \
        b"".join(cl.mask(p).tobytes() for p in range(min(cl.n_parts, 8)))


def _check(g, tag):
    c = G.ctx()
    cl = _run(c, g)
    _same_as_ref(cl, CR.cluster(**g), tag)
    cl.close()


def _genome(shortcuts):
    if shortcuts not in _GENOME:
        _GENOME[shortcuts] = CC.genome_graph(11, 3000, 3, shortcuts)[0]
    return _GENOME[shortcuts]


# ---- 1. the hand graphs -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CC.hand_graphs()))
def test_hand_graphs(name):
    _check(CC.hand_graphs()[name], name)


def test_a_neighbour_pair_that_is_all_ones_in_the_sorted_bytes_counts_once():
    """n = 65 536, k = 256: (part 255, read 65535) fills every byte the neighbour sort looks at; it must not be taken for an arc inside a part"""
    g = CC.all_ones_key_graph()
    want = CR.cluster(**g)
    assert want.part[65535] == 0 and want.part[65400] == want.part[65401] == 255
    assert want.part_stats[255].tolist() == [256, 256, 1, 2, 4] and want.part_stats[0, 2] == 2 and want.stats["edge_cut"] == 2
    c = G.ctx()
    cl = _run(c, g)
    _same_as_ref(cl, want, "all_ones_key 65536")
    cl.close()


def test_no_reads_at_all():
    c = G.ctx()
    cl = c.cluster_graph(0, [], [], 3)
    assert (cl.n_parts, cl.n_reads) == (3, 0) and not cl.part_stats.any() and cl.stats == dict.fromkeys(api.CLUSTER_STATS, 0)
    assert len(cl.mask(2)) == 0
    cl.close()


# ---- 2. read-overlap graphs without reads ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shortcuts", [0, 20])
@pytest.mark.parametrize("k", [1, 2, 3, 8, 3007])
def test_genome_graphs_equal_the_reference_and_themselves(shortcuts, k):
    g = dict(_genome(shortcuts), n_parts=k)
    c = G.ctx()
    want = CR.cluster(**g)
    first = _run(c, g)
    _same_as_ref(first, want, (shortcuts, k))
    second = _run(c, g)                       # run twice: the bytes are identical
    assert _bytes(first) == _bytes(second)
    weight = first.part_stats[:, 1].astype(np.int64)
    assert (np.abs(weight * k - int(g["w"].sum())) < int(g["w"].max()) * k).all()
    assert int(first.part_stats[:, 4].sum()) == len(g["a"]) + first.stats["edge_cut"]
    first.close()
    second.close()


def test_min_span_at_its_boundary_on_a_genome_graph():
    g = _genome(20)
    s = int(np.sort(g["span"])[len(g["span"]) // 3])          # a span that occurs: edges with exactly it are strong, at s + 1 they are weak
    assert (g["span"] == s).any()
    strong = []
    for ms in (s, s + 1):
        gg = dict(g, n_parts=3, min_span=ms)
        c = G.ctx()
        cl = _run(c, gg)
        _same_as_ref(cl, CR.cluster(**gg), ("min_span", ms))
        strong.append(cl.stats["strong_edges"])
        cl.close()
    assert strong[0] - strong[1] == int((g["span"] == s).sum()) > 0


# ---- 3. where the kernels take another path ---------------------------------------------------------------------------------------------
def test_a_path_of_3000_needs_many_batches_of_levels():
    g = CC.path_graph(3000, 3)
    want = CR.cluster(**g)
    assert want.stats["n_levels"] == 3000 and want.stats["n_components"] == 1       # 47 batches of 64 levels per sweep
    c = G.ctx()
    cl = _run(c, g)
    _same_as_ref(cl, want, "path3000")
    cl.close()


def test_a_hub_with_3000_neighbours():
    """more arcs than a wave, a block and a sort tile of 2 048 on one vertex; the frontier grows 1 -> 3 000 (from a leaf: 1 -> 1 -> 2 999)"""
    g = CC.star_graph(3000, 4)
    want = CR.cluster(**g)
    assert want.stats["n_levels"] == 3 and want.level[1500] == 1
    c = G.ctx()
    cl = _run(c, g)
    _same_as_ref(cl, want, "star3000")
    cl.close()
    # hubs of 32, 33 (the threshold between a thread and a wave), 64 and 65 neighbours side by side, all in one frontier
    edges, n = [], 0
    for leaves in (32, 33, 64, 65, 200):
        edges += [(n, n + 1 + i) for i in range(leaves)]
        n += leaves + 1
    g = CC.case(n, edges, 5, w=np.arange(n) % 7)
    _check(g, "hubs")


def test_half_a_million_reads_without_an_edge_pass_the_seam_of_the_scan():
    """n = 256 * 2048 + 1: the order sort's keys and the weight prefix both take k_scan_top (scan_sort_dev.hip) into its second round; without an edge
    the order is the ids, so every field shows where the sort or the scan slipped"""
    g = CC.edge_free_graph()
    assert g["n"] == CC.SCAN_SEAM + 1 == 524289 and g["n_parts"] == 7 and len(g["a"]) == 0 and int(g["w"].sum()) < 1 << 32
    want = CR.cluster(**g)
    assert np.array_equal(want.rank, np.arange(g["n"])) and want.stats["n_components"] == g["n"] and want.part[-1] == 6
    c = G.ctx()
    cl = _run(c, g)
    _same_as_ref(cl, want, "edge_free 524289")
    cl.close()


def test_more_parts_than_the_edge_statistics_hold_in_lds():
    """k = 1025: k_cl_edge_stats sums up to 1 024 parts in LDS first and goes to global atomics above"""
    g = dict(_genome(20), n_parts=1025)
    want = CR.cluster(**g)
    assert (want.part_stats[:, 0] > 0).sum() > 1000 and want.stats["edge_cut"] > 0 and int(want.part_stats[:, 3].sum()) > 0
    c = G.ctx()
    cl = _run(c, g)
    _same_as_ref(cl, want, "genome k=1025")
    cl.close()


# ---- 4. from reads, W = 256 -------------------------------------------------------------------------------------------------------------------
W = 256
READS = [("A", dict(max_occ=64, min_score=200)), ("B", PC.DEFAULTS)]
_SETS = {}


def _ctx_with(name):
    if name not in _SETS:
        _SETS[name] = dict((n, m) for n, m, _ in PC.SETS)[name]()
    c = G.ctx()
    PC.load(c, _SETS[name])
    return c, np.diff(np.asarray(_SETS[name].off).astype(np.int64))


def _edges(pairs):
    p = pairs.primaries.astype(np.int64)
    return p[:, 5], p[:, 0], np.minimum(p[:, 8] - p[:, 7], p[:, 3] - p[:, 2])


@pytest.mark.parametrize("name,kw", READS)
def test_the_handle_of_a_finder_call_equals_the_graph_of_its_primaries(name, kw):
    c, lens = _ctx_with(name)
    pairs = c.find_overlap_pairs(extend=False, **kw)
    a, b, span = _edges(pairs)
    assert pairs.n_pairs > 0
    w = shard.windows_of(lens, W).astype(np.uint32)
    ms = int(np.median(span))
    for k, min_span in ((3, 0), (3, ms), (2, ms + 1), (8, int(span.max()) + 1)):
        cl = pairs.cluster(k, weights=w, min_span=min_span)
        via = c.cluster_graph(len(lens), a, b, k, weights=w, span=span, min_span=min_span)
        assert _bytes(cl) == _bytes(via), (name, k, min_span)
        _same_as_ref(cl, CR.cluster(len(lens), w, a, b, span, k, min_span), (name, k, min_span))
        cl.close()
        via.close()
    cl = pairs.cluster(3)                                      # no weights: all 1
    _same_as_ref(cl, CR.cluster(len(lens), None, a, b, span, 3, 0), (name, "unit weights"))
    pairs.close()                                              # the pairs go before the clusters: the handle keeps its own graph
    assert np.array_equal(cl.mask(1), CR.cluster(len(lens), None, a, b, span, 3, 0).masks[1])
    cl.close()


def _records(rec):
    rids, ends, text = rec
    text, ends = bytes(text), np.concatenate([[0], np.asarray(ends).astype(np.int64)])
    return {int(r): text[ends[i]:ends[i + 1]] for i, r in enumerate(rids)}


@pytest.mark.parametrize("name,kw", READS)
def test_the_shards_of_cluster_masks_correct_what_core_masks_and_one_pass_correct(name, kw):
    c, lens = _ctx_with(name)
    read_name = lambda r: f"read{r}"
    whole = _records(shard.correct_reads_shard(c, np.ones(len(lens), np.uint8), W, 64, 0, read_name, **kw))
    assert len(whole) > 0
    by_windows = shard.core_masks(lens, W, 3)
    by_overlaps, cl = shard.cluster_masks(c, lens, W, 3, **kw)
    assert len(by_overlaps) == 3 and np.array_equal(np.sum(by_overlaps, 0), np.ones(len(lens)))
    assert all(m.dtype == np.uint8 and m.shape == by_windows[0].shape for m in by_overlaps)
    for masks in (by_windows, by_overlaps):
        got = _records(shard.merge_records([shard.correct_reads_shard(c, m, W, 64, 0, read_name, **kw) for m in masks]))
        assert got == whole, name
    # what the ranks align: pairs with at least one end in the part, summed = E + edge_cut
    pairs = c.find_overlap_pairs(extend=False, **kw)
    a, b, _ = _edges(pairs)
    pairs.close()
    part_w = np.zeros(len(lens), np.int64)
    for p, m in enumerate(by_windows):
        part_w[m != 0] = p
    touching_windows = len(a) + int((part_w[a] != part_w[b]).sum())
    touching_overlaps = int(cl.part_stats[:, 4].sum())
    print(f"set {name}: pairs {len(a)}, sum of pairs_touching by windows {touching_windows}, by overlaps {touching_overlaps}")
    assert touching_overlaps == len(a) + cl.stats["edge_cut"]
    assert touching_overlaps < touching_windows
    cl.close()


def test_correct_reads_sharded_takes_either_partition():
    """one rank: both partitions make every read core, and the records are those of one unsharded pass"""
    c, lens = _ctx_with("A")
    kw = dict(max_occ=64, min_score=200)
    read_name = lambda r: f"read{r}"
    whole = _records(shard.correct_reads_shard(c, np.ones(len(lens), np.uint8), W, 64, 0, read_name, **kw))
    for partition in ("windows", "overlaps"):
        rec, n_mine = shard.correct_reads_sharded(c, lens, W, 64, 0, read_name, partition=partition, **kw)
        assert n_mine == len(lens) and _records(rec) == whole, partition
    with pytest.raises(ValueError):
        shard.correct_reads_sharded(c, lens, W, 64, 0, read_name, partition="metis", **kw)


# ---- 5. handles ---------------------------------------------------------------------------------------------------------------------------------
def test_a_pairs_handle_of_another_context_is_refused():
    c, lens = _ctx_with("D")
    other = api.Context(0)
    try:
        PC.load(other, _SETS["D"])
        p_other = other.find_overlap_pairs(extend=False, **PC.DEFAULTS)
        h, P = C.c_void_p(), api.ClusterParams(n_parts=2)
        assert c._l.herro_pairs_cluster(c.h, p_other.h, None, C.byref(P), C.byref(h)) == -1 and not h.value
        assert "herro_pairs_cluster: the pairs handle belongs to another context" in c.last_error()
        cl = p_other.cluster(2)                                # on its own context it works
        assert cl.n_reads == len(lens) and int(cl.part_stats[:, 0].sum()) == len(lens)
        with pytest.raises(api.HerroError) as e:
            cl.mask(2)
        assert e.value.code == -1 and "herro_clusters_mask: part 2 of 2" in str(e.value)
        p_other.close()
        cl.close()
    finally:
        other.close()
