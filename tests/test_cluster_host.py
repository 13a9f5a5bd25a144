"""not-gpu: the specification of the clusters (tests/cluster_ref.py; include/herro_amd.h, "clusters") against answers derived by hand,
its properties on seeded graphs, its quality against the partition by window counts, the cluster-file format, and the argument checks of
herro_cluster_graph / herro_pairs_cluster through a device-free context.  The kernels are held to the same reference in tests/test_gpu_cluster.py."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cluster_cases as CC  # noqa: E402
import cluster_ref as CR  # noqa: E402
from herro_amd import api, io, shard  # noqa: E402

H = CC.hand_graphs()


def _ref(name):
    return CR.cluster(**H[name])


# ---- 1. hand-derived answers ----------------------------------------------------------------------------------------------------------------
def test_path_of_7_is_ordered_from_its_far_end():
    r = _ref("path7")
    assert r.comp.tolist() == [0] * 7
    order = np.argsort(r.rank).tolist()
    assert order == CC.PATH7_ORDER and r.level[order].tolist() == list(range(7))
    # T = 7, k = 3: S * 3 // 7 for S = 0 .. 6
    assert r.part[order].tolist() == [0, 0, 0, 1, 1, 2, 2]
    assert r.stats == {"n_components": 1, "n_levels": 7, "strong_edges": 6, "edge_cut": 2}
    assert r.part_stats.tolist() == [[3, 3, 1, 2, 3], [2, 2, 2, 1, 3], [2, 2, 1, 1, 2]]
    assert r.masks[1][order].tolist() == [0, 0, 2, 1, 1, 2, 0]


def test_two_vertices_tied_for_farthest_give_the_least_id():
    r = _ref("tie_far")                       # 2 - 1 - 0 - 3 - 4: far = 2
    assert r.level.tolist() == [2, 1, 0, 3, 4] and np.argsort(r.rank).tolist() == [2, 1, 0, 3, 4]
    assert r.part.tolist() == [0, 0, 0, 1, 1]          # S = 0 .. 4 in the order 2 1 0 3 4, * 2 // 5


def test_single_vertex_no_edges_and_more_parts_than_reads():
    for name in ("single", "single_k4"):
        r = _ref(name)
        assert (r.comp.tolist(), r.level.tolist(), r.rank.tolist(), r.part.tolist()) == ([0], [0], [0], [0])
        assert r.stats == {"n_components": 1, "n_levels": 1, "strong_edges": 0, "edge_cut": 0}
        assert r.part_stats[0].tolist() == [1, 1, 0, 0, 0] and not r.part_stats[1:].any()
    r = _ref("no_edges")
    assert r.comp.tolist() == list(range(5)) and not r.level.any() and r.rank.tolist() == list(range(5))
    assert r.part.tolist() == [0, 0, 0, 1, 1] and r.stats["n_components"] == 5 and not (r.masks == 2).any()
    r = _ref("k_gt_n")                        # 0 - 1 - 2, far = 2; S * 7 // 3 = 0, 2, 4
    assert np.argsort(r.rank).tolist() == [2, 1, 0] and r.part.tolist() == [4, 2, 0]
    assert r.part_stats[:, 0].tolist() == [1, 0, 1, 0, 1, 0, 0] and r.stats["edge_cut"] == 2
    assert r.masks[1].tolist() == [0, 0, 0] and r.masks[2].tolist() == [2, 1, 2]


def test_two_components_and_one_part():
    r = _ref("two_components")                # 0 - 2 - 4 - 6 and 1 - 3 - 5: far = 6 and 5
    assert r.comp.tolist() == [0, 1, 0, 1, 0, 1, 0]
    assert np.argsort(r.rank).tolist() == [6, 4, 2, 0, 5, 3, 1]
    assert r.part[[6, 4, 2, 0, 5, 3, 1]].tolist() == [0, 0, 0, 0, 1, 1, 1] and r.stats["edge_cut"] == 0 and r.stats["n_levels"] == 4
    r = _ref("k1")
    assert not r.part.any() and r.masks.tolist() == [[1] * 6] and r.part_stats.tolist() == [[6, 6, 0, 3, 3]]
    assert r.stats == {"n_components": 3, "n_levels": 3, "strong_edges": 3, "edge_cut": 0}


def test_zero_and_large_weights():
    r = _ref("weights")                       # a path 0 .. 5, far = 5: order 5 4 3 2 1 0, T = 2^32 - 1
    order = [5, 4, 3, 2, 1, 0]
    assert np.argsort(r.rank).tolist() == order
    w = [294967290, 0, 5, 0, 4000000000, 0]
    S = np.concatenate([[0], np.cumsum(w)])[:-1]
    assert r.part[order].tolist() == [CR.part_of(int(s), 2 ** 32 - 1, 3) for s in S] == [0, 0, 0, 0, 0, 2]   # (the last one clamped: S * k // T = 3 only at S = T)
    assert r.part_stats[:, 1].tolist() == [2 ** 32 - 1, 0, 0]
    r = _ref("t_zero")
    assert not r.part.any() and r.part_stats[0].tolist() == [4, 0, 0, 2, 2]


def test_span_at_min_span_is_strong_and_one_below_is_weak():
    r = _ref("span_boundary")                 # 0 = 1 . 2 = 3
    assert r.comp.tolist() == [0, 0, 2, 2] and r.stats["strong_edges"] == 2 and r.stats["n_components"] == 2
    r0 = CR.cluster(**dict(H["span_boundary"], min_span=499))
    assert r0.comp.tolist() == [0] * 4 and r0.stats["strong_edges"] == 3
    r = _ref("min_span_zero")
    assert r.comp.tolist() == [0] * 3 and r.stats["strong_edges"] == 2


def test_a_weak_edge_shows_in_masks_and_cut_but_not_in_comp_or_level():
    r = _ref("weak_edge")                     # 0 - 1 - 2 and 3 - 4 - 5 strong, 1 . 4 weak
    g = dict(H["weak_edge"])
    without = CR.cluster(g["n"], g["w"], g["a"][:4], g["b"][:4], g["span"][:4], g["n_parts"], g["min_span"])
    for f in ("comp", "level", "rank", "part"):
        assert np.array_equal(getattr(r, f), getattr(without, f)), f
    assert r.comp.tolist() == [0, 0, 0, 3, 3, 3] and r.part.tolist() == [0, 0, 0, 1, 1, 1]
    assert (r.stats["edge_cut"], without.stats["edge_cut"]) == (1, 0) and r.stats["strong_edges"] == 4
    assert r.masks.tolist() == [[1, 1, 1, 0, 2, 0], [0, 2, 0, 1, 1, 1]] and not (without.masks == 2).any()
    assert r.part_stats[:, 4].tolist() == [3, 3] and r.part_stats[:, 3].tolist() == [2, 2]


def test_duplicate_and_reversed_edges_count_as_given():
    r = _ref("dup_reversed")                  # 0 = 1 (three times), 2 = 3 (twice), 3 - 4, 1 - 2: the path 0 1 2 3 4
    once = CR.cluster(5, None, [0, 1, 2, 3], [1, 2, 3, 4], None, 2)
    for f in ("comp", "level", "rank", "part"):
        assert np.array_equal(getattr(r, f), getattr(once, f)), f
    assert np.array_equal(r.masks, once.masks)
    assert r.part.tolist() == [1, 1, 0, 0, 0]              # far = 4: order 4 3 2 1 0
    assert r.stats["strong_edges"] == 7 and r.stats["edge_cut"] == 1 and once.stats["edge_cut"] == 1
    assert r.part_stats[:, 3].tolist() == [3, 3] and r.part_stats[:, 4].tolist() == [4, 4]
    assert r.part_stats[:, 2].tolist() == [1, 1]           # a neighbour counts once however many edges reach it


def test_the_last_read_as_the_neighbour_of_the_last_part():
    r = _ref("all_ones_key")                  # 0 = 255 twice, 1 - 2; only read 255 has weight
    assert r.part[255] == 0 and (r.part[:255] == 255).all() and np.argsort(r.rank)[:2].tolist() == [255, 0]
    assert r.part_stats[0].tolist() == [1, 1, 1, 0, 2] and r.part_stats[255].tolist() == [255, 0, 1, 1, 3] and not r.part_stats[1:255].any()
    assert r.stats == {"n_components": 254, "n_levels": 2, "strong_edges": 3, "edge_cut": 2}   # {0, 255}, {1, 2} and the 252 reads 3 .. 254


def test_roots_that_are_their_own_far_vertex():
    r = _ref("root_is_far")
    assert r.comp.tolist() == [0, 1, 1, 3, 4, 4, 4, 7] and r.level.tolist() == [0, 1, 0, 0, 2, 1, 0, 0]
    assert np.argsort(r.rank).tolist() == [0, 2, 1, 3, 6, 5, 4, 7]


# ---- 2. properties ----------------------------------------------------------------------------------------------------------------------------
def _touching(part, a, b, k):
    pa, pb = part[a], part[b]
    return int(np.bincount(pa, minlength=k).sum() + np.bincount(pb[pa != pb], minlength=k).sum())


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_properties_on_seeded_graphs(seed):
    g, _ = CC.genome_graph(seed, 400, 2, shortcuts=seed)
    E = len(g["a"])
    assert E > 1000
    for k in (1, 3, 8, 401):
        r = CR.cluster(**dict(g, n_parts=k))
        assert r.part.max() < k and sorted(r.rank.tolist()) == list(range(400))
        assert (r.masks == 1).sum(0).tolist() == [1] * 400                        # every read is core in exactly one part
        assert r.part_stats[:, 0].sum() == 400
        T, wmax = int(g["w"].sum()), int(g["w"].max())
        weight = r.part_stats[:, 1].astype(np.int64)
        assert weight.sum() == T and (np.abs(weight * k - T) < wmax * k).all()    # |weight(p) - T / k| < max w
        assert int(r.part_stats[:, 4].sum()) == E + r.stats["edge_cut"] == _touching(r.part.astype(np.int64), g["a"], g["b"], k)
        for p in range(k):
            assert not ((r.masks[p] == 2) & (r.part == p)).any()                  # a neighbour is never core
            assert int((r.masks[p] == 2).sum()) == int(r.part_stats[p, 2])


# ---- 3. quality: a condition on the reference alone ----------------------------------------------------------------------------------------
def test_the_cut_is_a_quarter_of_the_cut_by_window_counts_at_most():
    """3 000 reads on 3 chromosomes, no false edges, 8 parts: the specification cuts 3 966 of 69 681 edges (5.7 %), the partition by window counts
    60 970 (87.5 %), 1/15; the bound of 1/4 leaves room for another seed of the generator.  (The cuts with 3 and 20 shortcuts are in DESIGN.md §14 as
    measured; they are not asserted.)"""
    g, _ = CC.genome_graph(11, 3000, 3, shortcuts=0)
    r = CR.cluster(**dict(g, n_parts=8))
    greedy = np.zeros(3000, np.int64)
    for p, ids in enumerate(shard.partition_targets(g["w"].astype(np.int64), 8)):
        greedy[ids] = p
    a, b = g["a"].astype(np.int64), g["b"].astype(np.int64)
    cut_greedy = int((greedy[a] != greedy[b]).sum())
    print(f"edges {len(a)} cut by window counts {cut_greedy} cut by the specification {r.stats['edge_cut']}")
    assert len(a) > 30000 and cut_greedy > len(a) // 2
    assert 4 * r.stats["edge_cut"] <= cut_greedy


# ---- 4. the cluster file ----------------------------------------------------------------------------------------------------------------------
NAMES = [b"r%d" % i for i in range(8)]
# the fixture: one cluster in the format scripts/create_clusters.py writes and `herro inference -c` reads (lib.rs:208-239) — `0\t<name>` per core read,
# then `1\t<name>` per neighbour — written by hand for the reads r0 .. r7
GOLDEN = os.path.join(HERE, "golden", "cluster_000.part")


def test_cluster_file_round_trip_against_the_fixture(tmp_path):
    mask = np.array([1, 2, 0, 1, 2, 0, 0, 1], np.uint8)
    path = str(tmp_path / "000.part")
    io.write_cluster(path, mask, NAMES)
    assert open(path, "rb").read() == open(GOLDEN, "rb").read() == b"0\tr0\n0\tr3\n0\tr7\n1\tr1\n1\tr4\n"
    assert np.array_equal(io.read_cluster(GOLDEN, NAMES), mask)
    assert np.array_equal(io.read_cluster(GOLDEN, [n.decode() for n in NAMES]), mask)
    r = _ref("weak_edge")                                   # a reference mask through the file and back
    io.write_cluster(path, r.masks[0], NAMES[:6])
    assert np.array_equal(io.read_cluster(path, NAMES[:6]), r.masks[0])
    with pytest.raises(ValueError):
        io.write_cluster(path, np.array([1, 3], np.uint8), NAMES[:2])
    with pytest.raises(ValueError):
        io.write_cluster(path, mask, NAMES[:7])


@pytest.mark.parametrize("text,what", [(b"0\tr0\n\n1\tr1\n", "line 2"), (b"2\tr0\n", "line 1"), (b"0 r0\n", "line 1"), (b"0\tr0\n1\n", "line 2"),
                                       (b"0\tr0\n1\tr9\n", "unknown read"), (b"0\tr0\n1\tr0\n", "listed twice"), (b"\n", "line 1")])
def test_malformed_cluster_lines_are_errors(tmp_path, text, what):
    path = str(tmp_path / "bad.part")
    open(path, "wb").write(text)
    with pytest.raises(ValueError) as e:
        io.read_cluster(path, NAMES)
    assert what in str(e.value)


# ---- 5. error codes and messages through a device-free context ------------------------------------------------------------------------------
def _raises(code, text, fn, *args, **kw):
    with pytest.raises(api.HerroError) as e:
        fn(*args, **kw)
    assert e.value.code == code and text in str(e.value), str(e.value)


def test_argument_checks_come_first_then_the_limits_then_the_device():
    c = api.HostContext(np.full(6, 1000, np.uint32))
    a, b = [0, 1, 2], [1, 2, 3]
    for k in (0, 65536, 2 ** 32 - 1):
        _raises(-1, f"herro_cluster_graph: n_parts = {k}: 1 <= n_parts <= 65535", c.cluster_graph, 6, a, b, k)
    _raises(-1, "herro_cluster_graph: edge 2: a == b = 4", c.cluster_graph, 6, [0, 1, 4], [1, 2, 4], 2)
    _raises(-1, "herro_cluster_graph: edge 1: read id 6 outside the 6 reads", c.cluster_graph, 6, [0, 6, 9], [1, 2, 3], 2)
    _raises(-1, "herro_cluster_graph: edge 0: read id 7 outside the 6 reads", c.cluster_graph, 6, [0], [7], 2)
    _raises(-1, "n_parts = 0", c.cluster_graph, 6, [0, 1, 4], [1, 2, 4], 0)                     # the parameters before the edges
    _raises(-4, "herro_cluster_graph: more than 2^31 - 1 reads", c.cluster_graph, 2 ** 31, [], [], 2)
    _raises(-1, "edge 0: a == b = 5", c.cluster_graph, 2 ** 31, [5], [5], 2)                    # the edges before the limits
    w = np.array([2 ** 31, 2 ** 31 - 1, 0, 1, 0, 0], np.uint32)                                 # T = 2^32
    _raises(-4, "herro_cluster_graph: the weights sum to 4294967296: the total must stay below 2^32", c.cluster_graph, 6, a, b, 2, weights=w)
    w[3] = 0                                                                                    # T = 2^32 - 1: legal, so the device is asked for
    _raises(-2, "herro_cluster_graph: the context has no device", c.cluster_graph, 6, a, b, 2, weights=w)
    _raises(-2, "herro_cluster_graph: the context has no device", c.cluster_graph, 6, [3, 1, 0, 1], [1, 3, 1, 0], 65535, span=[1, 2, 3, 4], min_span=9)
    _raises(-2, "herro_cluster_graph: the context has no device", c.cluster_graph, 0, [], [], 1)
    P = api.ClusterParams(n_parts=2, min_span=0)
    import ctypes as C
    h = C.c_void_p(1)
    assert c._l.herro_cluster_graph(c.h, 6, None, 0, None, None, None, None, C.byref(h)) == -1 and "params is NULL" in c.last_error() and not h.value
    assert c._l.herro_cluster_graph(c.h, 6, None, 1, None, None, None, C.byref(P), C.byref(h)) == -1 and "null edge arrays" in c.last_error()
    P.reserved[1] = 1
    assert c._l.herro_cluster_graph(c.h, 6, None, 0, None, None, None, C.byref(P), C.byref(h)) == -1 and "reserved fields must be 0" in c.last_error()
    assert c._l.herro_cluster_graph(c.h, 6, None, 0, None, None, None, C.byref(P), None) == -1
    c.close()


def test_pairs_cluster_checks_the_handle_and_the_parameters():
    import ctypes as C
    c = api.HostContext(np.full(4, 1000, np.uint32))
    rows = np.array([[1, 1000, 0, 600, 0, 0, 1000, 400, 1000], [3, 1000, 100, 700, 1, 2, 1000, 0, 500]], np.uint32)
    rids, aln_off, rec = np.array([0, 1, 2, 3], np.uint32), np.array([0, 1, 2, 3, 4], np.uint64), np.array([0, 2, 1, 3], np.uint32)
    p = c.pairs_from_table(rows, None, rids, aln_off, rec)
    _raises(-1, "herro_pairs_cluster: n_parts = 0", p.cluster, 0)
    _raises(-4, "herro_pairs_cluster: the weights sum to", p.cluster, 2, weights=np.full(4, 2 ** 30, np.uint32))
    _raises(-2, "herro_pairs_cluster: the context has no device", p.cluster, 2, weights=[1, 2, 3, 4], min_span=500)
    with pytest.raises(ValueError):
        p.cluster(2, weights=[1, 2, 3])
    other = api.HostContext(np.full(4, 1000, np.uint32))
    h, P = C.c_void_p(), api.ClusterParams(n_parts=2)
    assert other._l.herro_pairs_cluster(other.h, p.h, None, C.byref(P), C.byref(h)) == -1
    assert "herro_pairs_cluster: the pairs handle belongs to another context" in other.last_error()
    assert other._l.herro_pairs_cluster(other.h, None, None, C.byref(P), C.byref(h)) == -1 and "pairs is NULL" in other.last_error()
    p.close()
    other.close()
    c.close()
    for name in ("herro_cluster_graph", "herro_pairs_cluster", "herro_clusters_mask", "herro_clusters_free"):
        assert name in api.EXPORTS


def test_cluster_masks_refuses_the_keywords_it_sets_itself():
    """the graph is found with extend=False over all reads: extend= and core= are refused before the context is touched"""
    for kw in (dict(extend=True), dict(core=np.ones(4, np.uint8))):
        with pytest.raises(ValueError) as e:
            shard.cluster_masks(None, [1000] * 4, 256, 2, **kw)
        assert "cluster_masks: " + list(kw)[0] + "=" in str(e.value)
        with pytest.raises(ValueError):
            shard.correct_reads_sharded(None, [1000] * 4, 256, 64, 0, str, partition="overlaps", **kw)


def test_null_handles_are_harmless():
    L = api.lib()
    assert L.herro_clusters_n_parts(None) == 0 and L.herro_clusters_n_reads(None) == 0 and not L.herro_clusters_part(None)
    assert L.herro_clusters_stats(None, None) == -1 and L.herro_clusters_part_stats(None, 0, None) == -1 and L.herro_clusters_mask(None, 0, None) == -1
    L.herro_clusters_free(None)
