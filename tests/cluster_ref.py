"""The specification of herro_cluster_graph / herro_pairs_cluster (include/herro_amd.h, "clusters") in plain numpy: the
authority the kernels of csrc/cluster_dev.hip are compared with field for field.  It stands where the reference's workflow runs
scripts/create_clusters.py (METIS over the overlap graph) and whose files `herro inference -c` reads (lib.rs:208-239); it is NOT METIS: all
integer, independent of any order of evaluation.

Input: n reads, weights w (u32 [n], None: all 1), E undirected edges (a, b, span) (span None: every edge is strong), n_parts k, min_span.
  1. strong edges: span >= min_span.  Weak edges count in the masks and the statistics only.
  2. comp[v]: the least read id reachable from v over strong edges.
  3. d1[v]: BFS distance over strong edges from comp[v]; far[c]: the vertex of component c with the greatest d1, the least id among equals;
     level[v]: BFS distance from far[comp[v]].
  4. order: ascending (comp, level, v); rank[v] its position.
  5. S[v]: the sum of w over the reads before v in the order, T the total; part[v] = min(k - 1, S[v] * k // T) (T == 0: part 0).
  6. mask of part p over ALL edges: 1 core (part[v] == p), 2 neighbour (not core, adjacent to a core read of p), 0 otherwise.
  7. statistics: per part n_core, weight, n_neighbours, pairs_inside, pairs_touching; global n_components, n_levels, strong_edges, edge_cut.
"""
from __future__ import annotations

import dataclasses

import numpy as np

STAT_NAMES = ("n_components", "n_levels", "strong_edges", "edge_cut")
PART_STAT_NAMES = ("n_core", "weight", "n_neighbours", "pairs_inside", "pairs_touching")


@dataclasses.dataclass
class Clusters:
    n_parts: int
    comp: np.ndarray      # u32 [n]
    level: np.ndarray     # u32 [n]
    rank: np.ndarray      # u32 [n]
    part: np.ndarray      # u32 [n]
    masks: np.ndarray     # u8 [k, n]
    stats: dict           # STAT_NAMES
    part_stats: np.ndarray   # u64 [k, 5]: PART_STAT_NAMES


def _bfs(n, adj_off, adj, sources):
    """distance from the nearest source, every vertex reachable from one of them; -1 elsewhere"""
    dist = np.full(n, -1, np.int64)
    dist[sources] = 0
    frontier = np.unique(np.asarray(sources, np.int64))
    d = 0
    while len(frontier):
        nxt = []
        for u in frontier:
            for v in adj[adj_off[u]:adj_off[u + 1]]:
                if dist[v] < 0:
                    dist[v] = d + 1
                    nxt.append(int(v))
        frontier = np.asarray(nxt, np.int64)
        d += 1
    return dist


def part_of(S: int, T: int, k: int) -> int:
    """step 5 (herro::cluster_part, csrc/cluster_plan.h)"""
    return 0 if T == 0 else min(k - 1, S * k // T)


def cluster(n: int, w, a, b, span, n_parts: int, min_span: int = 0) -> Clusters:
    n, k = int(n), int(n_parts)
    a = np.asarray(a, np.int64).reshape(-1)
    b = np.asarray(b, np.int64).reshape(-1)
    E = len(a)
    assert 1 <= k <= 65535 and len(b) == E and (a != b).all() and (E == 0 or (max(a.max(), b.max()) < n and min(a.min(), b.min()) >= 0))
    w = np.ones(n, np.int64) if w is None else np.asarray(w, np.int64)
    strong = np.ones(E, bool) if span is None else np.asarray(span, np.int64) >= int(min_span)
    # adjacency over the strong edges
    src = np.concatenate([a[strong], b[strong]])
    dst = np.concatenate([b[strong], a[strong]])
    o = np.argsort(src, kind="stable")
    src, dst = src[o], dst[o]
    adj_off = np.zeros(n + 1, np.int64)
    np.add.at(adj_off, src + 1, 1)
    adj_off = np.cumsum(adj_off)
    # 2. components: the least id reachable (ids ascending, so the first unvisited vertex is its component's least)
    comp = np.full(n, -1, np.int64)
    for v in range(n):
        if comp[v] >= 0:
            continue
        comp[v] = v
        stack = [v]
        while stack:
            u = stack.pop()
            for x in dst[adj_off[u]:adj_off[u + 1]]:
                if comp[x] < 0:
                    comp[x] = v
                    stack.append(int(x))
    roots = np.flatnonzero(comp == np.arange(n))
    # 3. levels
    d1 = _bfs(n, adj_off, dst, roots)
    far = {}
    for v in range(n):
        c = int(comp[v])
        if c not in far or d1[v] > d1[far[c]]:
            far[c] = v
    level = _bfs(n, adj_off, dst, np.array([far[int(c)] for c in roots], np.int64)) if n else np.zeros(0, np.int64)
    assert (level >= 0).all()
    # 4. order
    order = np.lexsort((np.arange(n), level, comp))
    rank = np.empty(n, np.int64)
    rank[order] = np.arange(n)
    # 5. cut
    S = np.concatenate([[0], np.cumsum(w[order])])
    T = int(S[-1])
    part = np.zeros(n, np.int64)
    for i, v in enumerate(order):
        part[v] = part_of(int(S[i]), T, k)
    # 6. masks, 7. statistics: all edges
    masks = np.zeros((k, n), np.uint8)
    ps = np.zeros((k, 5), np.uint64)
    for p in range(k):
        core = part == p
        m = core.astype(np.uint8)
        nb = np.zeros(n, bool)
        nb[b[core[a]]] = True
        nb[a[core[b]]] = True
        m[nb & ~core] = 2
        masks[p] = m
        ca, cb = core[a], core[b]
        ps[p] = (int(core.sum()), int(w[core].sum()), int((m == 2).sum()), int((ca & cb).sum()), int((ca | cb).sum()))
    stats = {"n_components": len(roots), "n_levels": int(level.max()) + 1 if n else 0, "strong_edges": int(strong.sum()),
             "edge_cut": int((part[a] != part[b]).sum())}
    u32 = lambda x: x.astype(np.uint32)
    return Clusters(k, u32(comp), u32(level), u32(rank), u32(part), masks, stats, ps)
