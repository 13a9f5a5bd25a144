"""Cost and worth of the clusters (herro_pairs_cluster, csrc/cluster_dev.hip).  Three measurements:
 1. reads: `--reads` reads of `--read-len` +- 50 % bases drawn from `--chromosomes` random chromosomes of `--chrom-len` bases (1 % substitutions,
    every third read reversed and complemented).  find_overlap_pairs(extend=False) — the finder, code of the parent commit and the mark — beside
    OverlapPairs.cluster on its handle, 8 parts, windows per read as weights: the median wall time of `--reps` calls each (both return when the
    device is done) and the ratio cluster_over_finder.
 2. on the same reads, sum over the parts of pairs_touching — the pairs the ranks align — under shard.core_masks and under the clusters.
 3. the per-stage split of one more cluster call after the timed ones (HERRO_CLUSTER_STATS=1: the stages between events, the rounds of the two host loops), for the
    reads' graph and for a graph without reads (tests/cluster_cases.genome_graph, `--graph-reads` reads) whose cuts with 0, 3 and 20 shortcuts
    are reported too.
Prints one JSON line per measurement; `--out FILE` also writes them as a JSON list.

    python tools/clusterrate.py [--reads 1500] [--reps 7] [--out profiles/cluster_rate.json]"""
from __future__ import annotations

import argparse
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cluster_cases as CC  # noqa: E402
from herro_amd import api, shard  # noqa: E402

W = 4096


def with_stats(fn):
    """fn() under HERRO_CLUSTER_STATS=1 -> (its result, the fields of the CLUSTER line the library printed on stderr)"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        os.environ["HERRO_CLUSTER_STATS"] = "1"
        try:
            r = fn()
        finally:
            os.environ.pop("HERRO_CLUSTER_STATS", None)
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        text = f.read().decode(errors="replace")
    m = re.search(r"CLUSTER (.*)", text)
    return r, {k: float(v) if "." in v else int(v) for k, v in (kv.split("=") for kv in m.group(1).split())} if m else {}


class GenomeReads:
    """what set_reads takes: reads placed uniformly on random chromosomes"""

    def __init__(self, n, read_len, chromosomes, chrom_len, seed=77):
        rng = np.random.default_rng(seed)
        genome = rng.integers(0, 4, (chromosomes, chrom_len), dtype=np.uint8)
        letters = np.frombuffer(b"ACGT", np.uint8)
        reads = []
        for r in range(n):
            L = int(rng.integers(read_len // 2, read_len * 3 // 2 + 1))
            c, s = int(rng.integers(0, chromosomes)), int(rng.integers(0, chrom_len - L + 1))
            x = genome[c, s:s + L].copy()
            at = np.flatnonzero(rng.random(L) < 0.01)
            x[at] = (x[at] + rng.integers(1, 4, len(at))) % 4
            if r % 3 == 2:
                x = (3 - x)[::-1]
            reads.append(letters[x])
        self.n_reads = n
        self.seq = np.concatenate(reads)
        self.qual = np.full(len(self.seq), 40 + 33, np.uint8)
        self.off = np.concatenate([[0], np.cumsum([len(x) for x in reads])]).astype(np.uint64)


def median_call(fn, reps):
    """(median, least) wall time of the plain call, as the finder beside it is timed; then the split of one more call, which pays for its event
    records and for the line the library prints and is therefore not among the timed ones"""
    fn().close()                                   # warm-up: code objects, allocator
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        h = fn()
        times.append(time.perf_counter() - t0)
        h.close()
    h, st = with_stats(fn)
    h.close()
    return float(np.median(times)), min(times), st


def split_ms(st, seconds):
    stages = {k: st.get(k) for k in ("arcs_ms", "comp_ms", "bfs_ms", "order_ms", "stats_ms")}
    stages["rest_of_the_call_ms"] = 1e3 * seconds - sum(v or 0 for v in stages.values())   # (the median plain call less the stages of the split's call)
    return dict(stages, hook_rounds=st.get("hook_rounds"), bfs_launches=st.get("bfs_launches"), host_reads=st.get("host_reads"), levels=st.get("levels"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1500)
    ap.add_argument("--read-len", type=int, default=12000)
    ap.add_argument("--chromosomes", type=int, default=3)
    ap.add_argument("--chrom-len", type=int, default=600000)
    ap.add_argument("--graph-reads", type=int, default=3000)
    ap.add_argument("--parts", type=int, default=8)
    ap.add_argument("--min-span", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    out = []

    def emit(d):
        out.append(d)
        print(json.dumps(d), flush=True)

    rs = GenomeReads(a.reads, a.read_len, a.chromosomes, a.chrom_len)
    lens = np.diff(rs.off.astype(np.int64))
    c = api.Context(0)
    c.set_reads(rs.seq, rs.qual, rs.off)
    finder = lambda: c.find_overlap_pairs(extend=False)
    finder().close()
    ft = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        finder().close()
        ft.append(time.perf_counter() - t0)
    pairs = finder()
    w = shard.windows_of(lens, W).astype(np.uint32)
    t_med, t_min, st = median_call(lambda: pairs.cluster(a.parts, weights=w, min_span=a.min_span), a.reps)
    cl = pairs.cluster(a.parts, weights=w, min_span=a.min_span)
    prim = pairs.primaries.astype(np.int64)
    ea, eb = prim[:, 5], prim[:, 0]
    by_windows = np.zeros(len(lens), np.int64)
    for p, m in enumerate(shard.core_masks(lens, W, a.parts)):
        by_windows[m != 0] = p
    touch_w = len(ea) + int((by_windows[ea] != by_windows[eb]).sum())
    touch_c = int(cl.part_stats[:, 4].sum())
    emit({"measure": "reads", "reads": a.reads, "bases": int(rs.off[-1]), "pairs": pairs.n_pairs, "parts": a.parts, "min_span": a.min_span, "reps": a.reps,
          "finder_seconds_median": float(np.median(ft)), "finder_seconds_min": min(ft), "cluster_seconds_median": t_med, "cluster_seconds_min": t_min,
          "cluster_over_finder": t_med / float(np.median(ft)), "stats": cl.stats, "split": split_ms(st, t_med)})
    emit({"measure": "pairs_touching", "reads": a.reads, "pairs": pairs.n_pairs, "parts": a.parts, "sum_pairs_touching_core_masks": touch_w,
          "sum_pairs_touching_cluster_masks": touch_c, "aligned_twice_core_masks": (touch_w - len(ea)) / max(len(ea), 1),
          "aligned_twice_cluster_masks": (touch_c - len(ea)) / max(len(ea), 1), "weight_per_part": cl.part_stats[:, 1].tolist()})
    cl.close()
    pairs.close()
    for shortcuts in (0, 3, 20):
        g, _ = CC.genome_graph(11, a.graph_reads, 3, shortcuts)
        run = lambda: c.cluster_graph(g["n"], g["a"], g["b"], a.parts, weights=g["w"], span=g["span"], min_span=g["min_span"])
        t_med, t_min, st = median_call(run, a.reps)
        cl = run()
        greedy = np.zeros(g["n"], np.int64)
        for p, ids in enumerate(shard.partition_targets(g["w"].astype(np.int64), a.parts)):
            greedy[ids] = p
        E = len(g["a"])
        emit({"measure": "graph", "reads": g["n"], "edges": E, "shortcuts": shortcuts, "parts": a.parts, "cluster_seconds_median": t_med, "cluster_seconds_min": t_min,
              "edge_cut": cl.stats["edge_cut"], "edge_cut_share": cl.stats["edge_cut"] / E,
              "edge_cut_share_by_window_counts": float((greedy[g["a"].astype(np.int64)] != greedy[g["b"].astype(np.int64)]).mean()), "stats": cl.stats,
              "split": split_ms(st, t_med)})
        cl.close()
    c.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
