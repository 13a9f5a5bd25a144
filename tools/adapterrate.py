"""Rate of herro_find_adapters (csrc/adapter_dev.hip) on tools/overlaprate.py's synthetic read sets: two adapters of 28 and 22 bases, both
strands, max_err_pm 250.  The call returns when the device is done, so the wall clock around it is the call; HERRO_ADAPT_STATS=1 gives its
split into the scan kernel, the start kernel with the download, and the host's sort.  One warm-up call, then the median of --reps calls with
the fastest and the slowest.  Prints one JSON line per set; run it under `rocprofv3 --kernel-trace --stats` for the kernels alone.
--finder: also times find_overlaps on the same context and set (overlaprate's parameters), for the ratio of the two.
--dense: one 8-base adapter instead (k = 2: chance hits every few hundred bases), the shape in which many lanes append to the one hit counter
and the first scan may outgrow its buffer (`scans` in the result line says whether it ran twice).

    python tools/adapterrate.py [--targets 256] [--long-targets 8] [--reps 5] [--seg 256] [--finder] [--dense]"""
from __future__ import annotations

import argparse
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from herro_amd import api, synth  # noqa: E402


def with_stats(fn):
    """run fn() with HERRO_ADAPT_STATS=1 and return (its result, the fields of the ADAPT line the library printed on stderr)"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        os.environ["HERRO_ADAPT_STATS"] = "1"
        try:
            r = fn()
        finally:
            os.environ.pop("HERRO_ADAPT_STATS", None)
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        text = f.read().decode(errors="replace")
    m = re.search(r"ADAPT (.*)", text)
    return r, {k: float(v) if "." in v else int(v) for k, v in (kv.split("=") for kv in m.group(1).split())} if m else {}


def measure(name, sb, reps, adapters, finder_params):
    c = api.Context(0)
    c.set_reads(sb.seq, sb.qual, sb.off)
    kw = dict(max_err_pm=250)
    c.find_adapters(adapters, **kw)                                           # warm-up: code objects, allocator
    times, split = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        (hits, off), st = with_stats(lambda: c.find_adapters(adapters, **kw))
        times.append(time.perf_counter() - t0)
        split.append(st)
    t = float(np.median(times))
    mid = split[int(np.argsort(times)[len(times) // 2])]                      # the split of the median call
    bases = int(sb.off[-1])
    res = {"set": name, "reads": sb.n_reads, "bases": bases, "adapters": [len(a) for a in adapters], "patterns": mid.get("patterns"), "max_err_pm": 250,
           "seg": mid.get("seg"), "segments": mid.get("segments"), "hits": len(hits), "scans": mid.get("scans"), "reps": reps, "seconds_median": t,
           "seconds_min": min(times), "seconds_max": max(times), "bases_per_s": bases / t,
           "base_patterns_per_s": bases * (mid.get("patterns") or 0) / t,
           "split_ms": {"k_adapt_scan": mid.get("scan_ms"), "k_adapt_start_and_download": mid.get("start_ms"), "host_sort": mid.get("host_ms"),
                        "rest_of_the_call": 1e3 * t - sum(mid.get(k, 0) for k in ("scan_ms", "start_ms", "host_ms"))}}
    if finder_params is not None:
        c.find_overlaps(**finder_params)
        ft = []
        for _ in range(reps):
            t0 = time.perf_counter()
            c.find_overlaps(**finder_params)
            ft.append(time.perf_counter() - t0)
        res.update({"finder_seconds_median": float(np.median(ft)), "adapters_over_finder": t / float(np.median(ft))})
    print(json.dumps(res), flush=True)
    c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", type=int, default=256)
    ap.add_argument("--overlaps", type=int, default=32)
    ap.add_argument("--target-len", type=int, default=4096)
    ap.add_argument("--long-targets", type=int, default=8)
    ap.add_argument("--long-len", type=int, default=30000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seg", type=int, default=0, help="HERRO_ADAPT_SEG: bases per lane (0: the library's default)")
    ap.add_argument("--finder", action="store_true", help="also time find_overlaps on the same set")
    ap.add_argument("--dense", action="store_true", help="one 8-base adapter: dense chance hits")
    a = ap.parse_args()
    if a.seg:
        os.environ["HERRO_ADAPT_SEG"] = str(a.seg)
    rng = np.random.default_rng(28)
    adapters = [bytes(b"ACGT"[x] for x in rng.integers(0, 4, m)) for m in ((8,) if a.dense else (28, 22))]
    if a.targets:
        measure("bench shape", synth.generate_parallel(a.targets, a.target_len, a.overlaps, chunk=64), a.reps, adapters,
                dict(max_occ=128, min_score=100) if a.finder else None)
    if a.long_targets:
        measure(">= 30 kb", synth.generate_parallel(a.long_targets, a.long_len, 16, chunk=4, flank_min=200, flank_max=400), a.reps, adapters,
                dict(max_occ=128) if a.finder else None)


if __name__ == "__main__":
    main()
