"""Rate of herro_find_overlaps (csrc/overlap_dev.hip): bases sketched, anchors and overlap records per second for the whole
call (sketch, both sorts, chaining, results back; the call returns when the device is done, so the wall clock around it is the
call), next to herro_align_overlaps on the records it emitted.  Two sets: the bench's shape (targets of 4096 bp with 32
overlaps each) and reads of >= 30 kb.  Prints one JSON line per set; run it under `rocprofv3 --kernel-trace --stats` for the
kernels alone.

    python tools/overlaprate.py [--targets 256] [--long-targets 8] [--reps 5] [--no-align]"""
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


def stage_sizes(fn):
    """run fn() once with HERRO_OVL_STATS=1 and return (its result, the sizes the library printed on stderr)"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        os.environ["HERRO_OVL_STATS"] = "1"
        try:
            r = fn()
        finally:
            os.environ.pop("HERRO_OVL_STATS", None)
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        text = f.read().decode(errors="replace")
    m = re.search(r"OVL (.*)", text)
    return r, {k: int(v) for k, v in (kv.split("=") for kv in m.group(1).split())} if m else {}


def measure(name, sb, reps, params, align):
    c = api.Context(0)
    c.set_reads(sb.seq, sb.qual, sb.off)
    (rids, rows, off, sc), sizes = stage_sizes(lambda: c.find_overlaps(**params))     # also the warm-up (code objects, allocator)
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        c.find_overlaps(**params)
        times.append(time.perf_counter() - t0)
    t = float(np.median(times))
    bases = int(sb.off[-1])
    res = {"set": name, "reads": sb.n_reads, "bases": bases, **sizes, "records": len(rows), "params": params, "reps": reps,
           "seconds_median": t, "seconds_min": min(times), "seconds_max": max(times), "bases_per_s": bases / t,
           "anchors_per_s": sizes.get("anchors", 0) / t, "records_per_s": len(rows) / t}
    if align and len(rows):
        c.align(rows[: min(len(rows), 4096)])
        at = []
        for _ in range(max(2, reps // 2)):
            t0 = time.perf_counter()
            out, cig, asc, ok = c.align(rows)
            at.append(time.perf_counter() - t0)
        ta = float(np.median(at))
        res.update({"align_seconds_median": ta, "align_seconds_min": min(at), "align_seconds_max": max(at), "align_records_per_s": len(rows) / ta,
                    "align_failed": int((~ok).sum()), "find_over_align": t / ta})
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
    ap.add_argument("--no-align", action="store_true")
    a = ap.parse_args()
    if a.targets:
        measure("bench shape", synth.generate_parallel(a.targets, a.target_len, a.overlaps, chunk=64), a.reps,
                dict(max_occ=128, min_score=100), not a.no_align)
    if a.long_targets:
        measure(">= 30 kb", synth.generate_parallel(a.long_targets, a.long_len, 16, chunk=4, flank_min=200, flank_max=400), a.reps,
                dict(max_occ=128), not a.no_align)


if __name__ == "__main__":
    main()
