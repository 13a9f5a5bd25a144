"""Rate of herro_align_overlaps (csrc/align_dev.hip) at the bench's shape: targets of 4096 bp with 32 overlaps each, the
synthetic generator's default ONT-like error.  Prints one JSON line: records/s, band cells/s (128 per anti-diagonal) and
4096-bp-window equivalents/s (one window = 32 records), for the whole call (upload, kernel, ops back, text) — run it under
`rocprofv3 --kernel-trace --stats` for the kernel alone.

    python tools/alignrate.py [--targets 2048] [--reps 3]"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from herro_amd import api, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", type=int, default=2048)
    ap.add_argument("--overlaps", type=int, default=32)
    ap.add_argument("--target-len", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    sb = synth.generate_parallel(a.targets, a.target_len, a.overlaps, chunk=64)
    rows = np.ascontiguousarray(sb.aln[:, :9])
    c = api.Context(0)
    c.set_reads(sb.seq, sb.qual, sb.off)
    c.align(rows[: min(len(rows), 4096)])           # warm-up (code objects, allocator)
    times = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        out, cig, sc, ok = c.align(rows)
        times.append(time.perf_counter() - t0)
    t = min(times)
    cells = float(((rows[:, 3] - rows[:, 2]).astype(np.int64) + (rows[:, 8] - rows[:, 7]) + 1).sum()) * 128
    n = len(rows)
    print(json.dumps({"records": n, "failed": int((~ok).sum()), "seconds": t, "records_per_s": n / t, "cells_per_s": cells / t,
                      "window_equivalents_per_s": n / t / a.overlaps, "mean_record_bp": float((rows[:, 8] - rows[:, 7]).mean()),
                      "ops_bytes": int(out[:, 9].astype(np.int64).sum())}))
    c.close()


if __name__ == "__main__":
    main()
