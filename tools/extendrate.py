"""Cost and effect of herro_extend_overlaps (k_extend in csrc/align_dev.hip) on the bench's shape (targets of
4096 bp with 32 overlaps each): find -> extend -> align_dev against find -> align_dev in one process.  The calls are synchronous,
so the wall clock around a call is the call; every figure is the median of --reps runs after a warm-up, with the fastest and the
slowest.  Reports the extension call's time and its share of the aligner's time on the same run, the bases it adds, the diagonals
it computes, and the (overlap, window) pairs the reference's windowing rule (windowing.rs:53-108) takes from the target spans
before and after.  Prints the JSON and writes it to --out.

    python tools/extendrate.py [--targets 256] [--reps 5] [--out profiles/extend_rate.json]"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from herro_amd import api, synth  # noqa: E402


def window_pairs(rows, W):
    """(overlap, window) pairs the windowing takes from the target spans: none from a span shorter than W, whole windows only,
    except within 0.1 W of the read's ends"""
    ts, te, tlen = (rows[:, c].astype(np.int64) for c in (7, 8, 6))
    thr = int(np.float32(0.1) * np.float32(W))
    first = np.where(ts < thr, 0, (ts + W - 1) // W)
    last = np.where(te > tlen - thr, (te - 1) // W + 1, te // W)
    return int(np.where(te - ts < W, 0, np.maximum(last - first, 0)).sum())


def timed(fn, reps):
    out, times = None, []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return out, {"median": float(np.median(times)), "min": min(times), "max": max(times)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", type=int, default=256)
    ap.add_argument("--overlaps", type=int, default=32)
    ap.add_argument("--target-len", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "extend_rate.json"))
    a = ap.parse_args()
    sb = synth.generate_parallel(a.targets, a.target_len, a.overlaps, chunk=64)
    c = api.Context(0)
    c.set_reads(sb.seq, sb.qual, sb.off)
    params = dict(max_occ=128, min_score=100)
    rids, rows, off, sc = c.find_overlaps(**params)
    warm = rows[: min(len(rows), 4096)]
    c.extend_overlaps(warm)                                   # warm-up: code objects, allocator
    c.align_dev(warm).close()
    (rows_e, ext, esc), t_ext = timed(lambda: c.extend_overlaps(rows), a.reps)

    def align(r):
        h = c.align_dev(r)
        failed = h.failed
        h.close()
        return failed

    failed_plain, t_plain = timed(lambda: align(rows), a.reps)
    failed_ext, t_after = timed(lambda: align(rows_e), a.reps)
    # the diagonals a side computes are not returned; what is known is what it kept: i + j of the best cell
    kept = ext[:, 0].astype(np.int64) + ext[:, 1] + ext[:, 2] + ext[:, 3]
    res = {
        "set": "bench shape", "targets": a.targets, "target_len": a.target_len, "overlaps": a.overlaps, "reads": sb.n_reads,
        "bases": int(sb.off[-1]), "records": len(rows), "params": params, "reps": a.reps,
        "extend_seconds": t_ext, "align_dev_seconds_anchor_spans": t_plain, "align_dev_seconds_extended_spans": t_after,
        "extend_over_align": t_ext["median"] / t_after["median"],
        "extend_records_per_s": len(rows) / t_ext["median"],
        "align_failed_anchor_spans": failed_plain, "align_failed_extended_spans": failed_ext,
        "bases_added_per_record_mean": float(kept.mean()) / 2, "diagonals_kept_per_record_mean": float(kept.mean()),
        "sides_extended": int((esc > 0).sum()), "sides": 2 * len(rows),
        "target_bases_added_mean": float((ext[:, 0].astype(np.int64) + ext[:, 2]).mean()),
        "overlap_window_pairs": {str(W): {"anchor_spans": window_pairs(rows, W), "extended_spans": window_pairs(rows_e, W)}
                                 for W in (256, 1024, 4096)},
    }
    text = json.dumps(res, indent=1)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    c.close()


if __name__ == "__main__":
    main()
