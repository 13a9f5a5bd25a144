"""Rate of herro_align_overlaps (csrc/align_dev.hip) at the bench's shape: targets of 4096 bp with 32 overlaps each, the
synthetic generator's default ONT-like error.  Prints one JSON line: records/s, band cells/s (128 per anti-diagonal) and
4096-bp-window equivalents/s (one window = 32 records), for the whole call (upload, kernel, ops back, text) — run it under
`rocprofv3 --kernel-trace --stats` for the kernel alone.

Two legs follow in the same process on the same records, from the records to a job that is ready to featurize (DESIGN.md section 9,
"device-resident hand-off"), both straight on the C ABI so that neither pays for Python objects per record:
    text    herro_align_overlaps -> (regroup the records that aligned) -> herro_job_create -> herro_aligned_free
    dev     herro_align_overlaps_dev -> (the same regrouping, as indices) -> herro_job_create_aligned -> herro_aligned_dev_free
Each is timed --reps times after a warm-up; "legs" holds the median, the fastest and the slowest run of each and the ratio of the medians.

--pairs times two other legs instead ("Mirrored records"), on the n records and their n swaps — the two directions
a finder emits for every read pair, the swaps grouped by their own targets — and prints one JSON line for profiles/align_pairs_rate.json:
    dual    the 2n records through herro_align_overlaps_dev -> herro_job_create_aligned: every pair aligned twice (the yardstick)
    pair    the n primaries through herro_align_overlaps_dev -> herro_aligned_dev_mirror -> the same job
api.pair_rows, which finds the n primaries among the 2n rows, runs once in front of the clock and is timed on its own.

    python tools/alignrate.py [--targets 2048] [--reps 5] [--window 4096] [--pairs]"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from herro_amd import api, synth  # noqa: E402


def _job_or_raise(c, h):
    if not h:
        raise api.HerroError(c._l.herro_job_create_status(c.h), c.last_error())
    return h


def text_leg(c, arr, n, rids, aln_off, W):
    """seconds from the records to the job through CIGAR text; the job is freed outside the clock"""
    L = c._l
    t0 = time.perf_counter()
    h = C.c_void_p()
    c._chk(L.herro_align_overlaps(c.h, n, C.byref(arr), C.byref(h)))
    alns = L.herro_aligned_alignments(h)
    off = aln_off
    if L.herro_aligned_failed(h):                     # drop the failed records, keep every target's place (api.aligned_job_args)
        v = np.frombuffer((api.Alignment * n).from_address(alns), api.ALN_DTYPE, n)
        ok = v["f"][:, 9] > 0
        kept = np.ascontiguousarray(v[ok])
        alns = kept.ctypes.data
        off = np.concatenate([[0], np.cumsum(ok)]).astype(np.uint64)[aln_off.astype(np.int64)]
    job = _job_or_raise(c, L.herro_job_create(c.h, len(rids), rids.ctypes.data, off.ctypes.data, alns, W))
    L.herro_aligned_free(h)
    t = time.perf_counter() - t0
    L.herro_job_free(job)
    return t


def dev_leg(c, arr, n, rids, aln_off, W):
    """the same through the device-resident handle"""
    L = c._l
    t0 = time.perf_counter()
    h = C.c_void_p()
    c._chk(L.herro_align_overlaps_dev(c.h, n, C.byref(arr), C.byref(h)))
    n_ops = np.ctypeslib.as_array(C.cast(L.herro_aligned_dev_n_ops(h), C.POINTER(C.c_uint32)), (n,))
    _, off, rec = api.aligned_dev_job_args(rids, aln_off, n_ops > 0)
    job = _job_or_raise(c, L.herro_job_create_aligned(c.h, len(rids), rids.ctypes.data, off.ctypes.data, rec.ctypes.data, h, W))
    built = L.herro_debug_job_dev_built(job)
    L.herro_aligned_dev_free(h)
    t = time.perf_counter() - t0
    L.herro_job_free(job)
    assert built == 1, "the direct path was not taken"
    return t


def pair_leg(c, arr_prim, n_prim, rids, aln_off, rec_of_row, W):
    """the primaries aligned, every record mirrored on the device, the job over all 2n rows"""
    L = c._l
    t0 = time.perf_counter()
    h = C.c_void_p()
    c._chk(L.herro_align_overlaps_dev(c.h, n_prim, C.byref(arr_prim), C.byref(h)))
    m = C.c_void_p()
    c._chk(L.herro_aligned_dev_mirror(c.h, h, C.byref(m)))
    L.herro_aligned_dev_free(h)
    n_ops = np.ctypeslib.as_array(C.cast(L.herro_aligned_dev_n_ops(m), C.POINTER(C.c_uint32)), (2 * n_prim,))
    _, off, rec = api.paired_job_args(rids, aln_off, rec_of_row, n_ops > 0)
    job = _job_or_raise(c, L.herro_job_create_aligned(c.h, len(rids), rids.ctypes.data, off.ctypes.data, rec.ctypes.data, m, W))
    built = L.herro_debug_job_dev_built(job)
    L.herro_aligned_dev_free(m)
    t = time.perf_counter() - t0
    L.herro_job_free(job)
    assert built == 1, "the direct path was not taken"
    return t


def pairs_main(a, sb, c):
    """--pairs: the dual and the pair leg on the records and their swaps"""
    rows = np.ascontiguousarray(sb.aln[:, :9])
    n = len(rows)
    swaps = rows[:, [5, 6, 7, 8, 4, 0, 1, 2, 3]]
    o = np.argsort(swaps[:, 5], kind="stable")                            # the swaps grouped by their targets, the query reads
    both = np.ascontiguousarray(np.concatenate([rows, swaps[o]]))
    extra, cnt = np.unique(swaps[o][:, 5], return_counts=True)
    assert not np.intersect1d(extra, sb.tgt_rid).size, "a read is target and query at once: the grouping below would split it"
    rids = np.ascontiguousarray(np.concatenate([sb.tgt_rid, extra]), np.uint32)
    aln_off = np.concatenate([sb.tgt_aln_off, int(sb.tgt_aln_off[-1]) + np.cumsum(cnt)]).astype(np.uint64)
    t0 = time.perf_counter()
    prim, rec_of_row = api.pair_rows(both)
    t_pair_rows = time.perf_counter() - t0
    assert len(prim) == n and np.array_equal(prim, np.arange(n))
    arr2 = (api.Alignment * (2 * n))()
    np.frombuffer(arr2, api.ALN_DTYPE, 2 * n)["f"][:, :9] = both
    arr1 = (api.Alignment * n)()
    np.frombuffer(arr1, api.ALN_DTYPE, n)["f"][:, :9] = both[prim]
    legs = {}
    for name, run in (("dual", lambda: dev_leg(c, arr2, 2 * n, rids, aln_off, a.window)),
                      ("pair", lambda: pair_leg(c, arr1, n, rids, aln_off, rec_of_row, a.window))):
        run()                                           # warm-up (arenas of the job, code objects)
        ts = sorted(run() for _ in range(a.reps))
        legs[name] = {"median_s": ts[len(ts) // 2], "min_s": ts[0], "max_s": ts[-1], "rows_per_s": 2 * n / ts[len(ts) // 2]}
    legs["dual_over_pair"] = legs["dual"]["median_s"] / legs["pair"]["median_s"]
    legs["pair_rows_s"] = t_pair_rows
    legs["window"] = a.window
    legs["reps"] = a.reps
    print(json.dumps({"rows": 2 * n, "primaries": n, "targets": len(rids), "pairs": legs}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", type=int, default=2048)
    ap.add_argument("--overlaps", type=int, default=32)
    ap.add_argument("--target-len", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=int, default=4096)
    ap.add_argument("--legs-only", action="store_true", help="skip the timing of Context.align (a profiler run wants the two legs alone)")
    ap.add_argument("--pairs", action="store_true", help="time the dual and the pair leg (mirrored records) instead")
    a = ap.parse_args()
    sb = synth.generate_parallel(a.targets, a.target_len, a.overlaps, chunk=64)
    rows = np.ascontiguousarray(sb.aln[:, :9])
    c = api.Context(0)
    c.set_reads(sb.seq, sb.qual, sb.off)
    if a.pairs:
        pairs_main(a, sb, c)
        c.close()
        return
    n = len(rows)
    res = {"records": n}
    if not a.legs_only:
        c.align(rows[: min(len(rows), 4096)])           # warm-up (code objects, allocator)
        times = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            out, cig, sc, ok = c.align(rows)
            times.append(time.perf_counter() - t0)
        t = min(times)
        cells = float(((rows[:, 3] - rows[:, 2]).astype(np.int64) + (rows[:, 8] - rows[:, 7]) + 1).sum()) * 128
        res.update({"failed": int((~ok).sum()), "seconds": t, "records_per_s": n / t, "cells_per_s": cells / t,
                    "window_equivalents_per_s": n / t / a.overlaps, "mean_record_bp": float((rows[:, 8] - rows[:, 7]).mean()),
                    "ops_bytes": int(out[:, 9].astype(np.int64).sum())})
        del out, cig
    arr = (api.Alignment * max(n, 1))()
    np.frombuffer(arr, api.ALN_DTYPE, max(n, 1))["f"][:n, :9] = rows
    rids = np.ascontiguousarray(sb.tgt_rid, np.uint32)
    aln_off = np.ascontiguousarray(sb.tgt_aln_off, np.uint64)
    legs = {}
    for name, leg in (("text", text_leg), ("dev", dev_leg)):
        leg(c, arr, n, rids, aln_off, a.window)         # warm-up (arenas of the job, code objects)
        ts = sorted(leg(c, arr, n, rids, aln_off, a.window) for _ in range(a.reps))
        legs[name] = {"median_s": ts[len(ts) // 2], "min_s": ts[0], "max_s": ts[-1], "records_per_s": n / ts[len(ts) // 2]}
    legs["dev_over_text"] = legs["text"]["median_s"] / legs["dev"]["median_s"]
    legs["window"] = a.window
    legs["reps"] = a.reps
    res["legs"] = legs
    print(json.dumps(res))
    c.close()


if __name__ == "__main__":
    main()
