"""Rate of herro_find_adapters (csrc/adapter_dev.hip) on tools/overlaprate.py's synthetic read sets: two adapters of 28 and 22 bases, both
strands, max_err_pm 250.  The call returns when the device is done, so the wall clock around it is the call; HERRO_ADAPT_STATS=1 gives its
split into the scan kernel, the start kernel with the download, and the host's sort.  One warm-up call, then the median of --reps calls with
the fastest and the slowest.  Prints one JSON line per set; run it under `rocprofv3 --kernel-trace --stats` for the kernels alone.
--finder: also times find_overlaps on the same context and set (overlaprate's parameters), for the ratio of the two.
--dense: one 8-base adapter instead (k = 2: chance hits every few hundred bases), the shape in which many lanes append to the one hit counter
and the first scan may outgrow its buffer (`scans` in the result line says whether it ran twice).

--cut: instead, the cut of the store to the pieces the scan and the plan give ("The cut on the device"): the host path
(io.cut_reads + set_reads of the cut reads) against Context.cut_store, both from the same piece table, alternating in one process — every
timed call starts from the raw store, set again (untimed) before it.  The host clock around the synchronous calls, one warm-up of each,
the median of --reps.  One more cut under HERRO_CUT_STATS=2 gives the two kernels between events and a device-to-device hipMemcpyAsync of
the new word array and of the new quality array on the same device; GB/s counts the bytes read plus the bytes written.  Three sets in one
run — the two above and the bench shape at --big-targets (2048: 375 Mb; 0: left out) —, and --out (default profiles/adapter_cut_rate.json,
'' for none) is written anew with their result lines.

    python tools/adapterrate.py [--targets 256] [--long-targets 8] [--reps 5] [--seg 256] [--finder] [--dense] [--cut [--big-targets 2048] [--out FILE]]"""
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


def with_stats(fn, env="HERRO_ADAPT_STATS", value="1", tag="ADAPT"):
    """run fn() with the environment variable `env` set to `value` and return (its result, the fields of the line beginning with `tag` that the
    library printed on stderr; {} if there is none)"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        os.environ[env] = value
        try:
            r = fn()
        finally:
            os.environ.pop(env, None)
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        text = f.read().decode(errors="replace")
    m = re.search(tag + r" (.*)", text)
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


def measure_cut(name, sb, reps, adapters, out):
    from herro_amd import io
    c = api.Context(0)
    raw = io.Reads([b"r%d" % i for i in range(sb.n_reads)], [None] * sb.n_reads, sb.seq, sb.qual, sb.off)
    c.set_reads(raw.seq, raw.qual, raw.off)
    hits, hits_off = c.find_adapters(adapters, max_err_pm=250)
    pieces, _, stats = api.trim_plan(np.diff(np.asarray(sb.off, np.uint64)).astype(np.uint32), [len(a) for a in adapters], hits, hits_off)

    def host():
        t0 = time.perf_counter()
        cut = io.cut_reads(raw, pieces)
        t1 = time.perf_counter()
        c.set_reads(cut.seq, cut.qual, cut.off)
        return time.perf_counter() - t0, t1 - t0

    def device():
        t0 = time.perf_counter()
        c.cut_store(pieces)
        return time.perf_counter() - t0

    host_t, host_cut_t, dev_t = [], [], []
    for rep in range(reps + 1):                                               # rep 0: the warm-up of both
        t, tc = host()
        c.set_reads(raw.seq, raw.qual, raw.off)
        d = device()
        c.set_reads(raw.seq, raw.qual, raw.off)
        if rep:
            host_t.append(t); host_cut_t.append(tc); dev_t.append(d)
    _, st = with_stats(lambda: c.cut_store(pieces), env="HERRO_CUT_STATS", value="2", tag="CUT")
    nw, nq = st["words"], st["qual_bytes"]
    src_words = sum(-(-int(p["end"] - p["start"] + (p["start"] & 31)) // 32) for p in pieces)   # source words the pieces touch
    gbs = lambda nbytes, ms: nbytes / (ms * 1e6) if ms else None
    res = {"set": name, "reads": sb.n_reads, "bases": int(sb.off[-1]), "pieces": len(pieces), "bases_kept": int(nq), "trim_stats": list(stats), "reps": reps,
           "host_path_seconds_median": float(np.median(host_t)), "host_path_seconds_min": min(host_t), "host_path_seconds_max": max(host_t),
           "host_path_cut_reads_seconds_median": float(np.median(host_cut_t)),
           "device_path_seconds_median": float(np.median(dev_t)), "device_path_seconds_min": min(dev_t), "device_path_seconds_max": max(dev_t),
           "host_over_device": float(np.median(host_t)) / float(np.median(dev_t)),
           "kernels_ms": {"k_store_cut_words": st["words_ms"], "k_store_cut_qual": st["qual_ms"]},
           "kernels_GBps": {"k_store_cut_words": gbs(8 * src_words + 16 * nw, st["words_ms"]), "k_store_cut_qual": gbs(2 * nq, st["qual_ms"])},
           "memcpy_d2d_ms": {"word_array": st["copy_words_ms"], "quality_array": st["copy_qual_ms"]},
           "memcpy_d2d_GBps": {"word_array": gbs(16 * nw, st["copy_words_ms"]), "quality_array": gbs(2 * nq, st["copy_qual_ms"])}}
    line = json.dumps(res)
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()
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
    ap.add_argument("--cut", action="store_true", help="time the cut of the store instead: host path against Context.cut_store")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "adapter_cut_rate.json"),
                    help="--cut: the file the result lines are written to ('' for none)")
    ap.add_argument("--big-targets", type=int, default=2048, help="--cut: targets of the third set, the bench shape again (0: none)")
    a = ap.parse_args()
    if a.seg:
        os.environ["HERRO_ADAPT_SEG"] = str(a.seg)
    rng = np.random.default_rng(28)
    adapters = [bytes(b"ACGT"[x] for x in rng.integers(0, 4, m)) for m in ((8,) if a.dense else (28, 22))]
    if a.cut:
        out = open(a.out, "w") if a.out else None
        if a.targets:
            measure_cut("bench shape", synth.generate_parallel(a.targets, a.target_len, a.overlaps, chunk=64), a.reps, adapters, out)
        if a.long_targets:
            measure_cut(">= 30 kb", synth.generate_parallel(a.long_targets, a.long_len, 16, chunk=4, flank_min=200, flank_max=400), a.reps, adapters, out)
        if a.big_targets:
            measure_cut("bench shape", synth.generate_parallel(a.big_targets, a.target_len, a.overlaps, chunk=64), a.reps, adapters, out)
        if out:
            out.close()
        return
    if a.targets:
        measure("bench shape", synth.generate_parallel(a.targets, a.target_len, a.overlaps, chunk=64), a.reps, adapters,
                dict(max_occ=128, min_score=100) if a.finder else None)
    if a.long_targets:
        measure(">= 30 kb", synth.generate_parallel(a.long_targets, a.long_len, 16, chunk=4, flank_min=200, flank_max=400), a.reps, adapters,
                dict(max_occ=128) if a.finder else None)


if __name__ == "__main__":
    main()
