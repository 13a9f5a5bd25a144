"""Rate of the corrected-reads text on one MI355X: the host path herro_job_fasta — every padded window slot down, records
assembled by the library's host pool; the parent's code, the yardstick — against herro_job_fasta_dev (csrc/fasta_dev.hip), which forms the
text on the device and brings it down finished.  One job of the bench's shape (4096-bp windows, 32 overlaps) with targets long enough to be
chopped: --targets x --target-len, a few thousand windows.  In one process, after a warm-up of each, alternating, the median of --reps by
the host clock around the synchronous call (fastest .. slowest beside it); the consensus pass is run again and awaited before every timed
call, outside the clock, so that each call fetches what a fresh job would:

    host       Job.fasta(ids, as_array=True) into a buffer that is reused (its sizing call does the fetch, its second call the assembly)
    device     Job.fasta_dev(ids, as_array=True): all-zero parameters, the same bytes
    chopped    Job.fasta_dev(ids, **api.POSTPROCESS, as_array=True): scripts/postprocess_corrected.sh's two numbers

and the bytes that cross PCIe on the way out: the window slots plus 4 bytes per window against the text.

    python tools/fastarate.py [--targets 192] [--target-len 45056] [--reps 7] [--out profiles/fasta_rate.json]"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from herro_amd import api, model_io, synth  # noqa: E402


def stats(ts):
    ts = sorted(ts)
    return {"median_s": ts[len(ts) // 2], "min_s": ts[0], "max_s": ts[-1]}


def with_stderr(fn):
    """fn() and what the library printed on stderr meanwhile"""
    sys.stderr.flush()
    with tempfile.TemporaryFile() as tf:
        saved = os.dup(2)
        os.dup2(tf.fileno(), 2)
        try:
            r = fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tf.seek(0)
        return r, tf.read().decode(errors="replace")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", type=int, default=192)
    ap.add_argument("--target-len", type=int, default=11 * 4096)
    ap.add_argument("--overlaps", type=int, default=32)
    ap.add_argument("--window", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fasta_rate.json"))
    a = ap.parse_args()
    import torch   # (first: PyTorch brings its own HIP runtime and finds no device once the library's has initialised — tests/conftest.py)
    torch.cuda.init()
    c = api.Context(0)
    path, _ = model_io.default_model_file(os.path.join(ROOT, "tests", "_cache"))
    c.load_model(path)
    c.set_precision(api.DEFAULT_PRECISION)
    sb = synth.generate_parallel(a.targets, a.target_len, a.overlaps, chunk=16)
    c.set_reads(sb.seq, sb.qual, sb.off)
    ids = [b"read%d" % t for t in range(sb.n_targets)]
    job = api.job_from_synth(c, sb, a.window)
    job.featurize(); job.infer(a.batch, 1)
    win = c.job_arrays(job)["win"]
    buf = {}

    def alloc(n):
        if buf.get("a") is None or len(buf["a"]) < n:
            buf["a"] = np.empty(n, np.uint8)
        return buf["a"][:n]

    calls = {"host": lambda: job.fasta(ids, as_array=True, out_alloc=alloc),
             "device": lambda: job.fasta_dev(ids, as_array=True),
             "chopped": lambda: job.fasta_dev(ids, as_array=True, **api.POSTPROCESS)}

    def fresh(name):
        job.consensus()
        c.synchronize()
        t0 = time.perf_counter()
        r = calls[name]()
        return time.perf_counter() - t0, r

    os.environ["HERRO_FASTA_STATS"] = "1"
    texts, lines = {}, {}
    for name in calls:                                         # warm-up, and the texts once against each other and the specification
        (_, r), err = with_stderr(lambda: fresh(name))
        texts[name] = bytes(r)
        lines[name] = [ln for ln in err.splitlines() if ln.startswith("FASTA ")]
    import chop_ref
    if texts["device"] != texts["host"] or texts["chopped"] != chop_ref.chop(texts["host"], **api.POSTPROCESS)[0]:
        raise SystemExit("the device's text and the host path's differ")
    ts = {name: [] for name in calls}
    for _ in range(a.reps):                                    # alternating
        for name in calls:
            (t, _), err = with_stderr(lambda: fresh(name))
            ts[name].append(t)
            lines[name] = [ln for ln in err.splitlines() if ln.startswith("FASTA ")] or lines[name]   # the stages of the last timed call
    slots = int(win["lub"].astype(np.uint64).sum())
    res = {"shape": {"targets": a.targets, "target_len": a.target_len, "overlaps": a.overlaps, "window": a.window, "windows": int(job.n_windows)},
           "reps": a.reps, "texts_equal": True,
           "pcie_bytes": {"host": slots + 4 * int(job.n_windows), "device": len(texts["device"]), "chopped": len(texts["chopped"])},
           "records": {k: v.count(b">") for k, v in texts.items()},
           "stats_line": {k: (v[-1] if v else None) for k, v in lines.items() if k != "host"}}
    for name in calls:
        res[name] = dict(stats(ts[name]), text_bytes_per_s=len(texts[name]) / stats(ts[name])["median_s"])
    res["host_over_device"] = res["host"]["median_s"] / res["device"]["median_s"]
    res["host_over_chopped"] = res["host"]["median_s"] / res["chopped"]["median_s"]
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    job.close()
    c.close()


if __name__ == "__main__":
    main()
