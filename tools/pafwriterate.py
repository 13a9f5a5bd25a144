"""Rate of the PAF writer (herro_pairs_paf, herro_pairs_write_alns; csrc/paf_dev.hip) at the bench shape of DESIGN.md §10: 256
targets x 4096 bp x 32 overlaps, `max_occ=128, min_score=100` — 135 168 pairs, 270 336 rows.  The alignments are found once
(find_overlap_pairs -> align); then, alternating in one process after a warm-up of each, the median of --reps by the host clock around the
synchronous call, fastest .. slowest beside it:

    device     p.paf(m, names): k_paf_len, the scan, k_paf_write in chunks, the text down through two pinned buffers into one host block
    baseline   what a host has to do today for the same bytes: the op store down with one copy (timed as a device-to-host copy of as many bytes
               into pageable memory), then the host formatter — the HostContext path over those ops, i.e. the specification code itself
    files      p.write_alns(...) plain and .oec.zst, with the seconds the call spent inside the zstd compressor (HERRO_PAF_STATS)

The ops of the baseline's handle are parsed back, outside every clock, from the device's text — which tests/test_gpu_paf_write.py holds to the
host formatter byte for byte; the two texts are compared here once more.  For the kernels alone run it under the profiler, on its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o paf -- python tools/pafwriterate.py --device-only
    python tools/pafwriterate.py [--targets 256] [--reps 5] [--out profiles/paf_write_rate.json] [--kernel-stats OUT/.../paf_kernel_stats.csv]

--kernel-stats: the profiler's table of such a run; the times of k_paf_len and k_paf_write and the write bandwidth of k_paf_write (text bytes
over kernel time, against the 8 TB/s of an MI355X) go into the result."""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from herro_amd import api, synth  # noqa: E402

HBM_BYTES_PER_S = 8e12


def ops_of_text(text: bytes):
    """(n_ops u32 [lines], ops u32) of a PAF text whose names hold no upper-case letter: vectorised, the CIGAR is the field behind the 12th tab"""
    t = np.frombuffer(text, np.uint8)
    nl = np.flatnonzero(t == 10)
    tabs = np.flatnonzero(t == 9)
    assert len(tabs) == 12 * len(nl)
    cstart = tabs[11::12] + 6                                   # behind "cg:Z:"
    edge = np.zeros(len(t) + 1, np.int8)
    edge[cstart] += 1
    edge[nl] -= 1
    in_cig = np.cumsum(edge[:-1], dtype=np.int8) > 0
    pos = np.flatnonzero(in_cig & (t > 57))                     # M I D ?
    line = np.searchsorted(nl, pos)
    n_ops = np.bincount(line, minlength=len(nl)).astype(np.uint32)
    prev = np.empty_like(pos)
    prev[1:] = pos[:-1]
    first = np.concatenate([[0], np.cumsum(n_ops)[:-1]]).astype(np.int64)[n_ops > 0]
    prev[first] = cstart[n_ops > 0] - 1
    width = pos - prev - 1
    val = np.zeros(len(pos), np.uint32)
    for k in range(int(width.max()) if len(pos) else 0):
        has = width > k
        val[has] += (t[pos[has] - 1 - k].astype(np.uint32) - 48) * np.uint32(10 ** k)
    ty = np.zeros(256, np.uint32)
    ty[ord("I")], ty[ord("D")], ty[ord("?")] = 1, 2, 3
    return n_ops, (val << np.uint32(2)) | ty[t[pos]]


def stats(ts):
    ts = sorted(ts)
    return {"median_s": ts[len(ts) // 2], "min_s": ts[0], "max_s": ts[-1]}


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


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


def kernel_stats(path, text_bytes, calls_per_text):
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            for k in ("k_paf_len", "k_paf_write"):
                if k + "(" in row["Name"]:
                    out[k] = {"calls": int(row["Calls"]), "total_ns": int(row["TotalDurationNs"]), "average_ns": float(row["AverageNs"])}
    if "k_paf_write" in out and calls_per_text:
        texts = out["k_paf_write"]["calls"] / calls_per_text          # whole texts the run wrote
        bw = text_bytes * texts / (out["k_paf_write"]["total_ns"] * 1e-9)
        out["k_paf_write"]["text_bytes_per_s"] = bw
        out["k_paf_write"]["share_of_8_TB_per_s"] = bw / HBM_BYTES_PER_S
        out["k_paf_write"]["ns_per_text"] = out["k_paf_write"]["total_ns"] / texts
        out["k_paf_len"]["ns_per_text"] = out["k_paf_len"]["total_ns"] / texts
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", type=int, default=256)
    ap.add_argument("--overlaps", type=int, default=32)
    ap.add_argument("--target-len", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "paf_write_rate.json"))
    ap.add_argument("--device-only", action="store_true", help="the device call alone, warm-up and --reps times (a profiler run); one JSON line, no file")
    ap.add_argument("--kernel-stats", default=None, help="kernel stats (csv) of a --device-only run under rocprofv3 --kernel-trace --stats")
    a = ap.parse_args()
    os.environ["HERRO_PAF_STATS"] = "1"
    if not a.device_only:
        import torch   # (first: PyTorch brings its own HIP runtime and finds no device once the library's has initialised — tests/conftest.py)
        torch.cuda.init()
    params = dict(max_occ=128, min_score=100)
    c = api.Context(0)                                       # (raises without a device)
    sb = synth.generate_parallel(a.targets, a.target_len, a.overlaps, chunk=64)
    c.set_reads(sb.seq, sb.qual, sb.off)
    names = [b"read%d" % i for i in range(c.n_reads)]
    p = c.find_overlap_pairs(**params)
    m = p.align()
    text, err = with_stderr(lambda: p.paf(m, names))         # warm-up of the device call
    chunks = int(err.split("chunks=")[1].split()[0])
    n_lines = text.count(b"\n")
    res = {"shape": {"targets": a.targets, "target_len": a.target_len, "overlaps": a.overlaps, "reads": int(c.n_reads)}, "params": params, "reps": a.reps,
           "rows": int(p.n_rows), "pairs": int(p.n_pairs), "failed_records": int(m.failed), "lines": n_lines, "text_bytes": len(text), "chunks": chunks}
    if a.device_only:
        ts = [with_stderr(lambda: timed(lambda: p.paf(m, names))[0])[0] for _ in range(a.reps)]
        res["device"] = stats(ts)
        res["device_calls"] = a.reps + 1
        print(json.dumps(res), flush=True)
        return

    # the baseline's handle: the same rows in table order over the same ops, on a context without a device
    n_ops, ops = ops_of_text(text)
    kept = p.rec_of_row[m.ok[p.rec_of_row]]
    assert len(kept) == n_lines == len(n_ops)
    host = api.HostContext(np.diff(sb.off.astype(np.int64)).astype(np.uint32))
    hb = host.aligned_dev_from_ops(m.rows[kept], np.concatenate([[0], np.cumsum(n_ops, dtype=np.uint64)]).astype(np.uint64), ops)
    res["ops"] = int(len(ops))
    d_ops = torch.zeros(len(ops), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def fetch():
        d_ops.cpu()                                           # one device-to-host copy of the op store's bytes into pageable memory
        torch.cuda.synchronize()

    fetch()
    same = with_stderr(lambda: hb.paf(names))[0] == text      # warm-up of the host formatter; the two texts once more
    res["texts_equal"] = bool(same)
    if not same:
        raise SystemExit("the device's text and the host formatter's differ")
    t_dev, t_fetch, t_fmt = [], [], []
    for _ in range(a.reps):                                   # alternating
        t_dev.append(with_stderr(lambda: timed(lambda: p.paf(m, names))[0])[0])
        t_fetch.append(timed(fetch)[0])
        t_fmt.append(with_stderr(lambda: timed(lambda: hb.paf(names))[0])[0])
    res["device"] = stats(t_dev)
    res["baseline"] = {"fetch": stats(t_fetch), "format": stats(t_fmt), "total": stats([x + y for x, y in zip(t_fetch, t_fmt)])}
    for k in ("device",):
        res[k]["text_bytes_per_s"] = len(text) / res[k]["median_s"]
        res[k]["rows_per_s"] = n_lines / res[k]["median_s"]
    res["baseline"]["total"]["text_bytes_per_s"] = len(text) / res["baseline"]["total"]["median_s"]
    res["baseline"]["total"]["rows_per_s"] = n_lines / res["baseline"]["total"]["median_s"]
    res["baseline_over_device"] = res["baseline"]["total"]["median_s"] / res["device"]["median_s"]

    # the files
    with tempfile.TemporaryDirectory() as d:
        files = {}
        for kind, fn in (("plain", "batch.paf"), ("oec_zst", "0.oec.zst")):
            path = os.path.join(d, fn)
            ts, zs, size = [], [], 0
            for i in range(a.reps + 1):
                (t, (lines, size)), err = with_stderr(lambda: timed(lambda: p.write_alns(m, names, path)))
                assert lines == n_lines
                if i:                                         # (the first is the warm-up)
                    ts.append(t)
                    zs.append(float(err.split("zstd_s=")[1].split()[0]))
            files[kind] = dict(stats(ts), file_bytes=int(size), zstd_s_median=sorted(zs)[len(zs) // 2])
            files[kind]["zstd_share"] = files[kind]["zstd_s_median"] / files[kind]["median_s"]
        back = api.Paf(names, path=path)                      # the .oec.zst through the library's reader
        files["oec_zst"]["read_back_rows"] = int(back.n_alns)
        back.close()
        res["write_alns"] = files
    if a.kernel_stats:
        res["kernels"] = kernel_stats(a.kernel_stats, len(text), chunks)
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    for x in (hb, p, m):
        x.close()
    host.close()
    c.close()


if __name__ == "__main__":
    main()
