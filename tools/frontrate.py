"""Reads -> (mirrored alignments, job arguments): the stepwise chain of the Python binding against the pair calls of the C ABI
(herro_find_overlap_pairs, herro_pairs_align; DESIGN.md §10, "Pairs on the device"), in one process, the two chains alternating.

    stepwise   find_overlaps -> pair_rows -> extend_overlaps(rows[prim]) -> align_dev -> mirror -> paired_job_args
    pairs      find_overlap_pairs -> OverlapPairs.align        (the job arguments are the handle's table)

Host clock around the synchronous calls; every figure is the median of --reps runs after one warm-up of each chain, with min .. max
beside it, the stages separately.  The two chains' results are compared once.  Needs a GPU (no fallback).  The bench's shape by default:
256 targets x 4096 bp x 32 overlaps, max_occ 128, min_score 100.

    python tools/frontrate.py [--targets 256] [--reps 5] [--out profiles/front_pairs_rate.json]

--shards G: a core set of targets ("A core set of targets").  For every power of two g <= G the pair calls with the core
mask of shard 0 of shard.core_masks(read lengths, 4096, g) against the same calls without a mask, alternating in one process: median of
--reps after a warm-up of each, fastest .. slowest, the masked anchors (the finder's own HERRO_OVL_STATS line), the pairs, the rows and
the pairs kept as a share of all pairs — what the aligner's time should follow.  Writes profiles/front_core_rate.json.
--unmasked: the pair calls without a mask alone — the call a library without the core entries has too (HERRO_LIB), for an A/B of two
builds on one box: one JSON line, no file."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from herro_amd import api, shard, synth  # noqa: E402


def _timed(stages, name, fn):
    t0 = time.perf_counter()
    r = fn()
    stages[name] = time.perf_counter() - t0
    return r


def stepwise(c, params):
    st = {}
    rids, rows, aln_off, scores = _timed(st, "find", lambda: c.find_overlaps(**params))
    prim, rec_of_row = _timed(st, "pair", lambda: api.pair_rows(rows))
    rows_e, ext, ext_sc = _timed(st, "extend", lambda: c.extend_overlaps(rows[prim]))
    h = _timed(st, "align", lambda: c.align_dev(rows_e))
    m = _timed(st, "mirror", h.mirror)
    h.close()
    args = _timed(st, "job_args", lambda: api.paired_job_args(rids, aln_off, rec_of_row, m.ok))
    return st, m, dict(primaries=rows_e, rids=rids, aln_off=aln_off, rec_of_row=rec_of_row, args=args)


def pairs(c, params, core=None):
    st = {}
    p = _timed(st, "find_pair_extend", lambda: c.find_overlap_pairs(**params) if core is None else c.find_overlap_pairs(core=core, **params))
    m = _timed(st, "align_mirror", p.align)
    return st, m, p


def summary(runs):
    keys = list(runs[0])
    out = {}
    for k in keys + ["total"]:
        v = [sum(r.values()) if k == "total" else r[k] for r in runs]
        out[k] = {"median_s": float(np.median(v)), "min_s": min(v), "max_s": max(v)}
    return out


def anchors_of(call):
    """the `anchors` figure of the finder's HERRO_OVL_STATS line for one call (the line goes to the process's stderr)"""
    import re
    import tempfile
    sys.stderr.flush()
    keep = os.dup(2)
    os.environ["HERRO_OVL_STATS"] = "1"
    try:
        with tempfile.TemporaryFile() as f:
            os.dup2(f.fileno(), 2)
            try:
                r = call()
            finally:
                os.dup2(keep, 2)
            f.seek(0)
            text = f.read().decode(errors="replace")
    finally:
        os.close(keep)
        del os.environ["HERRO_OVL_STATS"]
    return r, int(re.findall(r"anchors=(\d+)", text)[-1])


def spread(runs):
    return {k: {"median_s": v["median_s"], "fastest_s": v["min_s"], "slowest_s": v["max_s"]} for k, v in summary(runs).items()}


def unmasked_only(c, params, reps):
    _, m, p = pairs(c, params)
    n_pairs = p.n_pairs
    m.close(); p.close()
    runs = []
    for _ in range(reps):
        st, m, p = pairs(c, params)
        m.close(); p.close()
        runs.append(st)
    print(json.dumps({"lib": os.path.basename(os.path.dirname(api.LIB_PATH)) + "/" + os.path.basename(api.LIB_PATH), "call": "find_overlap_pairs -> align",
                      "pairs": n_pairs, "reps": reps, **spread(runs)}), flush=True)


def shards(c, sb, params, a):
    lens = np.diff(np.asarray(sb.off).astype(np.int64))
    (st0, m, p), all_anchors = anchors_of(lambda: pairs(c, params))           # warm-up of the unmasked calls
    all_pairs, all_rows = p.n_pairs, p.n_rows
    m.close(); p.close()
    out = []
    g = 1
    while g <= a.shards:
        mask = shard.core_masks(lens, a.target_len, g)[0]
        (_, m, p), anchors = anchors_of(lambda: pairs(c, params, core=mask))  # warm-up of the masked calls
        n_pairs, n_rows, failed = p.n_pairs, p.n_rows, m.failed
        m.close(); p.close()
        runs_u, runs_m = [], []
        for _ in range(a.reps):
            st, m, p = pairs(c, params)
            m.close(); p.close()
            runs_u.append(st)
            st, m, p = pairs(c, params, core=mask)
            m.close(); p.close()
            runs_m.append(st)
        su, sm = spread(runs_u), spread(runs_m)
        out.append({"shards": g, "core_reads": int(np.count_nonzero(mask)), "anchors": anchors, "pairs": n_pairs, "rows": n_rows, "failed_records": failed,
                    "pairs_kept": n_pairs / max(all_pairs, 1), "unmasked": su, "masked": sm,
                    "masked_over_unmasked_median": sm["total"]["median_s"] / su["total"]["median_s"],
                    "align_masked_over_unmasked_median": sm["align_mirror"]["median_s"] / su["align_mirror"]["median_s"]})
        g *= 2
    return {"shape": {"targets": a.targets, "target_len": a.target_len, "overlaps": a.overlaps, "reads": int(sb.n_reads), "bases": int(sb.off[-1])},
            "params": params, "reps": a.reps, "unmasked_anchors": all_anchors, "unmasked_pairs": all_pairs, "unmasked_rows": all_rows,
            "what": "reads -> mirrored alignments (find_overlap_pairs -> align) for shard 0 of core_masks, alternating with the unmasked calls", "per_shards": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", type=int, default=256)
    ap.add_argument("--overlaps", type=int, default=32)
    ap.add_argument("--target-len", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="default: profiles/front_pairs_rate.json, profiles/front_core_rate.json with --shards")
    ap.add_argument("--shards", type=int, default=0, help="G: masked against unmasked pair calls for shard 0 of 1, 2, 4 .. G shards")
    ap.add_argument("--unmasked", action="store_true", help="the unmasked pair calls alone, one JSON line (A/B of two libraries by HERRO_LIB)")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "front_core_rate.json" if a.shards else "front_pairs_rate.json")
    params = dict(max_occ=128, min_score=100)
    c = api.Context(0)                                       # (raises without a device)
    sb = synth.generate_parallel(a.targets, a.target_len, a.overlaps, chunk=64)
    c.set_reads(sb.seq, sb.qual, sb.off)
    if a.unmasked:
        unmasked_only(c, params, a.reps)
        c.close()
        return
    if a.shards:
        res = shards(c, sb, params, a)
        print(json.dumps(res), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")
        c.close()
        return

    # warm-up of each chain; the results compared once
    _, m_s, s = stepwise(c, params)
    _, m_p, p = pairs(c, params)
    same = (np.array_equal(p.primaries, s["primaries"]) and np.array_equal(p.rids, s["rids"]) and np.array_equal(p.aln_off, s["aln_off"])
            and np.array_equal(p.rec_of_row, s["rec_of_row"]) and np.array_equal(m_p.rows, m_s.rows) and np.array_equal(m_p.n_ops, m_s.n_ops)
            and np.array_equal(m_p.scores, m_s.scores))
    n_rows, n_pairs, failed = len(p.rec_of_row), p.n_pairs, m_p.failed
    for x in (m_s, m_p, p):
        x.close()
    if not same:
        raise SystemExit("the two chains disagree")
    runs_s, runs_p = [], []
    for _ in range(a.reps):
        st, m, _ = stepwise(c, params)
        m.close()
        runs_s.append(st)
        st, m, h = pairs(c, params)
        m.close()
        h.close()
        runs_p.append(st)
    ss, sp = summary(runs_s), summary(runs_p)
    ts = [sum(r.values()) for r in runs_s]
    tp = [sum(r.values()) for r in runs_p]
    res = {"shape": {"targets": a.targets, "target_len": a.target_len, "overlaps": a.overlaps, "reads": int(sb.n_reads), "bases": int(sb.off[-1])},
           "params": params, "reps": a.reps, "rows": n_rows, "pairs": n_pairs, "failed_records": failed, "results_equal": True,
           "stepwise": ss, "pairs_calls": sp,
           "stepwise_over_pairs_median": ss["total"]["median_s"] / sp["total"]["median_s"],
           # faster beyond the spread of the same run: the slowest run of the pair calls below the fastest of the stepwise chain
           "beyond_spread": max(tp) < min(ts)}
    text = json.dumps(res, indent=1)
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    c.close()


if __name__ == "__main__":
    main()
