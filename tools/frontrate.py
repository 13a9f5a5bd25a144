"""Reads -> (mirrored alignments, job arguments): the stepwise chain of the Python binding against the pair calls of the C ABI
(herro_find_overlap_pairs, herro_pairs_align; DESIGN.md §10, "Pairs on the device"), in one process, the two chains alternating.

    stepwise   find_overlaps -> pair_rows -> extend_overlaps(rows[prim]) -> align_dev -> mirror -> paired_job_args
    pairs      find_overlap_pairs -> OverlapPairs.align        (the job arguments are the handle's table)

Host clock around the synchronous calls; every figure is the median of --reps runs after one warm-up of each chain, with min .. max
beside it, the stages separately.  The two chains' results are compared once.  Needs a GPU (no fallback).  The bench's shape by default:
256 targets x 4096 bp x 32 overlaps, max_occ 128, min_score 100.

    python tools/frontrate.py [--targets 256] [--reps 5] [--out profiles/front_pairs_rate.json]"""
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


def pairs(c, params):
    st = {}
    p = _timed(st, "find_pair_extend", lambda: c.find_overlap_pairs(**params))
    m = _timed(st, "align_mirror", p.align)
    return st, m, p


def summary(runs):
    keys = list(runs[0])
    out = {}
    for k in keys + ["total"]:
        v = [sum(r.values()) if k == "total" else r[k] for r in runs]
        out[k] = {"median_s": float(np.median(v)), "min_s": min(v), "max_s": max(v)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", type=int, default=256)
    ap.add_argument("--overlaps", type=int, default=32)
    ap.add_argument("--target-len", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "front_pairs_rate.json"))
    a = ap.parse_args()
    params = dict(max_occ=128, min_score=100)
    c = api.Context(0)                                       # (raises without a device)
    sb = synth.generate_parallel(a.targets, a.target_len, a.overlaps, chunk=64)
    c.set_reads(sb.seq, sb.qual, sb.off)

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
