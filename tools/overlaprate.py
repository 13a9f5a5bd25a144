"""Rate of herro_find_overlaps (csrc/overlap_dev.hip): bases sketched, anchors and overlap records per second for the whole
call (sketch, both sorts, chaining, results back; the call returns when the device is done, so the wall clock around it is the
call), next to herro_align_overlaps on the records it emitted.  Two sets: the bench's shape (targets of 4096 bp with 32
overlaps each) and reads of >= 30 kb.  Prints one JSON line per set; run it under `rocprofv3 --kernel-trace --stats` for the
kernels alone.
--occ-frac-ppm N: every set is measured three times on one context — with the fixed cut, with the cut taken from the index (occ_frac_ppm = N)
and with the fixed cut set to the value the index gave, so that the last two differ by the census and the pick alone (`occ_share`).
--occ-dist N [--rescue-max-occ M]: every call rescues high-frequency minimizers (Context.set_seed_rescue; 200 = minimap2 -e200); the sizes gain
resc_high, resc_rescued and resc_anchors.
--lookback N: every call chains over the N nearest predecessors of an anchor (Context.set_chain_lookback; a multiple of 64 in 64 .. 1024, 64 = the
default and its kernels); the sizes gain chain_lookback and chain_chained when N is not 64.
--index-kmers N [--occ-ranges R] (or --index-blocks B: the least N that gives no more than B read blocks): every set is measured with the index
in one piece and in parts of at most N k-mers (Context.set_index_parts) on one context; a last line has both times, their ratio, the time and share
of the occurrence pass and the `OVLPART` line's figures (part_blocks, part_pairs, part_ranges, part_peak_bytes).
--tandem: only read pairs around tandem arrays (--tandem-pairs 64 pairs of flank + unit x copies + flank bases, two copies of one genome each with 1 %
substitutions), the shape a look-back of 64 cuts short; `pair_coverage` is the mean share of the target an overlap between the two reads of a
pair covers — the true overlap is the whole read.
--deep: one short genome under many reads (--deep-reads 200 of --deep-len 400 bases), the shape a fixed cut below the depth finds nothing in.

    python tools/overlaprate.py [--targets 256] [--long-targets 8] [--reps 5] [--no-align] [--occ-frac-ppm 5000] [--occ-dist 200] [--lookback 256] [--index-kmers N] [--occ-ranges R] [--index-blocks B] [--tandem] [--deep]"""
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
    sizes = {}
    for tag, prefix in (("OVL", ""), ("OVLOCC", "occ_"), ("OVLRESC", "resc_"), ("OVLCHAIN", "chain_"), ("OVLPART", "part_")):
        m = re.search(tag + r" (.*)", text)
        if m:
            sizes.update({prefix + k: int(v) for k, v in (kv.split("=") for kv in m.group(1).split())})
    return r, sizes


class Deep:
    """n reads of one genome of L bases with 0.5 % substitutions, every third one reversed and complemented: what set_reads takes"""

    def __init__(self, n, L, seed=43):
        rng = np.random.default_rng(seed)
        g = rng.integers(0, 4, L)
        comp = bytes.maketrans(b"ACGT", b"TGCA")
        reads = []
        for r in range(n):
            x = g.copy()
            at = np.flatnonzero(rng.random(L) < 0.005)
            x[at] = (x[at] + rng.integers(1, 4, len(at))) % 4
            b = bytes(b"ACGT"[v] for v in x)
            reads.append(b.translate(comp)[::-1] if r % 3 == 2 else b)
        self.n_reads = n
        self.seq = np.frombuffer(b"".join(reads), np.uint8)
        self.qual = np.full(len(self.seq), 40 + 33, np.uint8)
        self.off = (np.arange(n + 1) * L).astype(np.uint64)


class Tandem:
    """n read pairs, each two copies with 1 % substitutions of flank random bases + a unit of `unit` bases x copies + flank random bases
    (the generator of tests/lookback_cases.py, one seed per pair)"""

    def __init__(self, n, unit, copies, flank, seed=5):
        reads = []
        for p in range(n):
            rng = np.random.default_rng(seed + p)
            u = rng.integers(0, 4, unit)
            g = np.concatenate([rng.integers(0, 4, flank), np.tile(u, copies), rng.integers(0, 4, flank)])
            for _ in range(2):
                r = g.copy()
                m = rng.random(len(r)) < 0.01
                r[m] = (r[m] + rng.integers(1, 4, m.sum())) & 3
                reads.append(bytes(b"ACGT"[x] for x in r))
        self.n_reads = len(reads)
        self.seq = np.frombuffer(b"".join(reads), np.uint8)
        self.qual = np.full(len(self.seq), 40 + 33, np.uint8)
        self.off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)


def pair_coverage(rows):
    """mean (tend - tstart) / tlen over the records between the two reads of a Tandem pair (reads 2 p and 2 p + 1); None: no such record"""
    own = rows[(rows[:, 0] >> 1) == (rows[:, 5] >> 1)]
    return float(np.mean((own[:, 8].astype(np.int64) - own[:, 7]) / own[:, 6])) if len(own) else None


def store_kmers(sb, k=25, w=17) -> int:
    """k-mers of the reads that have a window (the block rule's nk, include/herro_amd.h, "an index in parts")"""
    lens = np.diff(np.asarray(sb.off).astype(np.int64))
    return int(np.where(lens >= k + w - 1, lens - k + 1, 0).sum())


def measure_parts(c, name, sb, reps, params, index_kmers, occ_ranges):
    """the call with its index in parts beside the unpartitioned call on the same reads: the times, their ratio, the OVLPART line and pass A's share
    (the occurrence pass alone is what the census hook runs under the setting)"""
    off = measure_on(c, name, sb, reps, params, False)
    on = measure_on(c, name + f" index_kmers={index_kmers}", sb, reps, dict(params, index_kmers=index_kmers, occ_ranges=occ_ranges), False)
    census = dict({k: v for k, v in params.items() if k in ("k", "w")}, occ_frac_ppm=5000, index_kmers=index_kmers, occ_ranges=occ_ranges)
    c.occ_census(**census)
    ta = []
    for _ in range(reps):
        t0 = time.perf_counter()
        c.occ_census(**census)
        ta.append(time.perf_counter() - t0)
    same = all(on.get(f) == off.get(f) for f in ("kmers", "minimizers", "anchors", "groups", "chained", "records"))
    print(json.dumps({"set": name, "index_kmers": index_kmers, "occ_ranges": occ_ranges, "seconds_off": off["seconds_median"],
                      "seconds_parts": on["seconds_median"], "parts_over_off": on["seconds_median"] / off["seconds_median"],
                      "seconds_pass_a": float(np.median(ta)), "pass_a_share": float(np.median(ta)) / on["seconds_median"], "same_figures": same,
                      **{k: v for k, v in on.items() if k.startswith("part_")}}), flush=True)


def measure(name, sb, reps, params, align, occ_frac_ppm=0, rescue=(0, 0), lookback=0, index_kmers=0, occ_ranges=0, index_blocks=0):
    c = api.Context(0)
    c.set_reads(sb.seq, sb.qual, sb.off)
    if lookback:
        c.set_chain_lookback(lookback)
        name += f" lookback={lookback}"
    if rescue[0]:
        c.set_seed_rescue(*rescue)
        name += f" occ_dist={rescue[0]}"
    if index_blocks:                               # the least part size that gives no more read blocks (the count falls as the size grows)
        k, w = params.get("k", 25), params.get("w", 17)
        lens = np.diff(np.asarray(sb.off).astype(np.int64))
        lo, hi = 1, 2 * max(store_kmers(sb, k, w), 1)      # (hi: one block)
        while lo < hi:
            mid = (lo + hi) // 2
            if len(api.index_plan(lens, k, w, mid)) - 1 <= index_blocks:
                hi = mid
            else:
                lo = mid + 1
        index_kmers = lo
    if index_kmers:
        measure_parts(c, name, sb, reps, dict(params, **({"occ_frac_ppm": occ_frac_ppm} if occ_frac_ppm else {})), index_kmers, occ_ranges)
    elif occ_frac_ppm:
        fixed = measure_on(c, name, sb, reps, params, False)
        frac = measure_on(c, name, sb, reps, dict({k: v for k, v in params.items() if k != "max_occ"}, occ_frac_ppm=occ_frac_ppm), align)
        same = measure_on(c, name, sb, reps, dict(params, max_occ=frac["occ_cut"]), False)
        print(json.dumps({"set": name, "occ_frac_ppm": occ_frac_ppm, "cut": frac["occ_cut"], "seconds_fixed": fixed["seconds_median"],
                          "seconds_frac": frac["seconds_median"], "seconds_fixed_at_the_cut": same["seconds_median"],
                          "same_records": frac["records"] == same["records"] and frac["anchors"] == same["anchors"],
                          "occ_share": (frac["seconds_median"] - same["seconds_median"]) / frac["seconds_median"]}), flush=True)
    else:
        measure_on(c, name, sb, reps, params, align)
    c.close()


def measure_on(c, name, sb, reps, params, align):
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
    if isinstance(sb, Tandem):
        res["pair_coverage"] = pair_coverage(rows)
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
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", type=int, default=256)
    ap.add_argument("--overlaps", type=int, default=32)
    ap.add_argument("--target-len", type=int, default=4096)
    ap.add_argument("--long-targets", type=int, default=8)
    ap.add_argument("--long-len", type=int, default=30000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-align", action="store_true")
    ap.add_argument("--occ-frac-ppm", type=int, default=0, help="also measure with the cut taken from the index (5000 = minimap2 -f0.005)")
    ap.add_argument("--occ-dist", type=int, default=0, help="rescue high-frequency minimizers, about one per N bases (200 = minimap2 -e200)")
    ap.add_argument("--rescue-max-occ", type=int, default=0, help="with --occ-dist: hashes above this many occurrences are never rescued (0: 4095)")
    ap.add_argument("--lookback", type=int, default=0, help="chain over the N nearest predecessors (a multiple of 64 in 64 .. 1024; 0: the default, 64)")
    ap.add_argument("--index-kmers", type=int, default=0, help="also measure with the index in parts of at most N k-mers (Context.set_index_parts)")
    ap.add_argument("--occ-ranges", type=int, default=0, help="with --index-kmers / --index-blocks: the hash ranges of the occurrence pass (0: chosen by the library)")
    ap.add_argument("--index-blocks", type=int, default=0, help="--index-kmers chosen so that the store falls into B read blocks")
    ap.add_argument("--tandem", action="store_true", help="only the tandem shape: read pairs around tandem arrays")
    ap.add_argument("--tandem-pairs", type=int, default=64)
    ap.add_argument("--tandem-unit", type=int, default=40)
    ap.add_argument("--tandem-copies", type=int, default=30)
    ap.add_argument("--tandem-flank", type=int, default=2400)
    ap.add_argument("--deep", action="store_true", help="only the deep shape: one short genome under many reads")
    ap.add_argument("--deep-reads", type=int, default=200)
    ap.add_argument("--deep-len", type=int, default=400)
    a = ap.parse_args()
    rescue = (a.occ_dist, a.rescue_max_occ)
    if a.tandem:
        measure("tandem", Tandem(a.tandem_pairs, a.tandem_unit, a.tandem_copies, a.tandem_flank), a.reps, dict(k=15, w=5, max_occ=4096, min_score=100),
                not a.no_align, a.occ_frac_ppm, rescue, a.lookback, a.index_kmers, a.occ_ranges, a.index_blocks)
        return
    if a.deep:
        measure("deep", Deep(a.deep_reads, a.deep_len), a.reps, dict(k=15, w=5, max_occ=128, min_score=60), not a.no_align, a.occ_frac_ppm, rescue, a.lookback, a.index_kmers, a.occ_ranges, a.index_blocks)
        return
    if a.targets:
        measure("bench shape", synth.generate_parallel(a.targets, a.target_len, a.overlaps, chunk=64), a.reps,
                dict(max_occ=128, min_score=100), not a.no_align, a.occ_frac_ppm, rescue, a.lookback, a.index_kmers, a.occ_ranges, a.index_blocks)
    if a.long_targets:
        measure(">= 30 kb", synth.generate_parallel(a.long_targets, a.long_len, 16, chunk=4, flank_min=200, flank_max=400), a.reps,
                dict(max_occ=128), not a.no_align, a.occ_frac_ppm, rescue, a.lookback, a.index_kmers, a.occ_ranges, a.index_blocks)


if __name__ == "__main__":
    main()
