"""Capacity cases: seeded inputs whose windows cross the LDS capacities of the pileup and consensus kernels (csrc/pileup.hip), at
insertion rates near raw ONT reads rather than the synthetic defaults.  Above a cap a kernel takes its second path (several passes,
or global memory instead of LDS); the named cases of the other tests stay below every cap.

Shared by test_capacity_cases.py (no device: every case crosses what it claims, with the caps read from the source) and
test_gpu_capacity.py (the kernels against the oracle on these cases)."""
import os
import re

import numpy as np

import oracle_lib as O
from herro_amd import api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PILEUP = os.path.join(ROOT, "herro_amd", "csrc", "pileup.hip")
API_JOB = os.path.join(ROOT, "herro_amd", "csrc", "api_job.h")
MAX_COLS = 30   # selected overlaps per window (columns 1 .. 30 of the pileup)

# crosses: RW_ICAP   k_rows runs its insertion rows in several passes and reads the informative flags back from global memory
#          CP_ICAP   k_consensus_p keeps the insertion-row votes in global memory (emit's non-FAST branch)
#          CP_OCAP   k_consensus_p writes the corrected bases as byte stores (L' here; the corrected length on the device)
#          QEVCAP    k_quals does not stage the insertion events in LDS
#          FUSED_ROWS  a window above the informative rows of the fused f16 stack (layer-by-layer kernels)
CASES = {
    "A_w4096_ont": dict(W=4096, n=2, ov=30, kw=dict(p_sub=0.03, p_ins=0.06, p_del=0.04),
                        crosses=("RW_ICAP", "CP_ICAP", "QEVCAP", "FUSED_ROWS")),
    "B_w8192_ont": dict(W=8192, n=2, ov=30, kw=dict(p_sub=0.03, p_ins=0.05, p_del=0.03),
                        crosses=("RW_ICAP", "CP_ICAP", "CP_OCAP", "QEVCAP", "FUSED_ROWS")),
    "C_w8192_mid": dict(W=8192, n=2, ov=20, kw=dict(p_sub=0.02, p_ins=0.02, p_del=0.02),
                        crosses=("RW_ICAP", "CP_OCAP", "QEVCAP")),
    "D_w2048": dict(W=2048, n=2, ov=34, kw=dict(p_sub=0.006, p_ins=0.08, p_del=0.03),
                    crosses=("RW_ICAP", "QEVCAP")),
    "E_w1000_deep": dict(W=1000, n=2, ov=40, kw=dict(p_sub=0.02, p_ins=0.1, p_del=0.03),
                         crosses=("QEVCAP",)),
}
# the caps a case must stay BELOW (the pairings a case exists for: C and D run k_rows in passes with the consensus votes in LDS; E runs
# k_quals past its event cap with k_rows in one pass)
STAYS_UNDER = {"C_w8192_mid": ("CP_ICAP",), "D_w2048": ("CP_ICAP",), "E_w1000_deep": ("RW_ICAP", "CP_ICAP")}


def target_len(W):
    return 2 * W + W // 3 + 17   # two full windows and a ragged tail


def seed(name):
    return synth.SEED + sum(map(ord, name))


def generate(name):
    cs = CASES[name]
    return synth.generate(cs["n"], target_len(cs["W"]), cs["ov"], seed=seed(name), **cs["kw"])


def caps():
    """The capacities as the kernels are compiled with them: `constexpr uint32_t NAME = N;` in pileup.hip, HERRO_RW_ICAP's default, and
    the fused f16 stack's row limit (FUSED_MAX_SIB sibling tiles of 64 rows, api_job.h)."""
    src = open(PILEUP).read()
    val = {n: int(v) for n, v in re.findall(r"constexpr uint32_t (\w+) = (\d+)u?;", src)}
    m = re.search(r"#define HERRO_RW_ICAP (\d+)", src)
    assert m and re.search(r"constexpr uint32_t RW_ICAP = HERRO_RW_ICAP;", src), "k_rows' insertion-row cap moved"
    out = {"RW_ICAP": int(m.group(1))}
    for k in ("CP_ICAP", "CP_OCAP", "QEVCAP"):
        assert k in val, f"{k} is no longer a constexpr of pileup.hip"
        out[k] = val[k]
    m = re.search(r"constexpr uint32_t FUSED_MAX_SIB = (\d+);", open(API_JOB).read())
    assert m, "FUSED_MAX_SIB moved"
    out["FUSED_ROWS"] = int(m.group(1)) * 64
    return out


def oracle_windows(sb, store, W):
    """[(target, window index, OracleWindow, FeatResult)] of every window, target order."""
    out = []
    for t in range(sb.n_targets):
        rid, rows, cigs = O.target_alignments(sb, t)
        res = store.extract_features(rid, rows, cigs, W)
        for wi in range(len(res)):
            out.append((t, wi, res.window(wi), res))
    return out


def insertion_events(sb, W):
    """Per window (job order): insertion ops of the selected overlaps' op slices, from the host-built job (no device).  Counts only the
    ops strictly inside a slice (its first and last op may lie partly outside the window), so it is a lower bound of the events
    k_quals stages — when the window's selected overlaps are the oracle's."""
    store = O.store_from_synth(sb)
    sel = [set(int(q) for q in ow.qids) for _, _, ow, _ in oracle_windows(sb, store, W)]
    lens = (sb.off[1:] - sb.off[:-1]).astype(np.uint32)
    c = api.HostContext(lens)
    job = api.job_from_synth(c, sb, W)
    try:
        arr = c.job_arrays(job)
    finally:
        job.close()
        c.close()
    ops, ow = arr["ops"], arr["ow"]
    assert len(arr["win"]) == len(sel)
    ev = np.zeros(len(sel), np.int64)
    for d in ow:
        w, b, n = int(d["win"]), int(d["op_begin"]), int(d["op_cnt"])
        if int(d["qid"]) in sel[w] and n > 2:
            ev[w] += int(((ops[b + 1:b + n - 1] & 3) == 1).sum())
    return ev


def oracle_stats(sb, W):
    """Per window: insertion rows (L' - window length), L', informative rows — from the oracle's features."""
    store = O.store_from_synth(sb)
    irows, lp, nsup = [], [], []
    for _, _, ow, _ in oracle_windows(sb, store, W):
        L = ow.bases.shape[0]
        lp.append(L)
        irows.append(int((ow.bases[:, 0] == ord("*")).sum()))
        nsup.append(len(ow.sup_pos))
    return dict(irows=np.array(irows), lp=np.array(lp), nsup=np.array(nsup))


_CNT = np.full(256, 255, np.uint8)
for _ch, _v in zip(b"ACGT*acgt#", (0, 1, 2, 3, 4, 0, 1, 2, 3, 4)):
    _CNT[_ch] = _v


def corrected_window(ow, base_logits):
    """consensus.rs:113-205 on one window of the oracle's features: the corrected bases (bytes; '' for a window with < 2 alignments).
    Only the lengths of these are used (the FASTA itself is compared with the oracle's own decoder)."""
    n_alns = min(ow.n_alns, MAX_COLS)
    if n_alns < 2:
        return b""
    tok = _CNT[ow.bases[:, :n_alns + 1]]
    counts = np.stack([(tok == k).sum(axis=1) for k in range(5)], axis=1)
    order = np.argsort(-counts, axis=1, kind="stable")
    c0 = np.take_along_axis(counts, order[:, :1], 1)[:, 0]
    c1 = np.take_along_axis(counts, order[:, 1:2], 1)[:, 0]
    tb = tok[:, 0]
    vote = np.where((c0 < 2) | ((c0 == c1) & ((order[:, 0] == tb) | (order[:, 1] == tb))), tb, order[:, 0])
    tidx = np.flatnonzero(tok[:, 0] != 4)
    rows = tidx[ow.sup_pos.astype(np.int64)] + ow.sup_ins.astype(np.int64)
    for k, r in enumerate(rows):
        v = base_logits[k]
        arg = 0
        for c in range(1, 5):
            if np.isnan(v[c]) or (not np.isnan(v[arg]) and v[c] >= v[arg]):
                arg = c
        vote[r] = arg
    return bytes(b"ACGT*"[int(x)] for x in vote if x != 4)
