"""Width cases: hand-built inputs that reach the widths of the packed fields of the feature kernels (csrc/pileup.hip, csrc/job_dev.h) and the
fallbacks behind them — the 16-bit halves of k_cols' shared scan, the 16-bit lengths of an insertion event, the 20 + 12 bits of a directory
word (k_rfq counts where a word is flagged), the 6-bit row counts of sup_nr and the tiles of the largest window the format admits.  The data
of the other tests are error-rate data (many short indels, spread evenly) and reach none of them; test_width_cases.py holds the census that
says so.

A case is a random target and queries that ARE the target but for a planned list of (position, inserted length) per query, on both strands,
with rows and CIGAR text written from the plan — no generator, no noise model.  Two kinds of planted disagreement give the windows
informative rows (two symbols seen at least 3 times in the 31 columns, features.rs:712):
  * SNPs: half of the queries carry another base at a planned target position (4 + the target against 4);
  * insertion columns: the queries that carry the insertions come in two families whose inserted bases differ in every column (2 against 2
    against the '*' of the plain queries and of the target: nothing reaches 3 but '*'), EXCEPT in a few planned columns where one or both
    queries of the second family carry the first family's base (3 or 4 against 5 '*': an informative insertion row).  Were the inserted
    bases equal everywhere, every one of the 65 000 insertion rows of a case would be informative; were they random, none.
`largest_window` has two carriers only, so its insertion rows cannot be informative (2 < 3) whatever they hold: its informative rows are the
SNPs' base rows, which stand between the insertion rows (the receptive field of each reaches two insertion rows to either side).

Shared by test_width_cases.py (no device: every case crosses what it claims, the old data sets cross nothing) and test_gpu_width.py."""
import os
import re

import numpy as np

import oracle_lib as O
from herro_amd import api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PILEUP = os.path.join(ROOT, "herro_amd", "csrc", "pileup.hip")
LONGEST_KEPT = 50   # features.rs:315-324: an overlap leaves a window when one indel there is longer

# ins: insertions in front of which the carriers share the target: (first window position, count, length) — one insertion of `length` bases
#      behind each of `count` consecutive positions of window `win`
# carriers / plain: queries with / without the insertions (strands alternate in both groups)
# nsup: informative rows per window the plan aims at (base rows from SNPs + insertion rows from agreeing columns), [window 0, the others]
CASES = {
    # one insertion above 16 bits inside window 1 of 3: the slice has qlen >= 65536 (two scans), is not staged, its event's lengths are clamped, and it is
    # dropped; windows 0 and 2 of the same overlaps and the two plain queries in window 1 are ordinary.  At the smallest and at a large k_cols<QI, NWI>
    "dropped_long_insertion_w64": dict(W=64, tl=3 * 64 + 64 // 3 + 17, win=1, ins=(64 // 2, 1, 66000), carriers=6, plain=2, nsup=(12, 12)),
    "dropped_long_insertion_w4096": dict(W=4096, tl=3 * 4096 + 4096 // 3 + 17, win=1, ins=(4096 // 2, 1, 66000), carriers=6, plain=2, nsup=(40, 40)),
    # 1300 insertions of 50 bases (the longest a kept slice may hold): the slice's query span is 2048 + 65000 >= 65536 and it is KEPT — planes, events and
    # directory of a slice built by the two-scan branch are all consumed.  51 W >= 65536 needs W >= 1286
    "kept_wide_slice_w2048": dict(W=2048, tl=2 * 2048 + 2048 // 3 + 17, win=0, ins=(0, 1300, 50), carriers=4, plain=4, nsup=(90, 40)),
    # 4200 one-base insertions: the events in front of a word pass 0xfff inside the column — fitting directory words in front, flagged ones behind
    "directory_events_w8192": dict(W=8192, tl=8192 + 8192 // 3 + 17, win=0, ins=(0, 4200, 1), carriers=4, plain=4, nsup=(90, 40)),
    # 50 bases behind every one of the 8192 positions of the window (the insertion behind the last position stays with this window: windowing.rs cuts a slice
    # behind the insertions that follow the op that reaches the window's end): 8192 positions of 51 rows = 417 792 rows in 408 tiles, every 6-bit field of sup_nr
    # at 51, 8192 events per slice, and an ordinary (ragged) window behind it.  Window 0 has more informative rows than k_rows stages (RW_SUPCAP).  The oracle
    # takes 0.3 s for it, so the window is not shrunk to 4096
    "largest_window_w8192": dict(W=8192, tl=8192 + 8192 // 3 + 17, win=0, ins=(0, 8192, 50), carriers=2, plain=6, nsup=(300, 40)),
}
COMP = np.array([3, 2, 1, 0], np.uint8)
ASCII = np.frombuffer(b"ACGT", np.uint8)


def seed(name):
    return synth.SEED + 7 * sum(map(ord, name))


def plan(name):
    """The case's plan: the insertion positions (absolute, sorted) and length, per window the SNP positions, and the (insertion, column) pairs where the
    second family of carriers agrees with the first (kind 0: both of its queries, 1: one of them)."""
    cs = CASES[name]
    W, tl = cs["W"], cs["tl"]
    g = np.random.default_rng(seed(name))
    p0, cnt, length = cs["ins"]
    pos = cs["win"] * W + p0 + np.arange(cnt)
    n_win = -(-tl // W)
    kept = length <= LONGEST_KEPT
    two_families = kept and cs["carriers"] >= 4
    snps, agree = [], []
    for w in range(n_win):
        lo, hi = w * W, min((w + 1) * W, tl)
        want = cs["nsup"][0] if w == cs["win"] else cs["nsup"][1]
        n_ins_rows = min(want // 2, 64) if (two_families and w == cs["win"]) else 0
        n_snp = min(want - n_ins_rows, hi - lo)
        snps.append(np.sort(g.choice(np.arange(lo, hi), n_snp, replace=False)))
        if n_ins_rows:
            cols = g.choice(cnt * length, n_ins_rows, replace=False)
            agree = [(int(c) // length, int(c) % length, k & 1) for k, c in enumerate(np.sort(cols))]
    return dict(pos=pos, length=length, snps=snps, agree=agree, n_win=n_win)


def build(name):
    """(SynthBatch, W): read 0 is the target (the only one), reads 1 .. the queries — carriers first."""
    cs = CASES[name]
    W, tl = cs["W"], cs["tl"]
    pl = plan(name)
    g = np.random.default_rng(seed(name) + 1)
    target = g.integers(0, 4, tl).astype(np.uint8)
    pos, length = pl["pos"], pl["length"]
    n_q = cs["carriers"] + cs["plain"]
    fam0 = g.integers(0, 4, (len(pos), length)).astype(np.uint8)                 # the first family's inserted bases
    fam1 = ((fam0 + g.integers(1, 4, fam0.shape)) & 3).astype(np.uint8)          # the second family's: another base in every column
    snp_pos = np.concatenate(pl["snps"])
    alt = ((target[snp_pos] + g.integers(1, 4, len(snp_pos))) & 3).astype(np.uint8)
    # the text: M up to and including each insertion's position, the insertion, ... the rest of the target
    runs = np.diff(np.concatenate([[-1], pos]))
    cigar_ins = ("".join(f"{int(r)}M{length}I" for r in runs) + f"{tl - 1 - int(pos[-1])}M").encode()
    cigar_plain = f"{tl}M".encode()
    assert pos[-1] < tl - 1
    out_idx = np.arange(tl) + np.searchsorted(pos, np.arange(tl), side="left") * length   # a target base's place in a carrier
    reads, rows, cigs = [target], [], []
    for k in range(n_q):
        carrier = k < cs["carriers"]
        strand = k & 1
        t = target.copy()
        if _has_snp(k, cs):
            t[snp_pos] = alt
        if carrier:
            ins = (fam1 if _second_family(k, cs) else fam0).copy()
            if length > LONGEST_KEPT:
                ins = g.integers(0, 4, ins.shape).astype(np.uint8)                # a dropped slice: nobody reads these
            elif _second_family(k, cs):
                for i, c, kind in pl["agree"]:
                    if kind == 0 or k == _second_family_first(cs):
                        ins[i, c] = fam0[i, c]
            a = np.empty(tl + len(pos) * length, np.uint8)
            a[out_idx] = t
            ins_idx = (out_idx[pos] + 1)[:, None] + np.arange(length)[None, :]
            a[ins_idx] = ins
        else:
            a = t
        stored = COMP[a[::-1]] if strand else a
        reads.append(stored)
        rows.append((1 + k, len(a), 0, len(a), strand, 0, tl, 0, tl))
        cigs.append(cigar_ins if carrier else cigar_plain)
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    seq = ASCII[np.concatenate(reads)]
    qual = g.integers(33 + 2, 33 + 60, len(seq)).astype(np.uint8)
    aln = np.zeros((n_q, 10), np.uint32)
    aln[:, :9] = np.array(rows, np.uint32)
    aln[:, 9] = [len(c) for c in cigs]
    cig_off = np.concatenate([[0], np.cumsum([len(c) for c in cigs])[:-1]]).astype(np.uint64)
    sb = synth.SynthBatch(seq=seq, qual=qual, off=off, aln=aln, cig_off=cig_off, cig=np.frombuffer(b"".join(cigs), np.uint8).copy(),
                          tgt_aln_off=np.array([0, n_q], np.uint64), tgt_rid=np.array([0], np.uint32))
    return sb, W


def _second_family(k, cs):
    """carriers 2, 3, 6, 7 .. (one of each strand in a group of four); with two carriers, the second one"""
    return k < cs["carriers"] and ((k >> 1) & 1 == 1 if cs["carriers"] >= 4 else k == 1)


def _second_family_first(cs):
    return 2 if cs["carriers"] >= 4 else 1


def _has_snp(k, cs):
    """half of the queries, both strands, carriers and plain ones among them: queries 1, 2 of every group of four"""
    return k % 4 in (1, 2)


# ---- the switches, read from the source ------------------------------------------------------------------------------------------------------------
def limits():
    """The widths and capacities as the kernels are compiled with them; an assertion fires when a source line moved."""
    src = open(PILEUP).read()
    out = {}
    m = re.search(r"const bool packed_scan = d\.qlen < (\d+)u;", src)
    assert m, "k_cols' packed_scan moved"
    out["SCAN"] = int(m.group(1))
    m = re.search(r"const bool staged = nqw <= qcap;", src)
    assert m, "k_cols' staged moved"
    m = re.search(r"ev\[idx\] = make_uint4\(\(\(uint32_t\)pos & 0xffffu\) \| \(min\(e, (0x[0-9a-f]+)u\) << 16\), q, codes, min\(len, (0x[0-9a-f]+)u\)\);", src)
    assert m, "k_cols' insertion event moved"
    out["EV_LEN"], out["EV_LEN_RAW"] = int(m.group(1), 16), int(m.group(2), 16)
    m = re.search(r"atomicMax\(&s_cov\[slot\], \(\(idx \+ 1u\) << 12\) \| min\(ev_before, (0x[0-9a-f]+)u\)\);", src)
    assert m, "k_cols' covering-op word moved"
    out["DIR_EV"] = int(m.group(1), 16)
    m = re.search(r"gd\[wi\] = \(dQ\[wi_i\] < \(1u << (\d+)\) && de < (0x[0-9a-f]+)u && !\(J\.dbg_flags & 1u\)\) \? \(dQ\[wi_i\] \| \(de << (\d+)\)\) : 0xffffffffu;", src)
    assert m and m.group(1) == m.group(3) and int(m.group(2), 16) == out["DIR_EV"], "k_cols' directory word moved"
    out["DIR_Q"] = 1 << int(m.group(1))
    m = re.search(r"constexpr uint32_t MDCAP = (\d+);", src)
    assert m, "MDCAP moved"
    out["MDCAP"] = int(m.group(1))
    m = re.search(r"inline uint32_t cols_qcap\(uint32_t nw\) \{ return nw \+ (\d+)u < (\d+)u \? nw \+ (\d+)u : (\d+)u; \}", src)
    assert m and m.group(1) == m.group(3) and m.group(2) == m.group(4), "cols_qcap moved"
    out["QCAP_ADD"], out["QCAP_MAX"] = int(m.group(1)), int(m.group(2))
    m = re.search(r"constexpr int LY_NT = (\d+)", src)
    m2 = re.search(r"constexpr uint32_t TCAP = 2 \* LY_NT;", src)
    assert m and m2, "TCAP moved"
    out["TCAP"] = 2 * int(m.group(1))
    m = re.search(r"constexpr uint32_t ROWCAP = HERRO_TILE;", src)
    m2 = re.search(r"#define HERRO_TILE (\d+)", open(os.path.join(ROOT, "herro_amd", "csrc", "job_dev.h")).read())
    assert m and m2, "ROWCAP moved"
    out["ROWCAP"] = int(m2.group(1))
    m = re.search(r"#define HERRO_RW_ICAP (\d+)", src)
    assert m and re.search(r"constexpr uint32_t RW_ICAP = HERRO_RW_ICAP;", src), "RW_ICAP moved"
    out["RW_ICAP"] = int(m.group(1))
    val = {n: int(v) for n, v in re.findall(r"constexpr uint32_t (\w+) = (\d+)u?;", src)}
    for k in ("QEVCAP", "CP_ICAP", "CP_OCAP", "RW_SUPCAP"):
        assert k in val, f"{k} is no longer a constexpr of pileup.hip"
        out[k] = val[k]
    assert re.search(r"rows \(1 \+ max insertion, <= 51\) of positions pos - 2, pos - 1, pos, pos \+ 1, 6 bits each", open(os.path.join(ROOT, "herro_amd", "csrc", "job_dev.h")).read()), \
        "sup_nr moved"
    out["NR_ROWS"] = 1 + LONGEST_KEPT   # the largest 6-bit field of sup_nr
    return out


def cols_qcap(lim, nw):
    return min(nw + lim["QCAP_ADD"], lim["QCAP_MAX"])


# ---- the census -----------------------------------------------------------------------------------------------------------------------------------
def host_job(sb, W):
    """The host-built job's arrays (no device)."""
    lens = (sb.off[1:] - sb.off[:-1]).astype(np.uint32)
    c = api.HostContext(lens)
    job = api.job_from_synth(c, sb, W)
    try:
        return c.job_arrays(job)
    finally:
        job.close()
        c.close()


def slice_walk(d, ops):
    """One slice as k_cols walks it: per op its type, effective length, and the window position, query index and insertion events in front of it."""
    n = int(d["op_cnt"])
    o = ops[int(d["op_begin"]):int(d["op_begin"]) + n].astype(np.int64)
    ty, ln = o & 3, o >> 2
    e = ln.copy()
    if n == 1:
        e[0] = int(d["end_off"]) - int(d["start_off"])
    else:
        e[0] = ln[0] - int(d["start_off"])
        e[-1] = int(d["end_off"])
    tadv = np.where((ty == 0) | (ty == 2), e, 0)
    qadv = np.where((ty == 0) | (ty == 1), e, 0)
    t = np.cumsum(tadv) - tadv
    q = np.cumsum(qadv) - qadv
    isI = ty == 1
    ev_before = np.cumsum(isI) - isI
    P = int(d["tstart"]) - int(d["wtstart"]) + t
    return dict(ty=ty, len=ln, e=e, P=P, q=q, ev_before=ev_before, n_ev=int(isI.sum()), t_total=int(tadv.sum()), q_total=int(qadv.sum()))


def directory_words(d, ops, lim, nw):
    """The directory words k_cols writes for a kept slice, restated on the host: per word of 32 window positions the query index of the first base at or
    behind its first position and the insertion events in front of it, read off the M / D op that covers that position (0 / 0 in front of the overlap,
    0 / all events behind it) — (dQ, de) as int64 arrays; a word is flagged where de >= DIR_EV or dQ >= DIR_Q."""
    s = slice_walk(d, ops)
    md = np.flatnonzero(((s["ty"] == 0) | (s["ty"] == 2)) & (s["e"] > 0))
    off = int(d["tstart"]) - int(d["wtstart"])
    end = off + s["t_total"]
    dQ = np.zeros(nw, np.int64)
    de = np.zeros(nw, np.int64)
    starts = s["P"][md]
    for wi in range(nw):
        ws = 32 * wi
        if ws < off:
            continue
        if ws >= min(end, int(d["wlen"])):
            de[wi] = s["n_ev"]
            continue
        k = md[np.searchsorted(starts, ws, side="right") - 1]
        dQ[wi] = s["q"][k] + (ws - s["P"][k] if s["ty"][k] == 0 else 0)
        de[wi] = s["ev_before"][k]
    return dQ, de


def census(sb, W, lim=None):
    """What the slices of a batch reach, from the host-built job and the oracle: a list of one dict per overlap-window slice (job order) with
    qlen, ops, batches of MDCAP ops, insertion events, the longest insertion op, two_scans / unstaged / clamped / flagged words / query index beyond the
    directory's field, and `kept` (the oracle selected the overlap for the window); and per window L', insertion rows, informative rows, informative
    insertion rows, tiles, the largest rows per position."""
    lim = lim or limits()
    arr = host_job(sb, W)
    ops, ows = arr["ops"], arr["ow"]
    nw = (W + 31) // 32
    store = O.store_from_synth(sb)
    wins = []
    for t in range(sb.n_targets):
        rid, rows, cigs = O.target_alignments(sb, t)
        res = store.extract_features(rid, rows, cigs, W)
        for wi in range(len(res)):
            ow = res.window(wi)
            star = ow.bases[:, 0] == ord("*")
            base_rows = np.flatnonzero(~star)
            per_pos = np.diff(np.concatenate([base_rows, [len(star)]])) if len(base_rows) else np.zeros(0, np.int64)
            wins.append(dict(qids=set(int(x) for x in ow.qids), n_alns=int(ow.n_alns), lp=int(len(star)), irows=int(star.sum()), nsup=len(ow.sup_pos),
                             nsup_ins=int((ow.sup_ins > 0).sum()), tiles=-(-len(star) // lim["ROWCAP"]), rows_per_pos=int(per_pos.max()) if len(per_pos) else 0,
                             events=0))
    assert len(wins) == len(arr["win"])
    slices = []
    for d in ows:
        s = slice_walk(d, ops)
        qbeg, qlen = int(d["qbeg"]), int(d["qlen"])
        nqw = ((qbeg + qlen) >> 5) - (qbeg >> 5) + 2
        isI = s["ty"] == 1
        long_indel = bool(((s["ty"] != 0) & (s["len"] > LONGEST_KEPT)).any())
        kept = int(d["qid"]) in wins[int(d["win"])]["qids"]
        rec = dict(win=int(d["win"]), qid=int(d["qid"]), strand=int(d["strand"]), qlen=qlen, ops=int(d["op_cnt"]), batches=-(-int(d["op_cnt"]) // lim["MDCAP"]),
                   n_ev=s["n_ev"], longest_ins=int(s["len"][isI].max()) if isI.any() else 0, long_indel=long_indel, kept=kept,
                   two_scans=qlen >= lim["SCAN"], unstaged=nqw > cols_qcap(lim, nw),
                   clamped=bool((isI & ((s["e"] > lim["EV_LEN"]) | (s["len"] > lim["EV_LEN_RAW"]))).any()),
                   ev_before_max=int(s["ev_before"].max()), q_total=s["q_total"], flagged_words=0, fitting_words=0, first_flagged=-1, dq_beyond=False)
        assert s["q_total"] == qlen, (rec, s["q_total"])
        if kept:
            dQ, de = directory_words(d, ops, lim, nw)
            nwin_words = (int(d["wlen"]) + 31) // 32
            fl = (de[:nwin_words] >= lim["DIR_EV"]) | (dQ[:nwin_words] >= lim["DIR_Q"])
            rec.update(flagged_words=int(fl.sum()), fitting_words=int((~fl).sum()), first_flagged=int(np.flatnonzero(fl)[0]) if fl.any() else -1,
                       dq_beyond=bool((dQ >= lim["DIR_Q"]).any()))
            wins[rec["win"]]["events"] += s["n_ev"]
        slices.append(rec)
    return slices, wins


# ---- the fp32 twin on a window of 417 792 rows -------------------------------------------------------------------------------------------------------
TOKMAP = np.full(256, 255, np.uint8)
for _i, _ch in enumerate("ACGT*acgt#."):     # inference.rs BASES_MAP
    TOKMAP[ord(_ch)] = _i


def compact_twin_inputs(wins, margin):
    """The twin's inputs for windows [(tokens [L, 31], qualities [L, 31], informative rows, ascending)], with the rows that no informative row's receptive
    field reaches cut out: the twin's dense convolutions over a batch of [windows, 417 792, 31, 64] floats are 100 GB of activations for 300 rows that matter.

    What is computed is the same function.  A logit of informative row r reads the convolution stack at r only, i.e. (two convolutions of width kw along the
    rows, margin = 2 (kw // 2)) the input rows r - margin .. r + margin of the batch array — the window's rows, behind them the collate padding (token 11,
    quality 126, inference.rs:86-97) up to the longest window of the batch, and nothing (zeros in front of each convolution) beyond either end of the array.
    So: per window the union of those stretches, clipped to the batch array and merged where they touch, laid end to end.  A stretch clipped at row 0 is
    the first and starts the compact array, one clipped at the array's end is the last and ends it (the filler that brings all windows to one length goes in
    front of the last stretch), so both still meet the end of an array where they did; everywhere else a stretch's neighbour is never read by the rows it
    was cut for.  The positional term takes the rows' numbers in the window (positions), not their new places (indices).
    Returns (bases [B, Lc, 31], quals, lens, indices_flat, positions_flat).  test_width_cases.py holds it equal to the uncut batch."""
    lmax = max(b.shape[0] for b, _, _ in wins)
    parts = []
    for b, q, rows in wins:
        rows = np.asarray(rows, np.int64)
        iv = []
        for r in rows:
            lo, hi = max(0, int(r) - margin), min(lmax, int(r) + margin + 1)
            if iv and lo <= iv[-1][1]:
                iv[-1][1] = max(iv[-1][1], hi)
            else:
                iv.append([lo, hi])
        parts.append(iv)
    lc = max([sum(hi - lo for lo, hi in iv) for iv in parts] + [1])
    B = len(wins)
    bases = np.full((B, lc, 31), 11, np.uint8)
    quals = np.full((B, lc, 31), 126, np.uint8)
    lens, idx, pos = [], [], []
    for k, ((b, q, rows), iv) in enumerate(zip(wins, parts)):
        L = b.shape[0]
        at_end = len(iv) > 0 and (len(iv) > 1 or (iv[0][1] == lmax and iv[0][0] != 0))
        assert not (len(iv) == 1 and iv[0][0] == 0 and iv[0][1] == lmax and lmax != lc), "one stretch that meets both ends of the batch array"
        place, o = {}, 0
        for n, (lo, hi) in enumerate(iv):
            if at_end and n == len(iv) - 1:
                o = lc - (hi - lo)
            n_own = max(0, min(hi, L) - lo)                 # the window's own rows; the rest of the stretch is collate padding
            bases[k, o:o + n_own] = b[lo:lo + n_own]
            quals[k, o:o + n_own] = q[lo:lo + n_own]
            place[n] = (lo, hi, o)
            o += hi - lo
        n = 0
        for r in rows:
            while not place[n][0] <= r < place[n][1]:   # (the stretches are disjoint and ascending, like the rows)
                n += 1
            idx.append(place[n][2] + int(r) - place[n][0])
            pos.append(int(r))
        lens.append(len(rows))
    return bases, quals, np.array(lens, np.int32), np.array(idx, np.int32), np.array(pos, np.int32)
