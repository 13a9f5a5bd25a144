"""Models with 1-, 9- and 13-row receptive fields, the inputs their job tests run on, and a census of what those inputs reach.

herro_job_featurize / herro_job_infer pick their code by the model's receptive field (rows within half = 2 * (kw / 2) of an informative row):
compact 16-byte records for up to 8 rows (k_rfq / k_rows), the job's own planes behind a lean featurize for more (k_layout<true> + k_tokens,
then k_quals<false>(J, half) around the informative rows only; the model front pads virtually to the batch's longest window).  The default
model (kw 3, half 2) is the only one the other job tests run.  Everything here is numpy over the oracle's windows: no device.

The census counts, per (input, batch size, batch mode, half), the informative rows and windows at which those branches can go wrong; the
not-gpu test (test_rf_cases.py) holds every class populated, so that a change to the generator cannot empty one behind the GPU tests' back."""
import functools

import numpy as np

import oracle_lib as O
from herro_amd import model_io, synth

W = 256

# name -> (hyper-parameters, rows of the receptive field, the encoder stack behind the bf16x3 front of model.hip is the f16 one)
MODELS = {
    "kw1_f16": (dict(kw=1, c1=64, c2=128, d_model=256, n_heads=8, d_ff=256, n_layers=2), 1, True),
    "kw1_generic": (dict(kw=1, d_model=128, n_heads=4, d_ff=256, n_layers=2), 1, False),
    "kw5_f16": (dict(kw=5, c1=32, c2=64, d_model=256, n_heads=8, d_ff=512, n_layers=2), 9, True),
    "kw7_f16": (dict(kw=7, c1=32, c2=32, d_model=256, n_heads=8, d_ff=256, n_layers=2), 13, True),
    "kw5_generic": (dict(kw=5, c1=32, c2=64, d_model=128, n_heads=4, d_ff=512, n_layers=2), 9, False),
}

INPUTS = {
    # 4 windows per target, the last one of 5 target positions: shorter than the 9- and 13-row fields (the seed: one of them has an informative row)
    "edges": dict(n=3, tl=3 * W + 5, ov=16, seed=synth.SEED + 1207, kw=dict(flank_min=30, flank_max=60, p_ins=0.05, p_snp=0.02, p_partial=0.3)),
    # windows above 64 informative rows (sibling tiles) next to ordinary ones, one of exactly 64; one above the 78 rows k_quals<false> expands per pass
    # for a 13-row field (RFCAP / 13).  The generator draws a SNP per target position with p_snp, so a window of 256 positions passes 64
    # informative rows only from p_snp of about 0.25 on (0.06 gives about 15: that rate passes 64 at W = 4096 only).  The seed: two windows of
    # a read within a few rows of each other's length, with informative rows at both ends — classes b - d
    "dense": dict(n=2, tl=2 * W, ov=32, seed=synth.SEED + 1368, kw=dict(flank_min=30, flank_max=60, p_snp=0.27)),
}
BATCHES = (3, 5)
MODES = (0, 1)          # 0: the reference's grouping, per read; 1: submission order in chunks
HALVES = (0, 4, 6)

TOKMAP = np.full(256, 255, np.uint8)
for _i, _ch in enumerate("ACGT*acgt#."):     # inference.rs BASES_MAP
    TOKMAP[ord(_ch)] = _i


def hyper(name):
    return model_io.Hyper(**MODELS[name][0])


def half_of(name):
    return 2 * (MODELS[name][0]["kw"] // 2)


def export_model(name, directory):
    """(path of the flat file, raw parameters, Hyper) of one model of the table, written below `directory`."""
    hp = hyper(name)
    raw = model_io.random_raw_params(hp, seed=5100 + sum(map(ord, name)))
    path = str(directory / f"{name}.hrro")
    model_io.export(raw, hp, path)
    return path, raw, hp


@functools.lru_cache(maxsize=None)
def generate(name, seed_shift=0):
    cs = INPUTS[name]
    return synth.generate(cs["n"], cs["tl"], cs["ov"], seed=cs["seed"] + seed_shift, **cs["kw"])


class Win:
    """One window of the oracle, as the model sees it: tokens / qualities u8 [L', 31] and the final rows of the informative rows."""

    def __init__(self, ow, t, wi):
        self.ow, self.t, self.wi = ow, t, wi
        self.enc = TOKMAP[ow.bases]
        self.quals = ow.quals
        self.len = self.enc.shape[0]
        self.is_target_row = self.enc[:, 0] != 4                  # the target shows '*' on an insertion row (get_target_indices, inference.rs:255-268)
        tidx = np.flatnonzero(self.is_target_row)
        self.sup_ins = ow.sup_ins.astype(np.int64)
        self.rows = (tidx[ow.sup_pos.astype(np.int64)] + self.sup_ins).astype(np.int64)
        self.n_sup = len(self.rows)


@functools.lru_cache(maxsize=None)
def windows(name, seed_shift=0):
    """(windows in job order, tgt_win_off) of an input, from the oracle; results kept alive next to them for consensus_fasta."""
    sb = generate(name, seed_shift)
    store = O.store_from_synth(sb)
    wins, off, results = [], [0], []
    for t in range(sb.n_targets):
        rid, rows, cigs = O.target_alignments(sb, t)
        res = store.extract_features(rid, rows, cigs, W)
        wins += [Win(res.window(wi), t, wi) for wi in range(len(res))]
        off.append(len(wins))
        results.append((rid, res))
    return wins, off, results


def groups(wins, tgt_win_off, batch, mode):
    """The batches herro_job_infer forms: [(members, span)] — members: the windows with informative rows that share a batch (and its padding
    length), span: every window the batch passed over.  mode 0 flushes every `batch` windows of a read and at its end, empty windows
    counted (features.rs:884-893); mode 1 takes the non-empty windows of the job in order, `batch` at a time."""
    out = []
    if mode == 0:
        for t in range(len(tgt_win_off) - 1):
            for g0 in range(tgt_win_off[t], tgt_win_off[t + 1], batch):
                span = list(range(g0, min(g0 + batch, tgt_win_off[t + 1])))
                mem = [w for w in span if wins[w].n_sup]
                if mem:
                    out.append((mem, span))
    else:
        sel = [w for w in range(len(wins)) if wins[w].n_sup]
        for g0 in range(0, len(sel), batch):
            mem = sel[g0:g0 + batch]
            out.append((mem, list(range(mem[0], mem[-1] + 1))))
    return out


def collate(members):
    """Win list -> (bases, quals [B, lmax, 31] padded with 11 / 126, lens, flat row indices): what collate hands the model (inference.rs:73-145)."""
    lmax = max(m.len for m in members)
    bases = np.full((len(members), lmax, 31), 11, np.uint8)
    quals = np.full((len(members), lmax, 31), 126, np.uint8)
    for k, m in enumerate(members):
        bases[k, :m.len] = m.enc
        quals[k, :m.len] = m.quals
    lens = np.array([m.n_sup for m in members], np.int32)
    flat = np.concatenate([m.rows for m in members]).astype(np.int32)
    return bases, quals, lens, flat


CLASSES = "abcdefghi"


def census(name, batch, mode, half):
    """Counts of the informative rows of kinds (a)-(f) and of the windows of kinds (g)-(i) of the module docstring's branches:
    a  the field starts above the window (r0 - half < 0)
    b  the field ends below the LONGEST window of its batch: the convolution's zero padding
    c  the field ends below a shorter window, inside [len, lmax): pad cells only
    d  ... and reaches past lmax: pad cells, then zeros
    e  the informative row is an insertion row
    f  the field holds an insertion row with target rows on both sides of it
    g  a window (with informative rows) shorter than the field
    h  a window without informative rows inside a batch that has some
    i  a window above 64 informative rows"""
    wins, off, _ = windows(name)
    n = dict.fromkeys(CLASSES, 0)
    for mem, span in groups(wins, off, batch, mode):
        lmax = max(wins[w].len for w in mem)
        n["h"] += sum(1 for w in span if wins[w].n_sup == 0)
        for w in mem:
            m = wins[w]
            n["g"] += m.len < 2 * half + 1
            n["i"] += m.n_sup > 64
            for r0, ins in zip(m.rows, m.sup_ins):
                lo, hi = int(r0) - half, int(r0) + half
                n["a"] += lo < 0
                if hi >= m.len:
                    if m.len == lmax:
                        n["b"] += 1
                    elif hi < lmax:
                        n["c"] += 1
                    else:
                        n["d"] += 1
                n["e"] += ins > 0
                t = m.is_target_row[max(lo, 0):min(hi, m.len - 1) + 1]
                tr = np.flatnonzero(t)
                n["f"] += len(tr) >= 2 and not t[tr[0]:tr[-1] + 1].all()
    return {k: int(v) for k, v in n.items()}


def census_union(half):
    tot = dict.fromkeys(CLASSES, 0)
    for name in INPUTS:
        for batch in BATCHES:
            for mode in MODES:
                for k, v in census(name, batch, mode, half).items():
                    tot[k] += int(v)
    return tot
