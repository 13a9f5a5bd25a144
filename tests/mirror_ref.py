"""numpy restatement of herro_aligned_dev_mirror (k_mirror in csrc/align_dev.hip; DESIGN.md §9, "Mirrored records"): the alignment of
(q, t) derived from the final ops of (t, q) instead of a second sweep.  The kernel is held to this file bit for bit.

Row' swaps query and target (same strand); ops' swap I and D and are reversed on strand 1; T' / Q' are record_seqs(row'); then the
steps of §9 unchanged — fix_cigar(ops', T', Q'), one trailing indel dropped, the coordinates moved with what was dropped, failed when
the result is empty or does not start and end with M.  A failed source and a source with an op of type 3 mirror to a failed record:
no ops, score INT32_MIN, the swapped coordinates untrimmed.  Score' = score + g(ops) - g(final ops'), g the sum of 4 + 2 len over the
I and D ops.  Everything about sequences, fix_cigar and scores comes from tests/align_ref.py."""
from __future__ import annotations

import numpy as np

from align_ref import D_, GAP_EXT, GAP_OPEN, I_, INT32_MIN, M_, cigar_text, fix_cigar, parse_cigar, record_seqs, score_cigar  # noqa: F401

SWAP = [5, 6, 7, 8, 4, 0, 1, 2, 3]     # row' = row[SWAP]


def swap_row(row) -> np.ndarray:
    """(qid, qlen, qstart, qend, strand, tid, tlen, tstart, tend) -> (tid, tlen, tstart, tend, strand, qid, qlen, qstart, qend)"""
    return np.asarray(row)[:9][SWAP].astype(np.uint32)


def mirror_ops(ops, strand: int):
    """ops' before the normalisation: I <-> D, reversed iff strand == 1 (types other than M / I / D are left alone)"""
    out = [(int(ln), {I_: D_, D_: I_}.get(int(t), int(t))) for ln, t in ops]
    return out[::-1] if strand else out


def gap_cost(ops) -> int:
    return sum(GAP_OPEN + GAP_EXT * int(ln) for ln, t in ops if t != M_)


def mirror_record(read_codes, row, ops, score: int):
    """One record: row (its final, trimmed coordinates), ops [(len, type)] (empty: a failed source), score.
    Returns (row' u32 [9], ops' [(len, type)], score', ok)."""
    out = swap_row(row)
    if not ops or any(t not in (M_, I_, D_) for _, t in ops):
        return out, [], INT32_MIN, False
    T, Q = record_seqs(read_codes, out)
    cig, tsh0, qsh0 = fix_cigar(mirror_ops(ops, int(out[4])), T, Q)
    tsh1 = qsh1 = 0
    if cig and cig[-1][1] != M_:
        if cig[-1][1] == I_:
            qsh1 = cig[-1][0]
        else:
            tsh1 = cig[-1][0]
        cig = cig[:-1]
    if not cig or cig[0][1] != M_ or cig[-1][1] != M_:
        return out, [], INT32_MIN, False
    out[7] += tsh0
    out[8] -= tsh1
    if out[4] == 0:
        out[2] += qsh0
        out[3] -= qsh1
    else:
        out[3] -= qsh0
        out[2] += qsh1
    return out, cig, int(score) + gap_cost(ops) - gap_cost(cig), True


def mirror_records(read_codes, rows, cigars, scores):
    """mirror_record over a handle's records: rows u32 [n, >= 9], cigars list of CIGAR text (b"": failed), scores [n].
    Returns (rows' u32 [n, 10] with column 9 zero, cigars' list of bytes, scores' i64 [n], ok bool [n]) — records n .. 2n - 1 of the
    mirrored handle."""
    n = len(rows)
    rows_out = np.zeros((n, 10), np.uint32)
    cig_out, sc_out, ok = [], np.full(n, INT32_MIN, np.int64), np.zeros(n, bool)
    for r in range(n):
        row, cig, sc, good = mirror_record(read_codes, rows[r], parse_cigar(cigars[r]), int(scores[r]))
        rows_out[r, :9] = row
        cig_out.append(cigar_text(cig))
        sc_out[r], ok[r] = sc, good
    return rows_out, cig_out, sc_out, ok
