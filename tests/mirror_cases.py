"""Cases shared by tests/test_mirror_host.py and tests/test_gpu_mirror.py (herro_aligned_dev_mirror; DESIGN.md §9, "Mirrored records").

Every hand case is written in the MIRROR's terms — its target T', its oriented query Q', its ops before the normalisation and the CIGAR
that must come out — and the source record is derived from it: the source's query read is T' as stored, its target read is Q' (reversed
and complemented on strand 1), its ops are the mirror's with I and D exchanged, reversed on strand 1 (the transformation is its own
inverse).  The expected CIGARs were worked out by hand from fix_cigar's rules, not taken from tests/mirror_ref.py."""
import numpy as np

COMP = bytes.maketrans(b"ACGT", b"TGCA")
M, I, D = 0, 1, 2
_TY = {"M": M, "I": I, "D": D}


def rc(s: bytes) -> bytes:
    return s.translate(COMP)[::-1]


def ops_of(text: str):
    """'8M2I6M' -> [(8, 0), (2, 1), (6, 0)]"""
    out, num = [], 0
    for ch in text:
        if ch.isdigit():
            num = num * 10 + int(ch)
        else:
            out.append((num, _TY[ch]))
            num = 0
    return out


def unmirror(ops, strand):
    out = [(ln, {I: D, D: I}.get(t, t)) for ln, t in ops]
    return out[::-1] if strand else out


# name: (strand, T', Q', the mirror's ops before fix_cigar, the final CIGAR or None for a failed record,
#        {column of row': what the trim adds to it}); ops as text, or as a list where a type has no letter
HAND = {
    # exchanged and nothing else: no indel sits in a repeat
    "swap_strand0": (0, b"GATTACAGTGAAGTACATG", b"GATTACAGCCTGAAGTCATG", "8M2I6M1D4M", "8M2I6M1D4M", {}),
    "reverse_strand1": (1, b"CATGTACTTCACTGTAATC", b"CATGACTTCAGGCTGTAATC", "4M1D6M2I8M", "4M1D6M2I8M", {}),
    # strand 1: the source's left-most indels arrive right-most — the deleted A is the last of six, the inserted T the last of six
    "homopolymer_strand1": (1, b"GCTGAAAAAAGCCGTTTTTCAGC", b"GCTGAAAAAGCCGTTTTTTCAGC", "9M1D9M1I4M", "4M1D9M1I9M", {}),
    # ... and the last unit of (TAG)3 / of (CGT)4: six and nine bases to the left
    "repeat3_strand1": (1, b"TGCCTAGTAGTAGCCAACGTCGTCGTGATC", b"TGCCTAGTAGCCAACGTCGTCGTCGTGATC", "10M3D13M3I4M", "4M3D10M3I13M", {}),
    # the 2D moves three bases through TATAT and uses up the 3M in front of it: 5M 1D 0M 2D 9M -> 5M 3D 9M
    "shift_eats_the_m": (0, b"ACGTGCTATATGGCTCA", b"ACGTGTATGGCTCA", "5M1D3M2D6M", "5M3D9M", {}),
    # the indel moves to the front of the record (ATATA), where it is dropped: the coordinates move
    "uncovers_leading_d_strand0": (0, b"ATATAGGCTCAGT", b"ATAGGCTCAGT", "3M2D8M", "11M", {7: 2}),
    "uncovers_leading_d_strand1": (1, b"ATATAGGCTCAGT", b"ATAGGCTCAGT", "3M2D8M", "11M", {7: 2}),
    "uncovers_leading_i_strand0": (0, b"ATAGGCTCAGT", b"ATATAGGCTCAGT", "3M2I8M", "11M", {2: 2}),
    "uncovers_leading_i_strand1": (1, b"ATAGGCTCAGT", b"ATATAGGCTCAGT", "3M2I8M", "11M", {3: -2}),
    # the trailing D is dropped and an I is left at the end
    "ends_i_next_to_d": (0, b"ACGTGCAT", b"ACGTGTT", "5M2I3D", None, {}),
    "failed_source": (0, b"ACGTGCAT", b"ACGTGTT", "", None, {}),
    "type_3": (1, b"ACGTTGCAAGC", b"ACGTTGCAAGC", [(5, M), (1, 3), (5, M)], None, {}),
    "single_m": (1, b"ACGTTGCAAGCT", b"ACGTTGCAAGCT", "12M", "12M", {}),
    # two and three ops: an indel at j = 0 or j = c - 1 is never moved, only dropped
    "two_ops_trailing": (0, b"ACGTGCA", b"ACGTG", "5M2D", "5M", {8: -2}),
    "two_ops_leading_strand1": (1, b"CAACGTG", b"ACGTG", "2D5M", "5M", {7: 2}),
    "three_ops_both_ends": (0, b"GGACGT", b"ACGTCCC", "2D4M3I", "4M", {7: 2, 3: -3}),
    "three_ops_both_ends_strand1": (1, b"GGACGT", b"ACGTCCC", "2D4M3I", "4M", {7: 2, 2: 3}),
    "three_ops_middle_moves": (1, b"ACGGTCAT", b"ACGGGTCAT", "4M1I4M", "2M1I6M", {}),
}


def build(cases):
    """[(strand, T', Q', mirror ops [(len, type)])] -> (reads [ASCII], rows u32 [n, 9] of the SOURCE records over their whole reads,
    op_off u64 [n + 1], ops u32): record i has target read 2i and query read 2i + 1"""
    reads, rows, ops, off = [], [], [], [0]
    for strand, tp, qp, mops in cases:
        t = rc(qp) if strand else qp           # Q' = the source's target, reversed and complemented on strand 1
        q = tp                                 # T' = the source's query as stored
        rows.append([len(reads) + 1, len(q), 0, len(q), strand, len(reads), len(t), 0, len(t)])
        reads += [t, q]
        src = unmirror(mops, strand)
        ops += [(ln << 2) | ty for ln, ty in src]
        off.append(len(ops))
    return reads, np.array(rows, np.uint32).reshape(-1, 9), np.array(off, np.uint64), np.array(ops, np.uint32)


def hand():
    """(names, reads, rows, op_off, ops, want): want[i] = (row' u32 [9], CIGAR text or None)"""
    names = list(HAND)
    cases = [(s, tp, qp, ops_of(o) if isinstance(o, str) else o) for s, tp, qp, o, _, _ in HAND.values()]
    reads, rows, off, ops = build(cases)
    want = []
    for i, (_, _, _, _, text, delta) in enumerate(HAND.values()):
        row = rows[i][[5, 6, 7, 8, 4, 0, 1, 2, 3]].astype(np.int64)
        for col, d in delta.items():
            row[col] += d
        want.append((row.astype(np.uint32), None if text is None else text.encode()))
    return names, reads, rows, off, ops, want


def alternating(n):
    """n >= 1 ops that start and end with M and never repeat a type (M D M I ...; an even n holds one 'D I'): one-base gaps, M of 2-5"""
    ty = [M if i % 2 == 0 else (D, I)[(i // 2) % 2] for i in range(n if n % 2 else n - 1)]
    if n % 2 == 0:
        ty.insert(2, I)
    assert len(ty) == n and ty[0] == ty[-1] == M and all(a != b for a, b in zip(ty, ty[1:]))
    return [(2 + (i * 7) % 4 if t == M else 1, t) for i, t in enumerate(ty)]


def counted(rng, counts=(1, 2, 3, 63, 64, 65, 201), alphabet=2):
    """mirror-space cases with `counts` ops on both strands over a two-letter alphabet, so that most one-base gaps sit in a repeat and
    move: M copies the target, an insertion is random"""
    out = []
    for n in counts:
        for strand in (0, 1):
            mops = alternating(n) if n != 2 else [(6, M), (1, D)] if strand else [(1, I), (6, M)]
            tp, qp = bytearray(), bytearray()
            for ln, ty in mops:
                seg = bytes(b"ACGT"[x] for x in rng.integers(0, alphabet, ln))
                if ty == M:
                    tp += seg; qp += seg
                elif ty == D:
                    tp += seg
                else:
                    qp += seg
            out.append((strand, bytes(tp), bytes(qp), mops))
    return out


def store(reads):
    """Context.set_reads' three arrays"""
    seq = np.frombuffer(b"".join(reads), np.uint8).copy()
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    return seq, np.full(len(seq), 40 + 33, np.uint8), off


def handle_ops(h, r0=0, r1=None):
    """the CIGAR texts of a handle's records [r0, r1)"""
    return [h.cigar(r) for r in range(r0, h.n if r1 is None else r1)]
