"""The PAF line format of herro_aligned_dev_paf / herro_pairs_paf / herro_pairs_write_alns (include/herro_amd.h) restated in plain
Python: the text every writer test is held to.

One line per row whose record has ops, fields separated by tabs, closed by a newline:
    qname qlen qstart qend +|- tname tlen tstart tend mbases blocklen 255 cg:Z:<cigar>
the nine coordinate fields as decimal numbers, mbases the summed lengths of the record's type-0 ops, blocklen those of all its ops (Python
integers: no width), <cigar> the ops as "<len><M|I|D|?>" (type 3 prints '?')."""

LETTER = "MID?"


def cigar(ops) -> str:
    return "".join(f"{int(x) >> 2}{LETTER[int(x) & 3]}" for x in ops)


def line(row, ops, names) -> bytes:
    """row: the nine fields qid qlen qstart qend strand tid tlen tstart tend; ops: the record's `len << 2 | type`; no ops: no line"""
    if len(ops) == 0:
        return b""
    qid, qlen, qstart, qend, strand, tid, tlen, tstart, tend = (int(v) for v in row[:9])
    mbases = sum(int(x) >> 2 for x in ops if int(x) & 3 == 0)
    blocklen = sum(int(x) >> 2 for x in ops)
    head = b"\t".join([names[qid], b"%d" % qlen, b"%d" % qstart, b"%d" % qend, b"-" if strand else b"+",
                       names[tid], b"%d" % tlen, b"%d" % tstart, b"%d" % tend, b"%d" % mbases, b"%d" % blocklen, b"255"])
    return head + b"\tcg:Z:" + cigar(ops).encode() + b"\n"


def paf(rows, n_ops, op_off, ops, names, rec=None) -> bytes:
    """the text of records rec (None: all, in order) of a handle: rows [n, >= 9], n_ops [n], op_off [n] (each record's first op), ops"""
    order = range(len(rows)) if rec is None else [int(r) for r in rec]
    return b"".join(line(rows[r], ops[int(op_off[r]):int(op_off[r]) + int(n_ops[r])], names) for r in order)


def paf_cigars(rows, cigars, names, rec=None) -> bytes:
    """paf() over CIGAR texts instead of ops (the records a device aligned: AlignedDev.rows and AlignedDev.cigar)"""
    import re
    ty = {"M": 0, "I": 1, "D": 2, "?": 3}
    order = range(len(rows)) if rec is None else [int(r) for r in rec]
    out = []
    for r in order:
        got = re.findall(rb"(\d+)([MID?])", cigars[r])
        assert b"".join(n + t for n, t in got) == cigars[r]
        out.append(line(rows[r], [(int(n) << 2) | ty[t.decode()] for n, t in got], names))
    return b"".join(out)
