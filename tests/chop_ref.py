"""The specification of Job.fasta_dev / herro_job_fasta_dev as a pure function of FASTA bytes: it takes the text
herro_job_fasta returns and gives the text the device call must return, so the host path is the oracle of the device path.  Plain Python
over integers and bytes; nothing here knows the library.

It restates scripts/postprocess_corrected.sh of the reference's workflow in two numbers: `seqkit sliding -s C -W C -g` (pieces of C bases,
the last one of a record shorter, named <name>_sliding:<start>-<end> with 1-based inclusive coordinates) and `seqkit seq -m M` (pieces
below M bases dropped); C = 30000 and M = 10000 there.

  record in    '>' name ' ' [desc] '\\n' bases '\\n'         (herro_job_fasta: name is id, or id:i when the target has several segments)
  pieces       C == 0: [0, n) without suffix; C > 0: k = 0 .. ceil(n / C) - 1 -> [kC, min((k + 1)C, n)), suffix _sliding:<kC + 1>-<end>
  kept         end - start >= M
  record out   '>' name suffix ' ' [desc] '\\n' body '\\n', a '\\n' behind every L bases of the body except at its end (L == 0: one line)
"""
import collections

Stats = collections.namedtuple("Stats", "records bases pieces_dropped bases_dropped segments targets")


def pieces(n: int, chop_len: int):
    """every piece [start, end) of a sequence of n bases, before the filter"""
    if chop_len == 0:
        return [(0, n)]
    return [(k * chop_len, min((k + 1) * chop_len, n)) for k in range(-(-n // chop_len))]


def kept_pieces(n: int, chop_len: int, min_length: int):
    return [(a, b) for a, b in pieces(n, chop_len) if b - a >= min_length]


def parse(text: bytes):
    """[(name, desc, bases)] of herro_job_fasta's text: two lines per record, the name ends at the first space"""
    lines = text.split(b"\n")
    assert lines[-1] == b"" and len(lines) % 2 == 1, "the text ends with a newline and has two lines per record"
    out = []
    for h, s in zip(lines[0:-1:2], lines[1:-1:2]):
        assert h[:1] == b">" and b" " in h, h[:40]
        name, desc = h[1:].split(b" ", 1)
        out.append((name, desc, s))
    return out


def wrap(seq: bytes, line_width: int) -> bytes:
    if line_width == 0 or len(seq) <= line_width:
        return seq
    return b"\n".join(seq[i:i + line_width] for i in range(0, len(seq), line_width))


def chop(text: bytes, chop_len: int = 0, min_length: int = 0, line_width: int = 0, ends=None):
    """(text out, Stats, target_end out).  ends: herro_job_fasta's rec_end (the offset behind every target's records in `text`); None: the
    text is taken as one target's."""
    ends = [len(text)] if ends is None else [int(e) for e in ends]
    assert all(a <= b for a, b in zip(ends, ends[1:])) and (not ends or ends[-1] == len(text))
    out, out_ends = [], []
    at = n_out = 0
    records = bases = dropped = bases_dropped = segments = targets = 0
    for e in ends:
        had = records
        for name, desc, seq in parse(text[at:e]):
            segments += 1
            for a, b in pieces(len(seq), chop_len):
                if b - a < min_length:
                    dropped += 1
                    bases_dropped += b - a
                    continue
                suffix = b"_sliding:%d-%d" % (a + 1, b) if chop_len else b""
                rec = b">" + name + suffix + b" " + desc + b"\n" + wrap(seq[a:b], line_width) + b"\n"
                out.append(rec)
                n_out += len(rec)
                records += 1
                bases += b - a
        targets += records > had
        out_ends.append(n_out)
        at = e
    return b"".join(out), Stats(records, bases, dropped, bases_dropped, segments, targets), out_ends


def piece_table(lengths, chop_len: int, min_length: int):
    """herro_chop_plan's result over sequence lengths: ([(seq, start, end)], piece_off, (kept, dropped, bases kept, bases dropped))"""
    rows, off = [], [0]
    kept = dropped = bk = bd = 0
    for s, n in enumerate(lengths):
        for a, b in pieces(int(n), chop_len):
            if b - a >= min_length:
                rows.append((s, a, b)); kept += 1; bk += b - a
            else:
                dropped += 1; bd += b - a
        off.append(len(rows))
    return rows, off, (kept, dropped, bk, bd)
