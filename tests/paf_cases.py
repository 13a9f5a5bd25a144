"""The hand-made handles of the PAF writer's tests (tests/test_paf_write_host.py on a HostContext, tests/test_gpu_paf_write.py on a device),
all built through aligned_dev_from_ops, which takes rows and ops as given — the ops need not match the coordinates.  Six reads.

digits   every decimal width of an op length, 1 .. 10 digits, at both edges of each (1, 9, 10, 99, ... 999 999 999, 10^9, 2^30 - 1), one
         record per op type (3 prints '?') and one that cycles the types
blocks   records of 1, 2, 63, 64, 65, 127, 128, 129 and 4097 ops of mixed widths: k_paf_write takes 64 ops per step and carries the bytes
         written so far into the next one, so a wrong carry shifts every later byte
failed   records without ops as the first, a middle and the last row
none     every record failed: an empty text
coords   all nine coordinate fields at ten digits, both strands
sums     five M ops of 2^30 - 1 and more: mbases and blocklen above 2^32"""
import importlib.util
import os

import numpy as np

# tests/paf_ref.py by its path and under a name of its own: oracle/paf_ref.py (the parser's oracle) is a module `paf_ref` too, and which of the two
# an `import paf_ref` finds depends on the order of sys.path
_spec = importlib.util.spec_from_file_location("paf_write_ref", os.path.join(os.path.dirname(os.path.abspath(__file__)), "paf_ref.py"))
REF = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(REF)

N_READS = 6
NAMES = [b"r", b"n" * 300, b"twin", b"twin", b"a name with spaces", b"read/5 x=1"]     # one byte, 300 bytes, two equal names, spaces
UNIQUE = [b"read%d" % i for i in range(N_READS)]                                       # for the parser: it maps a name to one id
BAD_NAMES = {"empty": (2, b""), "tab": (4, b"a\tb"), "newline": (5, b"ab\n")}          # read, name: HERRO_E_INVALID naming the read
HOST_READ_LEN = np.full(N_READS, 4294967295, np.uint32)
U32 = 4294967295

EDGE_LENS = [1, 9]
for _k in range(1, 10):
    EDGE_LENS += [10 ** _k, 10 ** (_k + 1) - 1 if _k < 9 else (1 << 30) - 1]
assert EDGE_LENS[-2:] == [10 ** 9, (1 << 30) - 1] and 999999999 in EDGE_LENS and len(EDGE_LENS) == 20


def _op(ln, ty):
    return (ln << 2) | ty


def _mixed(n, salt=0):
    """n ops whose lengths run through 1 .. 7 digits and whose types through M, I, D"""
    return [_op(10 ** ((i + salt) % 7) + (i * 7 + salt) % 9, (i + salt) % 3) for i in range(n)]


def _row(i, strand=None):
    q, t = i % N_READS, (i + 1 + i // N_READS) % N_READS
    return [q, 5000 + i, 10 + i, 4000 + i, (i & 1) if strand is None else strand, t, 6000 + i, 20 + i, 4500 + i]


def handles():
    """name -> (rows u32 [n, 9], [the ops of every record])"""
    h = {}
    h["digits"] = [[_op(ln, ty) for ln in EDGE_LENS] for ty in range(4)] + [[_op(ln, i % 4) for i, ln in enumerate(EDGE_LENS)]]
    h["blocks"] = [_mixed(n, salt=n) for n in (1, 2, 63, 64, 65, 127, 128, 129, 4097)]
    h["failed"] = [[], _mixed(3), _mixed(70, 1), [], _mixed(5, 2), []]
    h["none"] = [[], [], []]
    h["sums"] = [[_op((1 << 30) - 1, 0)] * 3 + [_op(7, 1), _op((1 << 30) - 1, 2), _op((1 << 30) - 1, 0), _op((1 << 30) - 1, 0), _op((1 << 30) - 1, 2)],
                 [_op((1 << 30) - 1, 2)] * 5 + [_op(1, 0)]]
    out = {k: (np.array([_row(i) for i in range(len(v))], np.uint32), v) for k, v in h.items()}
    out["coords"] = (np.array([[0, U32, U32 - 1, U32, 0, 1, U32, 4000000000, U32],
                               [5, 4000000000, 1000000000, 3999999999, 1, 4, U32, 0, 1000000000]], np.uint32), [_mixed(4), _mixed(66, 3)])
    return out


def long_handle():
    """600 KB of text in lines of ~20 KB and one of ~100 KB: several chunks at HERRO_PAF_SCRATCH_MB=1 (chunks of 64 KiB), the long line alone in its"""
    per = [_mixed(4097, salt=i) for i in range(12)] + [_mixed(20000, 5)] + [_mixed(4097, salt=i) for i in range(12, 30)]
    return np.array([_row(i) for i in range(len(per))], np.uint32), per


def arrays(ops_per_record):
    """(op_off u64 [n + 1], ops u32) as aligned_dev_from_ops takes them"""
    off = np.zeros(len(ops_per_record) + 1, np.uint64)
    off[1:] = np.cumsum([len(o) for o in ops_per_record])
    flat = [x for o in ops_per_record for x in o]
    return off, np.array(flat, np.uint32) if flat else np.zeros(0, np.uint32)


def build(c, case):
    rows, per = case
    off, ops = arrays(per)
    return c.aligned_dev_from_ops(rows, off, ops)


def want(case, names, rec=None):
    rows, per = case
    off, ops = arrays(per)
    return REF.paf(rows, [len(o) for o in per], off, ops, names, rec)


def selections(n):
    """rec arguments over n records: all, a permutation, repeats, none"""
    return [None, list(range(n))[::-1], [0, n - 1, 0, 0, n // 2, n - 1], []]


def pair_table():
    """A hand-made pair handle over the six reads (read_len >= 5000 each): three primaries (t < q), the table of their six rows by (tid, qid), and
    the 2 P records (primaries, then their swaps) with made-up ops; records 1 (a primary) and 5 (a mirror) failed.
    -> dict(primaries, rids, aln_off, rec_of_row, rows2, ops2)"""
    prim = np.array([[1, 4000, 100, 3000, 0, 0, 4500, 200, 3100],
                     [3, 4200, 50, 2050, 1, 0, 4500, 1000, 3000],
                     [5, 3900, 0, 3900, 0, 2, 4100, 100, 4000]], np.uint32)
    swap = prim[:, [5, 6, 7, 8, 4, 0, 1, 2, 3]]
    rows2 = np.concatenate([prim, swap])
    key = rows2[:, 5].astype(np.int64) << 32 | rows2[:, 0]
    rec_of_row = np.argsort(key).astype(np.uint32)
    tids = rows2[rec_of_row, 5]
    rids = np.unique(tids).astype(np.uint32)
    aln_off = np.concatenate([[0], np.cumsum([(tids == t).sum() for t in rids])]).astype(np.uint64)
    ops2 = [_mixed(130, 1), [], _mixed(3, 2), _mixed(64, 3), _mixed(7, 4), []]
    return dict(primaries=prim, rids=rids, aln_off=aln_off, rec_of_row=rec_of_row, rows2=rows2, ops2=ops2)
