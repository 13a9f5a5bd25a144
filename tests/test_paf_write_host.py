"""not-gpu: the PAF / .oec.zst writer on a device-free context (herro_aligned_dev_paf, herro_pairs_paf, herro_pairs_write_alns).
A HostContext's handle goes through the host formatter, which is the specification the kernels are held to (tests/test_gpu_paf_write.py):
here it is held to tests/paf_ref.py byte for byte, to AlignedDev.cigar, and to the library's own parser.  Every error code of the entries is
covered but two causes of HERRO_E_UNSUPPORTED, which need inputs no test can hold: more than 2^31 - 1 rows, and a line of 2^32 bytes or more."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import paf_cases as K  # noqa: E402
from herro_amd import api  # noqa: E402

HANDLES = K.handles()


@pytest.fixture(scope="module")
def ctx():
    c = api.HostContext(K.HOST_READ_LEN)
    yield c
    c.close()


def _pairs(c):
    t = K.pair_table()
    p = c.pairs_from_table(t["primaries"], None, t["rids"], t["aln_off"], t["rec_of_row"])
    m = K.build(c, (t["rows2"], t["ops2"]))
    return t, p, m


def _raises(code, text, fn, *args, **kw):
    with pytest.raises(api.HerroError) as e:
        fn(*args, **kw)
    assert e.value.code == code and text in str(e.value), str(e.value)


# ---- 1. the text ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(HANDLES))
def test_every_case_equals_the_reference_restatement(ctx, name):
    case = HANDLES[name]
    h = K.build(ctx, case)
    for names in (K.NAMES, K.UNIQUE):
        for rec in K.selections(h.n):
            got = h.paf(names, rec)
            assert got == K.want(case, names, rec), (name, rec)
            assert got.count(b"\n") == sum(len(case[1][r]) > 0 for r in (range(h.n) if rec is None else rec))
    if name == "none":
        assert h.paf(K.NAMES) == b"" and h.failed == h.n
    if name == "sums":
        f = h.paf(K.NAMES).split(b"\n")[0].split(b"\t")
        assert int(f[9]) == 5 * ((1 << 30) - 1) > 1 << 32 and int(f[10]) == 7 * ((1 << 30) - 1) + 7
    if name == "coords":
        assert h.paf(K.UNIQUE).split(b"\n")[0].split(b"\t")[1:4] == [b"4294967295", b"4294967294", b"4294967295"]
    h.close()


@pytest.mark.parametrize("name", sorted(HANDLES))
def test_every_line_carries_the_cigar_of_its_record(ctx, name):
    h = K.build(ctx, HANDLES[name])
    lines = h.paf(K.NAMES).split(b"\n")[:-1]
    kept = [r for r in range(h.n) if h.ok[r]]
    assert len(lines) == len(kept)
    for ln, r in zip(lines, kept):
        f = ln.split(b"\t")
        assert len(f) == 13 and f[11] == b"255" and f[12] == b"cg:Z:" + h.cigar(r), (name, r)
    if name == "digits":
        assert b"?" in lines[3] and lines[3].count(b"?") == len(K.EDGE_LENS)
    h.close()


@pytest.mark.parametrize("name", sorted(HANDLES))
def test_the_parser_reads_the_text_back(ctx, name):
    rows, per = HANDLES[name]
    h = K.build(ctx, HANDLES[name])
    paf = api.Paf(K.UNIQUE, text=h.paf(K.UNIQUE))
    kept = [r for r in range(h.n) if per[r]]
    targets = list(dict.fromkeys(int(rows[r, 5]) for r in kept))            # first appearance
    assert paf.targets.tolist() == targets
    want = [tuple(int(v) for v in rows[r, :9]) + (K.REF.cigar(per[r]).encode(),) for t in targets for r in kept if rows[r, 5] == t]
    assert paf.rows() == want, name
    paf.close()
    h.close()


# ---- 2. pairs ---------------------------------------------------------------------------------------------------------------------------------
def test_pairs_paf_follows_the_table_and_drops_failed_rows(ctx):
    t, p, m = _pairs(ctx)
    assert m.ok.tolist() == [True, False, True, True, True, False]
    got = p.paf(m, K.UNIQUE)
    assert got == K.want((t["rows2"], t["ops2"]), K.UNIQUE, t["rec_of_row"])
    _, off2, rec = api.paired_job_args(p.rids, p.aln_off, p.rec_of_row, m.ok)       # what herro_job_create_paired keeps
    assert got == m.paf(K.UNIQUE, rec) and got.count(b"\n") == len(rec) == 4
    paf = api.Paf(K.UNIQUE, text=got)
    keep_t = np.diff(off2.astype(np.int64)) > 0
    assert paf.targets.tolist() == p.rids[keep_t].tolist()
    assert np.array_equal(paf.coords()[:, :9], t["rows2"][rec])
    for x in (paf, p, m):
        x.close()


def test_write_alns_plain_and_oec(ctx, tmp_path):
    t, p, m = _pairs(ctx)
    text = p.paf(m, K.UNIQUE)
    plain = str(tmp_path / "batch.paf")
    assert p.write_alns(m, K.UNIQUE, plain) == (4, len(text))
    assert open(plain, "rb").read() == text
    oec = str(tmp_path / "0.oec.zst")
    zstd_there = True
    try:
        C.CDLL("libzstd.so.1")
    except OSError:
        zstd_there = False
    if not zstd_there:
        _raises(-4, "libzstd.so.1 not available", p.write_alns, m, K.UNIQUE, oec)
        assert os.listdir(tmp_path) == ["batch.paf"]
        return
    lines, size = p.write_alns(m, K.UNIQUE, oec)
    assert lines == 4 and size == os.path.getsize(oec) and open(oec, "rb").read(4) == b"\x28\xb5\x2f\xfd"       # one zstd frame
    want = api.Paf(K.UNIQUE, text=text)
    got = api.Paf(K.UNIQUE, path=oec)
    assert got.targets.tolist() == want.targets.tolist() and got.aln_off.tolist() == want.aln_off.tolist() and got.rows() == want.rows()
    # (the rows above went through the library's reader, which skips the header by its count: a wrong count would have cost rows or raised.)
    # The header's own bytes, which that reader throws away: the same libzstd.so.1, one whole frame
    head = b"%d\n" % len(p.rids) + b"".join(K.UNIQUE[r] + b"\n" for r in p.rids)
    z = C.CDLL("libzstd.so.1")
    z.ZSTD_decompress.restype = z.ZSTD_findFrameCompressedSize.restype = C.c_size_t
    raw = open(oec, "rb").read()
    assert z.ZSTD_findFrameCompressedSize(raw, C.c_size_t(len(raw))) == len(raw)                # ONE frame
    buf = C.create_string_buffer(len(head) + len(text) + 64)
    n = z.ZSTD_decompress(buf, C.c_size_t(len(buf)), raw, C.c_size_t(len(raw)))
    assert not z.ZSTD_isError(C.c_size_t(n)) and buf.raw[:n] == head + text
    # explicit flags override the suffix
    assert p.write_alns(m, K.UNIQUE, str(tmp_path / "x.oec.zst"), oec=False) == (4, len(text))
    assert open(tmp_path / "x.oec.zst", "rb").read() == text
    assert sorted(os.listdir(tmp_path)) == ["0.oec.zst", "batch.paf", "x.oec.zst"]              # no .tmp left behind
    for x in (want, got, p, m):
        x.close()


def test_an_empty_table_writes_a_header_only(ctx, tmp_path):
    p = ctx.pairs_from_table(np.zeros((0, 9), np.uint32), None, np.zeros(0, np.uint32), np.zeros(1, np.uint64), np.zeros(0, np.uint32))
    m = ctx.aligned_dev_from_ops(np.zeros((0, 9), np.uint32), np.zeros(1, np.uint64), np.zeros(0, np.uint32))
    assert p.paf(m, K.UNIQUE) == b"" and m.paf(K.UNIQUE) == b""
    assert p.write_alns(m, K.UNIQUE, str(tmp_path / "e.paf")) == (0, 0) and os.path.getsize(tmp_path / "e.paf") == 0
    lines, size = p.write_alns(m, K.UNIQUE, str(tmp_path / "e.oec.zst"))
    assert lines == 0 and size > 0
    got = api.Paf(K.UNIQUE, path=str(tmp_path / "e.oec.zst"))
    assert got.n_alns == 0 and len(got.targets) == 0
    for x in (got, p, m):
        x.close()


# ---- 3. errors --------------------------------------------------------------------------------------------------------------------------------
def test_errors(ctx, tmp_path):
    t, p, m = _pairs(ctx)
    L = ctx._l
    blob, off = api._name_blob(ctx, K.UNIQUE)
    h, n64 = C.c_void_p(), C.c_uint64()
    path = str(tmp_path / "never.oec.zst")
    # null arguments
    assert L.herro_aligned_dev_paf(None, m.h, 0, None, blob, off.ctypes.data, C.byref(h)) == -1
    assert L.herro_aligned_dev_paf(ctx.h, None, 0, None, blob, off.ctypes.data, C.byref(h)) == -1
    assert L.herro_aligned_dev_paf(ctx.h, m.h, 0, None, None, off.ctypes.data, C.byref(h)) == -1
    assert L.herro_aligned_dev_paf(ctx.h, m.h, 0, None, blob, None, C.byref(h)) == -1
    assert L.herro_aligned_dev_paf(ctx.h, m.h, 0, None, blob, off.ctypes.data, None) == -1
    assert L.herro_pairs_paf(ctx.h, None, m.h, blob, off.ctypes.data, C.byref(h)) == -1
    assert L.herro_pairs_paf(ctx.h, p.h, None, blob, off.ctypes.data, C.byref(h)) == -1
    assert L.herro_pairs_write_alns(ctx.h, p.h, m.h, blob, off.ctypes.data, None, 0, C.byref(n64), C.byref(n64)) == -1
    assert not h.value
    # a bad name, named, before anything else (here: before the out-of-range row)
    for why, (r, bad) in K.BAD_NAMES.items():
        names = list(K.UNIQUE)
        names[r] = bad
        text = f"read {r}: " + ("empty name" if why == "empty" else "a name must not contain a tab or a newline")
        _raises(-1, "herro_aligned_dev_paf: " + text, m.paf, names, [99])
        _raises(-1, "herro_pairs_paf: " + text, p.paf, m, names)
        _raises(-1, "herro_pairs_write_alns: " + text, p.write_alns, m, names, path)
    # rec out of range, naming the index
    _raises(-1, "herro_aligned_dev_paf: rec[2] = 6 is outside the 6 records", m.paf, K.UNIQUE, [0, 5, 6])
    # a handle of another context
    other = api.HostContext(K.HOST_READ_LEN)
    m_other = K.build(other, (t["rows2"], t["ops2"]))
    p_other = other.pairs_from_table(t["primaries"], None, t["rids"], t["aln_off"], t["rec_of_row"])
    assert L.herro_aligned_dev_paf(ctx.h, m_other.h, 0, None, blob, off.ctypes.data, C.byref(h)) == -1
    assert "herro_aligned_dev_paf: the handle belongs to another context" in ctx.last_error()
    assert L.herro_pairs_paf(ctx.h, p_other.h, m.h, blob, off.ctypes.data, C.byref(h)) == -1 and "another context" in ctx.last_error()
    assert L.herro_pairs_paf(ctx.h, p.h, m_other.h, blob, off.ctypes.data, C.byref(h)) == -1 and "another context" in ctx.last_error()
    assert L.herro_pairs_write_alns(ctx.h, p.h, m_other.h, blob, off.ctypes.data, path.encode(), 1, None, None) == -1
    # not 2 P records
    prim_only = K.build(ctx, (t["rows2"][:3], t["ops2"][:3]))
    _raises(-1, "herro_pairs_paf: the aligned handle has 3 records, the pairs need 6", p.paf, prim_only, K.UNIQUE)
    _raises(-1, "herro_pairs_write_alns: the aligned handle has 3 records, the pairs need 6", p.write_alns, prim_only, K.UNIQUE, path)
    # a record of a read the context does not have
    rows = t["rows2"].copy()
    rows[2, 0] = K.N_READS
    far = K.build(ctx, (rows, t["ops2"]))
    _raises(-1, "herro_aligned_dev_paf: row 1 (record 2): read id outside the read store", far.paf, K.UNIQUE, [0, 2])
    _raises(-1, "herro_pairs_write_alns: row", p.write_alns, far, K.UNIQUE, path)
    # an unknown flag; a directory that does not exist
    assert L.herro_pairs_write_alns(ctx.h, p.h, m.h, blob, off.ctypes.data, path.encode(), 2, None, None) == -1 and "unknown flag" in ctx.last_error()
    _raises(-1, "herro_pairs_write_alns: cannot create", p.write_alns, m, K.UNIQUE, str(tmp_path / "no" / "such.paf"))
    # the Python side counts the names
    with pytest.raises(ValueError):
        m.paf(K.UNIQUE[:-1])
    assert os.listdir(tmp_path) == [] and not h.value                                # no failing call left a file or a handle
    for x in (m_other, p_other, prim_only, far, p, m):
        x.close()
    other.close()


def test_no_reads_is_a_state_error(tmp_path):
    """a context that knows no read: HERRO_E_STATE, from every entry (on a device context: herro_set_reads was not called)"""
    c = api.HostContext(np.zeros(0, np.uint32))
    h = c.aligned_dev_from_ops(np.zeros((0, 9), np.uint32), np.zeros(1, np.uint64), np.zeros(0, np.uint32))
    p = c.pairs_from_table(np.zeros((0, 9), np.uint32), None, np.zeros(0, np.uint32), np.zeros(1, np.uint64), np.zeros(0, np.uint32))
    _raises(-6, "herro_set_reads must be called first", h.paf, [])
    _raises(-6, "herro_set_reads must be called first", p.paf, h, [])
    _raises(-6, "herro_set_reads must be called first", p.write_alns, h, [], str(tmp_path / "never.paf"))
    assert os.listdir(tmp_path) == []
    for x in (h, p):
        x.close()
    c.close()
