"""Host-side file formats on either side of the hot path: thin ctypes wrappers over the C ABI
(csrc/fastx.cpp, include/herro_amd.h).

* `read_fastx`  — herro_fastx_read = get_reads (haec_io.rs:37-75) over needletail's record rules: FASTA / FASTQ, gzip,
  multi-line records; records shorter than `min_length` dropped, the header split at the first blank or tab into id /
  description, qualities mandatory, the `core` / `neighbour` filter (a read is kept if it is in either set; applied only
  when both are given).
* `write_window_features` / `write_job_features` — the `herro features` sink (features.rs:724-764, 783-839):
  `<base>/<read id>/<wid>.features.npy` = u8 `[2, L', 31]` (ASCII bases, then qualities), `<wid>.supported.npy` = records
  `{pos: <u2, ins: u1}`, `<wid>.ids.txt` = ranked overlap read ids, one per line.  NPY format 1.0 with the header numpy
  itself writes (the reference goes through the `npyz` crate; byte equality with a real `herro features` run was not
  checked: no Rust here).
"""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np

from . import api

SUPPORTED_DTYPE = np.dtype([("pos", "<u2"), ("ins", "u1")])


@dataclasses.dataclass
class Reads:
    ids: list[bytes]
    descriptions: list[bytes | None]
    seq: np.ndarray   # u8, all reads back to back
    qual: np.ndarray  # u8, same layout
    off: np.ndarray   # u64 [n+1]


def _lib():
    L = api.lib()
    if not getattr(L, "_io_ready", False):
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        L.herro_fastx_read.restype = vp
        L.herro_fastx_read.argtypes = [C.c_char_p, u32, vp, u64, vp, u64]
        L.herro_reads_count.restype = u32
        L.herro_reads_count.argtypes = [vp]
        for n in ("herro_reads_seq", "herro_reads_qual", "herro_reads_off", "herro_reads_ids", "herro_reads_descs"):
            getattr(L, n).restype = vp
            getattr(L, n).argtypes = [vp]
        L.herro_reads_free.restype = None
        L.herro_reads_free.argtypes = [vp]
        L.herro_write_window_features.restype = C.c_int
        L.herro_write_window_features.argtypes = [C.c_char_p, u32, vp, u32, vp, vp, u32, vp, vp, u32]
        L.herro_job_write_features.restype = C.c_int64
        L.herro_job_write_features.argtypes = [vp, C.c_char_p, vp]
        L._io_ready = True
    return L


def read_fastx(path: str, min_length: int = 0, core: set[str] | None = None, neighbour: set[str] | None = None) -> Reads:
    L = _lib()
    keep, n_keep = None, 0
    if core is not None and neighbour is not None:             # haec_io.rs:63: the filter needs both sets
        names = sorted(set(core) | set(neighbour))
        keep = (C.c_char_p * max(len(names), 1))(*[n.encode() for n in names])
        n_keep = len(names)
    err = C.create_string_buffer(256)
    h = L.herro_fastx_read(path.encode(), min_length, keep, n_keep, err, 256)
    if not h:
        raise ValueError(err.value.decode())
    try:
        return _take_reads(L, h)
    finally:
        L.herro_reads_free(h)


read_fastq = read_fastx   # the name the first rounds used


def _take_reads(L, h) -> Reads:
    n = L.herro_reads_count(h)
    def take(addr, count, dt):       # one memcpy out of the library's buffer (np.ctypeslib.as_array builds a ctypes array TYPE of that length first: seconds per GB)
        out = np.empty(count, dt)
        if count:
            C.memmove(out.ctypes.data, addr, out.nbytes)
        return out
    off = take(L.herro_reads_off(h), n + 1, np.uint64)
    nb = int(off[-1])
    seq = take(L.herro_reads_seq(h), nb, np.uint8)
    qual = take(L.herro_reads_qual(h), nb, np.uint8)
    idp = C.cast(L.herro_reads_ids(h), C.POINTER(C.c_char_p))
    dp = C.cast(L.herro_reads_descs(h), C.POINTER(C.c_char_p))
    return Reads([idp[i] for i in range(n)], [dp[i] for i in range(n)], seq, qual, off)


def cut_reads(reads: Reads, pieces) -> Reads:
    """The reads cut to a piece table (herro_reads_cut over a herro_reads_create handle): read x of the result is bases [start, end) of read rid
    of `reads`, in the order of `pieces` (api.PIECE_DTYPE, as api.trim_plan returns them).  A read with one piece keeps its id, one with n > 1
    pieces gives <id>_1 .. <id>_n; descriptions are kept.  ValueError with the library's message on a piece outside its read."""
    L = _lib()
    n = len(reads.ids)
    seq, qual = np.ascontiguousarray(reads.seq, np.uint8), np.ascontiguousarray(reads.qual, np.uint8)
    off = np.ascontiguousarray(reads.off, np.uint64)
    pieces = np.ascontiguousarray(pieces, api.PIECE_DTYPE)
    ids = (C.c_char_p * max(n, 1))(*[bytes(i) for i in reads.ids])
    descs = (C.c_char_p * max(n, 1))(*[None if d is None else bytes(d) for d in reads.descriptions])
    err = C.create_string_buffer(256)
    src = L.herro_reads_create(n, seq.ctypes.data, qual.ctypes.data, off.ctypes.data, ids, descs, err, 256)
    if not src:
        raise ValueError(err.value.decode())
    try:
        h = L.herro_reads_cut(src, len(pieces), pieces.ctypes.data, err, 256)
        if not h:
            raise ValueError(err.value.decode())
        try:
            return _take_reads(L, h)
        finally:
            L.herro_reads_free(h)
    finally:
        L.herro_reads_free(src)


def cut_names(ids, descriptions, off, pieces):
    """ids, descriptions and offsets of the reads that a piece table makes (herro_reads_cut_names: the library's naming rule, as cut_reads
    applies it), from the source reads' ids, descriptions and offsets alone — for a store cut on the device (Context.cut_store), whose bases
    never come to the host.  Returns (ids, descriptions, off u64 [n_pieces + 1]); ValueError with the library's message on a bad table."""
    L = _lib()
    n = len(ids)
    off = np.ascontiguousarray(off, np.uint64)
    if len(off) != n + 1 or len(descriptions) != n:
        raise ValueError("herro_reads_cut_names: off has n + 1 entries, descriptions n")
    pieces = np.ascontiguousarray(pieces, api.PIECE_DTYPE)
    idp = (C.c_char_p * max(n, 1))(*[bytes(i) for i in ids])
    dp = (C.c_char_p * max(n, 1))(*[None if d is None else bytes(d) for d in descriptions])
    err = C.create_string_buffer(256)
    h = L.herro_reads_cut_names(n, off.ctypes.data, idp, dp, len(pieces), pieces.ctypes.data, err, 256)
    if not h:
        raise ValueError(err.value.decode())
    try:
        m = L.herro_reads_count(h)
        out_off = np.empty(m + 1, np.uint64)
        C.memmove(out_off.ctypes.data, L.herro_reads_off(h), out_off.nbytes)
        ip = C.cast(L.herro_reads_ids(h), C.POINTER(C.c_char_p))
        dq = C.cast(L.herro_reads_descs(h), C.POINTER(C.c_char_p))
        return [ip[i] for i in range(m)], [dq[i] for i in range(m)], out_off
    finally:
        L.herro_reads_free(h)


def write_cluster(path: str, mask, names) -> None:
    """One part of Clusters as the file scripts/create_clusters.py writes and `herro inference -c` reads (lib.rs:208-239): `0\t<name>` for every
    core read (mask 1), then `1\t<name>` for every neighbour (mask 2), each in read order; reads with mask 0 are left out.  names[rid]: bytes or str."""
    mask = np.asarray(mask)
    if len(mask) != len(names):
        raise ValueError("write_cluster: one mask byte per name")
    if ((mask != 0) & (mask != 1) & (mask != 2)).any():
        raise ValueError("write_cluster: a mask byte is 0, 1 (core) or 2 (neighbour)")
    as_bytes = lambda x: x if isinstance(x, bytes) else str(x).encode()
    with open(path, "wb") as f:
        for kind, tag in ((1, b"0\t"), (2, b"1\t")):
            for r in np.flatnonzero(mask == kind):
                name = as_bytes(names[int(r)])
                if not name or b"\t" in name or b"\n" in name:
                    raise ValueError(f"write_cluster: read {int(r)}: a name is not empty and holds no tab or newline")
                f.write(tag + name + b"\n")


def read_cluster(path: str, names) -> np.ndarray:
    """The mask (u8 [len(names)]: 1 core, 2 neighbour, 0 neither) of a cluster file.  read_cluster of lib.rs:208-239 splits every line at tabs,
    takes `0` for core and `1` for neighbour and panics on anything else ("Invalid cluster file", lib.rs:231; a line without a tab — an empty one
    included — dies on fields[1]): all of these are a ValueError naming the line here, and so are a name the read set does not have and a read
    listed twice."""
    index = {(x if isinstance(x, bytes) else str(x).encode()): i for i, x in enumerate(names)}
    mask = np.zeros(len(names), np.uint8)
    with open(path, "rb") as f:
        lines = f.read().split(b"\n")
    if lines[-1] == b"":          # (the newline that ends the last line; BufRead::lines drops it too)
        lines.pop()
    for no, line in enumerate(lines, 1):
        fields = line.split(b"\t")
        if len(fields) < 2 or fields[0] not in (b"0", b"1"):
            raise ValueError(f"read_cluster: {path}: line {no}: invalid cluster file (expected `0<tab>name` or `1<tab>name`)")
        r = index.get(fields[1])
        if r is None:
            raise ValueError(f"read_cluster: {path}: line {no}: unknown read {fields[1]!r}")
        if mask[r]:
            raise ValueError(f"read_cluster: {path}: line {no}: read {fields[1]!r} is listed twice")
        mask[r] = 1 if fields[0] == b"0" else 2
    return mask


def write_window_features(out_dir: str, wid: int, ids: list[str], bases: np.ndarray, quals: np.ndarray,
                          sup_pos: np.ndarray, sup_ins: np.ndarray) -> None:
    """bases: ASCII u8 [L',31]; quals u8 [L',31]; supported positions in order (features.rs:724-764)."""
    L = _lib()
    bases = np.ascontiguousarray(bases, np.uint8)
    quals = np.ascontiguousarray(quals, np.uint8)
    sp = np.ascontiguousarray(sup_pos, np.uint16)
    si = np.ascontiguousarray(sup_ins, np.uint8)
    arr = (C.c_char_p * max(len(ids), 1))(*[i.encode() for i in ids])
    rc = L.herro_write_window_features(out_dir.encode(), wid, arr, len(ids), bases.ctypes.data, quals.ctypes.data, bases.shape[0],
                                       sp.ctypes.data, si.ctypes.data, len(sp))
    if rc:
        raise OSError(f"herro_write_window_features failed ({rc}) under {out_dir}")


def write_job_features(job, base_dir: str, read_names: list[str]) -> int:
    """`herro features` for a featurized job (herro_job_write_features): read_names[rid] for every read of the store."""
    L = _lib()
    arr = (C.c_char_p * max(len(read_names), 1))(*[n.encode() for n in read_names])
    n = L.herro_job_write_features(job.h, base_dir.encode(), arr)
    if n < 0:
        job.ctx._chk(int(n))
    return int(n)
