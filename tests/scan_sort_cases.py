"""Cases and references for the device primitives every stage of the front end stands on (csrc/scan_sort_dev.hip: the exclusive scan dev_scan_u32 and the
stable LSD radix sort dev_radix_sort; csrc/fasta_dev.hip: the 64-bit offset join), as tests/test_gpu_scan_sort.py runs them through herro_debug_scan_u32,
herro_debug_radix_sort and herro_debug_offsets64.  The references are plain numpy in 64 bits; tests/test_scan_sort_cases_host.py proves with the
constants below that the sizes reach every seam they are named for.

The kernels' constants: a scan tile is SC_TILE elements (256 threads x 8); k_scan_top is ONE workgroup that walks the tile totals TOP_STEP at a time
with a running carry, so its second round begins past TOP_STEP * SC_TILE elements.  A sort pass counts its digits per block of SC_TILE keys into a
histogram of 256 x blocks entries and scans that."""
from __future__ import annotations

import numpy as np

SC_TILE = 2048                       # elements of a scan tile and keys of a sort block (scan_sort_dev.h: SC_TILE)
TOP_STEP = 256                       # tile totals per round of k_scan_top (its block)
SCAN_SEAM = TOP_STEP * SC_TILE       # 524 288: above it k_scan_top runs a second round
U32 = 0xFFFFFFFF


def blocks(n: int) -> int:
    return (n + SC_TILE - 1) // SC_TILE


def top_rounds(n: int) -> int:
    """rounds of k_scan_top for a scan of n elements"""
    return (blocks(n) + TOP_STEP - 1) // TOP_STEP


def hist_entries(n: int) -> int:
    """what a sort pass over n keys scans: one count per (digit, block)"""
    return 256 * blocks(n)


# ---- scan ------------------------------------------------------------------------------------------------------------------------------------
SCAN_SIZES = [0, 1, 7, 8, 9, 2047, 2048, 2049, 4096, SCAN_SEAM - 1, SCAN_SEAM, SCAN_SEAM + 1, SCAN_SEAM + SC_TILE + 1, 1048579, 3000001]
SCAN_VALUES = ["ones", "random", "all_max", "zeros", "seam_ones"]
SEAM_INDICES = [0, 7, 8, 2047, 2048, SCAN_SEAM - 1, SCAN_SEAM]      # and n - 1


def scan_values(kind: str, n: int) -> np.ndarray:
    if kind == "ones":
        return np.ones(n, np.uint32)
    if kind == "random":                       # the full range: the prefix wraps modulo 2^32 every other element
        return np.random.default_rng(1000 + n).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    if kind == "all_max":
        return np.full(n, U32, np.uint32)
    if kind == "zeros":
        return np.zeros(n, np.uint32)
    if kind == "seam_ones":
        v = np.zeros(n, np.uint32)
        v[[i for i in SEAM_INDICES + [n - 1] if 0 <= i < n]] = 1
        return v
    raise KeyError(kind)


def scan_ref(v: np.ndarray) -> np.ndarray:
    return (np.concatenate([np.zeros(1, np.uint64), np.cumsum(v, dtype=np.uint64)]) & np.uint64(U32)).astype(np.uint32)


# ---- sort ------------------------------------------------------------------------------------------------------------------------------------
SORT_SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 16385, SCAN_SEAM + 1, 4194305]
SORT_LARGE = SCAN_SEAM + 1           # from here on two passes only: the numpy reference stays around a second
SORT_PATTERNS = ["random", "equal", "digit0", "digit255", "lane", "parity", "wave", "descending", "dup3"]


def pattern_shifts(n: int) -> list:
    """the passes of the digit-pattern cases: three (an odd count: the result lies in the second pair of arrays), two at the large sizes"""
    return [0, 8] if n >= SORT_LARGE else [0, 8, 16]


def _with_digits(base: np.ndarray, shifts, digit) -> np.ndarray:
    """base with the 8 bits at every shift replaced by digit(pass)"""
    k = base.copy()
    for j, sh in enumerate(shifts):
        k = (k & ~(np.uint64(255) << np.uint64(sh))) | (digit(j).astype(np.uint64) << np.uint64(sh))
    return k


def sort_keys(kind: str, n: int, shifts) -> np.ndarray:
    """u64 [n].  The digit patterns are stated by index: k_rs_scatter takes the keys of a block in rounds of 256, key i in lane i & 63 of wave
    (i >> 6) & 3 of round (i >> 8) & 7 — so the first pass meets them as stated, the later ones grouped by the digits before."""
    rng = np.random.default_rng(2000 + n)
    i = np.arange(n, dtype=np.uint64)
    rnd = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    lane, wave, rnd8 = i & np.uint64(63), (i >> np.uint64(6)) & np.uint64(3), (i >> np.uint64(8)) & np.uint64(7)
    if kind == "random":
        return rnd
    if kind == "equal":
        return np.full(n, 0x0123456789ABCDEF, np.uint64)
    if kind == "digit0":
        return _with_digits(rnd, shifts, lambda j: np.zeros(n, np.uint64))
    if kind == "digit255":
        return _with_digits(rnd, shifts, lambda j: np.full(n, 255, np.uint64))
    if kind == "lane":                         # a wave holds 64 distinct digits
        return _with_digits(rnd, shifts, lambda j: (lane + np.uint64(64 * j)) & np.uint64(255))
    if kind == "parity":                       # two digits, alternating by lane parity
        return _with_digits(rnd, shifts, lambda j: np.where((lane & np.uint64(1)) == 1, np.uint64(201 - j), np.uint64(17 + j)))
    if kind == "wave":                         # one digit per wave, different in the four waves of a round, and each digit in another wave every round
        return _with_digits(rnd, shifts, lambda j: np.uint64(37) * ((wave + rnd8 + np.uint64(j)) & np.uint64(3)) + np.uint64(5))
    if kind == "descending":
        return np.uint64(n) - np.uint64(1) - i if n else i
    if kind == "dup3":
        return np.array([0x00000000000000FF, 0x0000000100000100, 0xFFFFFFFFFFFF0001], np.uint64)[rng.integers(0, 3, n)]
    raise KeyError(kind)


def sort_ref(keys: np.ndarray, shifts):
    """(sorted keys, the original index of each): LSD over the digits, every pass stable"""
    order = np.arange(len(keys), dtype=np.int64)
    for sh in shifts:
        order = order[np.argsort(((keys[order] >> np.uint64(sh)) & np.uint64(255)).astype(np.uint8), kind="stable")]   # (u8: numpy's own radix sort)
    return keys[order], order.astype(np.uint64)


def bits_of(v: int) -> int:
    return int(v).bit_length()


def field_shifts(lo: int, nbits: int) -> list:
    """scan_sort_dev.h field_shifts: the digits that cover bits [lo, lo + nbits) — the last one may reach beyond the field"""
    return list(range(lo, lo + nbits, 8))


CL_LEVEL_BITS = 7                    # cl_build sorts by bits_of(min(levels, n)) bits of level; its sweeps count levels in batches of 64


def shift_lists() -> dict:
    L = {"empty": [], "one": [0], "two": [0, 8], "three": [0, 8, 16], "top_byte": [56], "all_eight": list(range(0, 64, 8))}
    # cl_build (cluster_dev.hip): arcs by source; reads by (component, level); neighbour keys by (part, read)
    for id_bits in (9, 17):
        L[f"cl_arcs_id{id_bits}"] = field_shifts(32, id_bits)
        L[f"cl_order_id{id_bits}"] = field_shifts(0, CL_LEVEL_BITS) + field_shifts(32, id_bits)
        for k in (3, 256):
            L[f"cl_nb_id{id_bits}_k{k}"] = field_shifts(0, id_bits) + field_shifts(32, bits_of(k))
    # the finder (overlap_dev.hip, overlap_rows.hip): minimizers by hash (2 k bits, k = 15 and 28), anchors by (tpos, qpos) and then by (t, q, strand) with its field at
    # bit 33, chains by score, rows by (target, query)
    L["ovl_hash_k15"] = field_shifts(0, 30)
    L["ovl_hash_k28"] = field_shifts(0, 56)
    L["ovl_anchor_pos"] = field_shifts(0, bits_of(50000)) + field_shifts(32, bits_of(50000))
    L["ovl_anchor_pair"] = field_shifts(0, 1 + bits_of(2999)) + field_shifts(33, bits_of(1499))
    L["ovl_chain_score"] = [0, 8, 16, 24]
    L["ovl_rows"] = field_shifts(0, bits_of(2999)) + field_shifts(32, bits_of(2999))
    return L


SHIFT_LIST_SIZES = [65, 2049, 16385]


# ---- 64-bit offsets ---------------------------------------------------------------------------------------------------------------------------
OFFSET_SIZES = [1, 2, 2047, 2048, 2049, SCAN_SEAM + 1]
OFFSET_VALUES = ["random", "all_max", "pairs", "mix", "seam_wrap"]


def offset_bytes(kind: str, n: int) -> np.ndarray:
    if kind == "random":                       # [1, 2^31]: the low prefix wraps every few pieces
        return np.random.default_rng(3000 + n).integers(1, (1 << 31) + 1, n, dtype=np.uint64)
    if kind == "all_max":
        return np.full(n, U32, np.uint64)
    if kind == "pairs":                        # the low prefix lands exactly on 0 behind every second piece
        return np.full(n, 1 << 31, np.uint64)
    if kind == "mix":                          # high words of their own, low words of 0 or little
        vals = np.array([1 << 32, (1 << 32) + 5, 3 << 32, 1, U32, 0, (1 << 31) + 7], np.uint64)
        return vals[(np.arange(n) * 5 + np.random.default_rng(3100 + n).integers(0, 2, n)) % len(vals)]
    if kind == "seam_wrap":                    # all 1 but two pieces sized so that the low prefix is 2^32 - 1 at 2047 and at 524 287, and 0 behind them
        b = np.ones(n, np.uint64)
        b[0] = (1 << 32) - 2047
        if n > 2048:
            b[2048] = (1 << 32) - 1 - (SCAN_SEAM - 1 - 2049)
        return b
    raise KeyError(kind)


def offsets_ref(b: np.ndarray) -> np.ndarray:
    return np.concatenate([np.zeros(1, np.uint64), np.cumsum(b, dtype=np.uint64)])


def first_difference(got: np.ndarray, want: np.ndarray) -> str:
    """'' when equal, else where the arrays first differ"""
    if got.shape != want.shape:
        return f"shape {got.shape} != {want.shape}"
    d = np.flatnonzero(got != want)
    return "" if not len(d) else f"{len(d)} of {len(want)} differ, first at {int(d[0])}: got {int(got[d[0]])}, want {int(want[d[0]])}"
