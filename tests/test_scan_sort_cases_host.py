"""not-gpu: the case family of tests/scan_sort_cases.py proves — with its own constants and references alone — that it holds what
tests/test_gpu_scan_sort.py is there to run: a size at every seam of the scan and of the sort's histogram scan, the digit patterns as stated, shift
lists of both parities with partial last digits and a field at bit 32 behind one at bit 0, offsets whose exact sums fit.  The three test hooks
refuse a context without a device and null arguments with the library's usual codes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import scan_sort_cases as SC
from herro_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _csrc(*names):
    return "".join(open(os.path.join(ROOT, "herro_amd", "csrc", n)).read() for n in names)


def test_the_constants_are_the_kernels():
    src = _csrc("scan_sort_dev.h", "scan_sort_dev.hip")
    items = int(re.search(r"constexpr int SC_ITEMS = (\d+);", src).group(1))
    assert re.search(r"constexpr uint32_t SC_TILE = 256 \* SC_ITEMS;", src) and 256 * items == SC.SC_TILE == 2048
    assert re.search(r"for \(uint32_t b0 = 0; b0 < nb; b0 \+= 256\)", src) and SC.TOP_STEP == 256      # k_scan_top's walk
    assert SC.SCAN_SEAM == 524288


# ---- scan --------------------------------------------------------------------------------------------------------------------------------------
def test_scan_sizes_sit_on_every_seam():
    S = set(SC.SCAN_SIZES)
    assert {0, 1, 7, 8, 9} <= S                                                        # nothing, one element, a thread's 8 items and either side
    assert {SC.SC_TILE - 1, SC.SC_TILE, SC.SC_TILE + 1, 2 * SC.SC_TILE} <= S           # one tile, and the first element of the second
    seam = SC.SCAN_SEAM
    assert {seam - 1, seam, seam + 1, seam + SC.SC_TILE + 1} <= S
    assert SC.top_rounds(seam) == 1 and SC.blocks(seam) == 256                          # the last size of one round: 256 totals
    assert SC.top_rounds(seam + 1) == 2 and SC.blocks(seam + 1) == 257                  # the second round holds one total ...
    assert SC.blocks(seam + SC.SC_TILE + 1) == 258                                      # ... and two, the second one a partial tile
    assert SC.top_rounds(1048579) == 3 and SC.top_rounds(3000001) == 6                  # carries through several rounds
    assert [n for n in SC.SCAN_SIZES if SC.top_rounds(n) > 1] == [seam + 1, seam + SC.SC_TILE + 1, 1048579, 3000001]


def test_scan_values_are_what_they_are_named_for():
    n = SC.SCAN_SEAM + SC.SC_TILE + 1
    r = SC.scan_values("random", n)
    assert r.dtype == np.uint32 and int(r.max()) > 0xFFFF0000 and int(r.min()) < 0x10000
    wraps = np.count_nonzero(np.diff(SC.scan_ref(r).astype(np.int64)) < 0)
    assert wraps > n // 3                                                               # the prefix wraps modulo 2^32 all the time
    assert SC.scan_ref(SC.scan_values("all_max", 5)).tolist() == [0, 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFC, 0xFFFFFFFB]
    assert SC.scan_ref(SC.scan_values("ones", 3)).tolist() == [0, 1, 2, 3] and not SC.scan_values("zeros", 9).any()
    s = SC.scan_values("seam_ones", n)
    assert np.flatnonzero(s).tolist() == [0, 7, 8, 2047, 2048, SC.SCAN_SEAM - 1, SC.SCAN_SEAM, n - 1]
    assert np.flatnonzero(SC.scan_values("seam_ones", 9)).tolist() == [0, 7, 8] and len(SC.scan_values("seam_ones", 0)) == 0
    # the second round of k_scan_top starts with a carry that is not zero in every pattern but the zeros
    for kind in SC.SCAN_VALUES:
        carry = int(SC.scan_ref(SC.scan_values(kind, n))[SC.SCAN_SEAM])
        assert (carry != 0) == (kind != "zeros"), kind


# ---- sort --------------------------------------------------------------------------------------------------------------------------------------
def test_sort_sizes_sit_on_every_seam():
    S = set(SC.SORT_SIZES)
    assert {0, 1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049} <= S                  # a wave, a round of 256, a block, and either side of each
    assert SC.hist_entries(16384) == SC.SC_TILE and 16385 in S and SC.hist_entries(16385) == 2304 and SC.blocks(SC.hist_entries(16385)) == 2
    assert SC.SCAN_SEAM + 1 in S and SC.blocks(SC.SCAN_SEAM + 1) == 257
    big = 4194305
    assert big in S and big == SC.SC_TILE * SC.SC_TILE + 1 and SC.hist_entries(big) == 524544
    assert SC.top_rounds(SC.hist_entries(big)) == 2 and SC.top_rounds(SC.hist_entries(big - 1)) == 1
    assert [n for n in SC.SORT_SIZES if SC.top_rounds(SC.hist_entries(n)) > 1] == [big]
    assert all(len(SC.pattern_shifts(n)) == (2 if n >= SC.SCAN_SEAM + 1 else 3) for n in SC.SORT_SIZES)
    assert 4 * 8 * big + 4 * (2 * SC.hist_entries(big) + 4 * SC.SC_TILE) < 140e6           # the largest sort: about 135 MB of device memory


def _digits(keys, sh):
    return ((keys >> np.uint64(sh)) & np.uint64(255)).astype(np.int64)


def test_digit_patterns_are_what_they_are_named_for():
    n = 4097
    shifts = SC.pattern_shifts(n)
    assert set(SC.SORT_PATTERNS) == {"random", "equal", "digit0", "digit255", "lane", "parity", "wave", "descending", "dup3"}
    keys = {p: SC.sort_keys(p, n, shifts) for p in SC.SORT_PATTERNS}
    assert all(k.dtype == np.uint64 and len(k) == n for k in keys.values())
    assert len(np.unique(keys["random"])) == n and int(keys["random"].max()) >> 60 and len(np.unique(keys["equal"])) == 1
    for sh in shifts:
        assert not _digits(keys["digit0"], sh).any() and (_digits(keys["digit255"], sh) == 255).all()
    assert len(np.unique(keys["digit0"])) == n                                          # the other bits differ: stability shows
    d = _digits(keys["lane"], 0)
    assert all(len(set(d[w:w + 64])) == 64 for w in range(0, n - 64, 64))               # every wave: 64 distinct digits
    d = _digits(keys["parity"], 0)
    assert len(set(d[0::2])) == 1 and len(set(d[1::2])) == 1 and d[0] != d[1]
    d = _digits(keys["wave"], 0)
    for r in range(0, n - 256, 256):                                                    # a round of 256 keys: four waves, one digit each, all different
        per_wave = [set(d[r + 64 * w:r + 64 * w + 64]) for w in range(4)]
        assert all(len(s) == 1 for s in per_wave) and len(set.union(*per_wave)) == 4
    assert len({int(d[256 * r]) for r in range(4)}) == 4                                # and wave 0 holds another digit every round: wcnt sums over every wave
    assert (np.diff(keys["descending"].astype(np.int64)) == -1).all() and len(np.unique(keys["dup3"])) == 3
    assert len(SC.sort_keys("descending", 0, shifts)) == 0 and SC.sort_keys("descending", 1, shifts).tolist() == [0]


def test_sort_reference_equals_np_sort_where_the_shifts_cover_the_key():
    all8 = SC.shift_lists()["all_eight"]
    assert all8 == [0, 8, 16, 24, 32, 40, 48, 56]
    for kind in SC.SORT_PATTERNS:
        k = SC.sort_keys(kind, 3001, all8)
        got, order = SC.sort_ref(k, all8)
        assert np.array_equal(got, np.sort(k)) and np.array_equal(order, np.argsort(k, kind="stable").astype(np.uint64)), kind
    k = SC.sort_keys("dup3", 500, [0])
    got, order = SC.sort_ref(k, [])
    assert np.array_equal(got, k) and np.array_equal(order, np.arange(500, dtype=np.uint64))        # nothing moves
    got, order = SC.sort_ref(k, [8])                                                     # by one digit, stable among equals
    assert (np.diff(_digits(got, 8)) >= 0).all() and all((np.diff(order[_digits(got, 8) == v].astype(np.int64)) > 0).all() for v in (0, 1))


def test_shift_lists_hold_what_the_clients_build():
    L = SC.shift_lists()
    assert [len(L[x]) for x in ("empty", "one", "two", "three")] == [0, 1, 2, 3] and L["top_byte"] == [56]
    assert {len(v) % 2 for v in L.values()} == {0, 1}                                    # the result in either pair of arrays
    # cl_build's three lists (cluster_dev.hip), id_bits 9 and 17, k 3 and 256
    assert L["cl_arcs_id9"] == [32, 40] and L["cl_arcs_id17"] == [32, 40, 48]
    assert L["cl_order_id9"] == [0, 32, 40] and L["cl_order_id17"] == [0, 32, 40, 48]
    assert L["cl_nb_id9_k3"] == [0, 8, 32] and L["cl_nb_id9_k256"] == [0, 8, 32, 40]
    assert L["cl_nb_id17_k3"] == [0, 8, 16, 32] and L["cl_nb_id17_k256"] == [0, 8, 16, 32, 40]
    src = _csrc("cluster_dev.hip")
    for call in ("field_shifts(sh, 32, id_bits);", "field_shifts(sh, 0, bits_of(std::min(levels2, n)));", "field_shifts(sh, 0, id_bits);",
                 "field_shifts(sh, 32, bits_of(k));"):
        assert call in src, call
    assert SC.bits_of(64) == SC.CL_LEVEL_BITS and SC.bits_of(3) == 2 and SC.bits_of(256) == 9
    assert 9 % 8 and 17 % 8 and SC.CL_LEVEL_BITS % 8 and SC.bits_of(3) % 8               # fields whose last digit is partial
    for name in ("cl_nb_id9_k3", "cl_order_id17", "ovl_anchor_pos", "ovl_rows"):          # a field at bit 32 sorted after a field at bit 0
        v = L[name]
        assert v[0] == 0 and 32 in v and v == sorted(v)
    # the finder's lists (overlap_dev.hip; the row table's: overlap_rows.hip)
    src = _csrc("overlap_dev.hip", "overlap_rows.hip")
    for call in ("field_shifts(shifts, 0, 2 * k);", "field_shifts(sa, 0, bits_of(max_len));", "field_shifts(sa, 32, bits_of(max_len));",
                 "field_shifts(sb, 0, 1 + bits_of(S.n_reads - 1));", "field_shifts(sb, 33, bits_of(t_hi - t_lo - 1));", "{0, 8, 16, 24}",
                 "field_shifts(shifts, 0, bits_of(n_reads - 1));", "field_shifts(shifts, 32, bits_of(n_reads - 1));"):
        assert call in src, call
    assert L["ovl_hash_k15"] == [0, 8, 16, 24] and L["ovl_hash_k28"] == [0, 8, 16, 24, 32, 40, 48]
    assert L["ovl_anchor_pos"] == [0, 8, 32, 40] and L["ovl_anchor_pair"] == [0, 8, 33, 41] and L["ovl_rows"] == [0, 8, 32, 40]
    assert all(0 <= s <= 63 for v in L.values() for s in v)
    assert SC.SHIFT_LIST_SIZES == [65, 2049, 16385]                                      # less than a block, two blocks, a second tile of the histogram scan


# ---- offsets -----------------------------------------------------------------------------------------------------------------------------------
def _exact_total(b):
    return (int(np.sum(b >> np.uint64(32), dtype=np.uint64)) << 32) + int(np.sum(b & np.uint64(SC.U32), dtype=np.uint64))


@pytest.mark.parametrize("kind", SC.OFFSET_VALUES)
def test_offset_cases_fit_and_wrap_where_they_say(kind):
    assert SC.OFFSET_SIZES == [1, 2, 2047, 2048, 2049, SC.SCAN_SEAM + 1]
    for n in SC.OFFSET_SIZES:
        b = SC.offset_bytes(kind, n)
        assert b.dtype == np.uint64 and len(b) == n
        total = _exact_total(b)
        assert total < 1 << 64 and int(np.sum(b >> np.uint64(32), dtype=np.uint64)) + n < 1 << 32      # the high words and every carry fit 32 bits
        ref = SC.offsets_ref(b)
        assert int(ref[-1]) == total and (n > 64 or ref.tolist() == [sum(int(x) for x in b[:i]) for i in range(n + 1)])
        lo = (ref & np.uint64(SC.U32)).astype(np.int64)
        falls = np.flatnonzero(np.diff(lo) < 0)                                          # pieces at which the low prefix wraps (k_fa_carry's test)
        if kind == "random" and n >= 2047:
            assert n // 8 < len(falls) < n // 2 and int(b.min()) >= 1 and int(b.max()) <= 1 << 31
        if kind == "all_max":
            assert falls.tolist() == list(range(1, n)) and (b == SC.U32).all()           # every piece but the first lowers the low prefix by one
        if kind == "pairs":
            assert (lo[0::2] == 0).all() and (lo[1::2] == 1 << 31).all() and falls.tolist() == list(range(1, n, 2))
        if kind == "mix" and n >= 2047:
            assert {1 << 32, (1 << 32) + 5, 3 << 32} <= set(int(x) for x in np.unique(b))
            hi = ref >> np.uint64(32)
            assert int(hi[-1]) > n // 2 and ((b & np.uint64(SC.U32)) == 0).any() and ((b >> np.uint64(32)) == 3).any()
        if kind == "seam_wrap":
            want = [p for p in (2047, SC.SCAN_SEAM - 1) if p < n]
            assert falls.tolist() == want                                                # the wrap exactly at pieces 2047 / 2048 and 524 287 / 524 288
            for p in want:
                assert lo[p] == SC.U32 and lo[p + 1] == 0


# ---- the hooks' refusals ---------------------------------------------------------------------------------------------------------------------
def test_the_hooks_refuse_null_arguments_and_a_context_without_a_device():
    L = api.lib()
    c = api.HostContext([10, 20])
    hits = C.c_uint32(0)
    v32, v64, out = np.ones(4, np.uint32), np.ones(4, np.uint64), np.zeros(5, np.uint64)
    sh = np.array([0, 64], np.uint32)
    assert L.herro_debug_scan_u32(None, v32.ctypes.data, 4, out.ctypes.data, C.byref(hits)) == -1
    assert L.herro_debug_radix_sort(None, v64.ctypes.data, v64.ctypes.data, 4, sh.ctypes.data, 1, C.byref(hits)) == -1
    assert L.herro_debug_offsets64(None, v64.ctypes.data, 4, out.ctypes.data, C.byref(hits)) == -1
    for call, name in ((lambda: L.herro_debug_scan_u32(c.h, None, 4, out.ctypes.data, C.byref(hits)), "herro_debug_scan_u32"),
                     (lambda: L.herro_debug_scan_u32(c.h, v32.ctypes.data, 4, None, C.byref(hits)), "herro_debug_scan_u32"),
                     (lambda: L.herro_debug_scan_u32(c.h, v32.ctypes.data, 4, out.ctypes.data, None), "herro_debug_scan_u32"),
                     (lambda: L.herro_debug_radix_sort(c.h, None, v64.ctypes.data, 4, sh.ctypes.data, 1, C.byref(hits)), "herro_debug_radix_sort"),
                     (lambda: L.herro_debug_radix_sort(c.h, v64.ctypes.data, None, 4, sh.ctypes.data, 1, C.byref(hits)), "herro_debug_radix_sort"),
                     (lambda: L.herro_debug_radix_sort(c.h, v64.ctypes.data, v64.ctypes.data, 4, None, 1, C.byref(hits)), "herro_debug_radix_sort"),
                     (lambda: L.herro_debug_radix_sort(c.h, v64.ctypes.data, v64.ctypes.data, 4, sh.ctypes.data, 1, None), "herro_debug_radix_sort"),
                     (lambda: L.herro_debug_offsets64(c.h, None, 4, out.ctypes.data, C.byref(hits)), "herro_debug_offsets64"),
                     (lambda: L.herro_debug_offsets64(c.h, v64.ctypes.data, 4, None, C.byref(hits)), "herro_debug_offsets64"),
                     (lambda: L.herro_debug_offsets64(c.h, v64.ctypes.data, 4, out.ctypes.data, None), "herro_debug_offsets64")):
        assert call() == -1 and c.last_error() == name + ": null argument"
    assert L.herro_debug_radix_sort(c.h, v64.ctypes.data, v64.ctypes.data, 4, sh.ctypes.data, 2, C.byref(hits)) == -1
    assert c.last_error() == "herro_debug_radix_sort: shift 1 is above 63"
    # well-formed calls: the context has no device
    for fn, name in ((c.debug_scan_u32, "herro_debug_scan_u32"), (c.debug_offsets64, "herro_debug_offsets64")):
        with pytest.raises(api.HerroError) as e:
            fn([1, 2, 3])
        assert e.value.code == -2 and name + ": the context has no device" in str(e.value)
    with pytest.raises(api.HerroError) as e:
        c.debug_radix_sort([3, 1], [0, 1], [0])
    assert e.value.code == -2 and "herro_debug_radix_sort: the context has no device" in str(e.value)
    c.close()
