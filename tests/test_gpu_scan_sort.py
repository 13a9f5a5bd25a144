"""gpu: the exclusive scan and the stable radix sort every device stage of the front end stands on (csrc/scan_sort_dev.hip: dev_scan_u32, dev_radix_sort) and the
64-bit offset join of the device FASTA (csrc/fasta_dev.hip), run on their own through herro_debug_scan_u32, herro_debug_radix_sort and
herro_debug_offsets64 against the numpy references of tests/scan_sort_cases.py: whole arrays, exactly equal, at the sizes where k_scan_top begins its
second round, where the sort's histogram scan takes a second tile and a second round, with values that wrap modulo 2^32, and with the shift lists the
clients build.  Every array of a call lies in one block exactly as large as its client sizes it, guard words behind it: none may change.
tests/test_scan_sort_cases_host.py proves that the cases reach what they are named for."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import scan_sort_cases as SC  # noqa: E402
from herro_amd import api  # noqa: E402

pytestmark = pytest.mark.gpu

_CTX = {}


def _ctx():
    """a context of its own: the hooks need neither reads nor a model"""
    if "c" not in _CTX:
        _CTX["c"] = api.Context(0)
    return _CTX["c"]


def _report(bad):
    assert not bad, "\n".join(bad)


# ---- scan --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SC.SCAN_SIZES)
def test_scan_equals_the_running_sum_modulo_2_32(n):
    c, bad = _ctx(), []
    for kind in SC.SCAN_VALUES:
        v = SC.scan_values(kind, n)
        got, hits = c.debug_scan_u32(v)
        diff = SC.first_difference(got, SC.scan_ref(v))
        if diff or hits:
            bad.append(f"scan n={n} {kind}: {diff or 'equal'}; guard words changed: {hits}")
    _report(bad)


# ---- sort --------------------------------------------------------------------------------------------------------------------------------------
def _sort_case(c, keys, shifts, tag, bad):
    pays = np.arange(len(keys), dtype=np.uint64)                      # the payload is the original index: stability shows in it
    want_k, want_p = SC.sort_ref(keys, shifts)
    got_k, got_p, hits = c.debug_radix_sort(keys, pays, shifts)
    dk, dp = SC.first_difference(got_k, want_k), SC.first_difference(got_p, want_p)
    if dk or dp or hits:
        bad.append(f"sort {tag} shifts={list(shifts)}: keys {dk or 'equal'}; payloads {dp or 'equal'}; guard words changed: {hits}")


@pytest.mark.parametrize("n", SC.SORT_SIZES)
def test_sort_digit_patterns(n):
    c, bad = _ctx(), []
    shifts = SC.pattern_shifts(n)
    for kind in SC.SORT_PATTERNS:
        _sort_case(c, SC.sort_keys(kind, n, shifts), shifts, f"n={n} {kind}", bad)
    _report(bad)


@pytest.mark.parametrize("name", sorted(SC.shift_lists()))
def test_sort_shift_lists(name):
    c, bad = _ctx(), []
    shifts = SC.shift_lists()[name]
    for n in SC.SHIFT_LIST_SIZES:
        for kind in ("random", "dup3"):
            _sort_case(c, SC.sort_keys(kind, n, shifts), shifts, f"{name} n={n} {kind}", bad)
    _report(bad)


def test_sort_payloads_are_64_bit():
    """cluster_dev.hip carries whole keys as payloads: all 64 bits arrive, at both parities of the pass count"""
    c, bad = _ctx(), []
    for shifts in ([32, 40], [0, 32, 40]):
        keys = SC.sort_keys("random", 2049, shifts)
        pays = ~keys
        order = SC.sort_ref(keys, shifts)[1].astype(np.int64)
        got_k, got_p, hits = c.debug_radix_sort(keys, pays, shifts)
        dk, dp = SC.first_difference(got_k, keys[order]), SC.first_difference(got_p, pays[order])
        if dk or dp or hits:
            bad.append(f"sort shifts={shifts}: keys {dk or 'equal'}; payloads {dp or 'equal'}; guard words changed: {hits}")
    _report(bad)


# ---- 64-bit offsets ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SC.OFFSET_SIZES)
def test_offsets64_equal_the_running_sum_in_64_bits(n):
    c, bad = _ctx(), []
    for kind in SC.OFFSET_VALUES:
        b = SC.offset_bytes(kind, n)
        got, hits = c.debug_offsets64(b)
        diff = SC.first_difference(got, SC.offsets_ref(b))
        if diff or hits:
            bad.append(f"offsets64 n={n} {kind}: {diff or 'equal'}; guard words changed: {hits}")
    _report(bad)


def test_no_elements():
    c = _ctx()
    got, hits = c.debug_offsets64([])
    assert got.tolist() == [0] and hits == 0
    k, p, hits = c.debug_radix_sort([], [], [])
    assert len(k) == 0 and len(p) == 0 and hits == 0
