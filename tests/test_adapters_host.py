"""The adapter step without a GPU: the reference of the scan against hand-computed cases, herro_trim_plan against the
reference's rule on generated hit tables and on the rule's corners, herro_reads_cut, and the scan's argument checks on a context without a
device (HERRO_E_INVALID before HERRO_E_NO_DEVICE)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import adapter_cases as AC  # noqa: E402
import adapter_ref as AR  # noqa: E402
from herro_amd import api, io  # noqa: E402

P8 = b"ACGTTGCA"


def _hits(text: bytes, adapters, **kw):
    h, off = AR.find_adapters([AR.store_codes(text)], adapters, **kw)
    assert off.tolist() == [0, len(h)]
    return [tuple(int(x[f]) for f in ("start", "end", "adapter", "strand", "errors")) for x in h]


# ---- 1. the reference against hand-computed cases ---------------------------------------------------------------------------------------------
def test_reference_exact_copy_and_the_bound():
    assert AR.max_errors(8, 1) == 0 and AR.max_errors(8) == 2 and AR.max_errors(64, 500) == 32 and AR.max_errors(9, 250) == 2 and AR.max_errors(28, 150) == 4
    assert _hits(b"TT" + P8 + b"TT", [P8], max_err_pm=1, forward_only=True) == [(2, 10, 0, 0, 0)]
    assert _hits(b"TT" + P8 + b"TT", [P8], max_err_pm=1) == [(2, 10, 0, 0, 0)]                      # rc(P8) = TGCAACGT is not in the text
    assert AR.last_row(AR.adapter_codes(P8), np.zeros(0, np.int64)).tolist() == [8]                # the empty substring: E <= m
    assert AR.last_row(AR.adapter_codes(P8), AR.store_codes(b"TTTT").astype(np.int64)).max() <= 8


def test_reference_one_substitution_insertion_deletion():
    # ACGTTGCA with G -> C at its third base: one error, and the neighbours of j = 10 are in the run (E <= 2) without being its end
    assert _hits(b"TT" + b"ACCTTGCA" + b"TT", [P8], forward_only=True) == [(2, 10, 0, 0, 1)]
    # a base missing in the text: ACGT-GCA
    assert _hits(b"GG" + b"ACGTGCA" + b"GG", [P8], forward_only=True) == [(2, 9, 0, 0, 1)]
    # a base too many in the text: ACGTT+C+GCA
    assert _hits(b"GG" + b"ACGTTCGCA" + b"GG", [P8], forward_only=True) == [(2, 11, 0, 0, 1)]
    # k = 0: the same three texts give nothing
    for t in (b"TTACCTTGCATT", b"GGACGTGCAGG", b"GGACGTTCGCAGG"):
        assert _hits(t, [P8], max_err_pm=1, forward_only=True) == []


def test_reference_ties_take_the_first_end_and_the_largest_start():
    # E(j) = 0 for j = 8, 9, 10: one run, its first position; the only substring ending at 8 at distance 0 begins at 0
    assert _hits(b"A" * 10, [b"A" * 8], max_err_pm=1, forward_only=True) == [(0, 8, 0, 0, 0)]
    # at k = 2 the run begins at j = 6 (AAAAAA: two bases short) and its least E is still first reached at 8
    assert _hits(b"A" * 10, [b"A" * 8], forward_only=True) == [(0, 8, 0, 0, 0)]
    # a text of six bases of an eight-base pattern: E(6) = 2 with T[0, 6); T[1, 6) would cost 3
    assert _hits(P8[:6], [P8], forward_only=True) == [(0, 6, 0, 0, 2)]
    # largest start: CCACGTTGCA holds the copy at 2; from 1 the distance is 1, from 2 it is 0
    assert _hits(b"CC" + P8, [P8], max_err_pm=1, forward_only=True) == [(2, 10, 0, 0, 0)]


def test_reference_strands_palindromes_and_the_order():
    rc = AC.LC.rc(P8)
    assert _hits(b"TT" + rc + b"TT", [P8], max_err_pm=1) == [(2, 10, 0, 1, 0)]                      # forward coordinates on strand 1
    assert _hits(b"TT" + rc + b"TT", [P8], max_err_pm=1, forward_only=True) == []
    pal = b"ACGTACGT"
    assert AC.LC.rc(pal) == pal
    assert _hits(b"GG" + pal + b"GG", [pal], max_err_pm=1) == [(2, 10, 0, 0, 0), (2, 10, 0, 1, 0)]  # one hit per strand
    # two adapters, two reads: ascending (rid, end, start, adapter, strand)
    h, off = AR.find_adapters([AR.store_codes(b"GG" + pal + b"TT" + P8), AR.store_codes(P8 + b"C" + P8)], [P8, pal], max_err_pm=1)
    got = [tuple(int(x[f]) for f in ("rid", "end", "start", "adapter", "strand")) for x in h]
    assert got == [(0, 10, 2, 1, 0), (0, 10, 2, 1, 1), (0, 20, 12, 0, 0), (1, 8, 0, 0, 0), (1, 17, 9, 0, 0)] and off.tolist() == [0, 3, 5]
    for bad in ([b"ACGTACG"], [b"A" * 65], [b"ACGTNCGT"], [], [P8] * 33):
        with pytest.raises(ValueError):
            AR.find_adapters([], bad)
    with pytest.raises(ValueError):
        AR.find_adapters([], [P8], max_err_pm=501)


def test_the_case_sets_reach_what_they_claim():
    def ref(name, call=0):
        return AC.reference(name, call)[0]
    g = AC.get("grid")
    assert [len(r) for r in g["reads"][:-1]] == list(AC.GRID_LENGTHS) and [len(a) for a in g["adapters"]] == list(AC.GRID_ADAPTER_LENGTHS)
    n = [len(ref("grid", c)) for c in range(len(AC.GRID_PM))]
    print("grid hits per bound", n)
    assert n[0] == n[3] and n[1] < n[2] < n[3] < n[4] and n[1] > 0                                 # 0 is the default 250; more errors, more hits
    assert len(g["reads"][0]) == 1 and (ref("grid", 4)["rid"] == 0).sum() == 0                      # one base: shorter than m - k of every adapter
    assert len(g["reads"][1]) == 7 and (ref("grid", 3)["rid"] == 1).sum() > 0 and (ref("grid", 1)["rid"] == 1).sum() == 0   # seven of an adapter's nine: at k = 2, not at k = 0
    p = ref("planted")
    assert len(p) >= 150 and set(p["strand"].tolist()) == {0, 1} and set(p["adapter"].tolist()) == {0, 1, 2}
    assert (p["start"] == 0).any() and (p["end"] == 300).any() and int(p["errors"].max()) == 4
    assert len(AC.reference("planted", 1)[0]) < len(p)
    pal = p[p["adapter"] == 2]
    assert len(pal) and len(pal) % 2 == 0 and np.array_equal(pal["end"][0::2], pal["end"][1::2])    # the palindrome: every hit on both strands
    r = ref("runs", 0)
    whole = r[(r["rid"] == 0) & (r["adapter"] == 0)]
    assert whole[["start", "end", "errors", "strand"]].tolist() == [(0, 8, 0, 0)]                   # A x 700: ONE run, from j = 6 to the read's last base
    assert (r[r["rid"] == 3]["strand"] == 1).all() and r[r["rid"] == 3]["end"].tolist() == [98]     # ... T x 530 behind 90 random bases: the other strand
    r5 = ref("runs", 1)
    assert ((r5["rid"] == 1) & (r5["adapter"] == 1) & (r5["errors"] == 0)).any()
    assert len(ref("nonacgt")) >= 10
    assert len(ref("random", 0)) > 0 and (ref("random", 0)["adapter"] == 2).all()                   # the 8-base adapter alone hits by chance at 150 per mille ...
    assert len(ref("random", 1)) >= 50 and len(ref("random", 2)) == 0                               # ... dozens of chance hits at k = 1 in 32 kb; 28 and 22 bases: none


# ---- 2. herro_trim_plan -------------------------------------------------------------------------------------------------------------------
def _table(rows, n_reads):
    """hits (rid, start, end, adapter, errors) -> (hits, hits_off)"""
    rows = sorted(rows, key=lambda x: x[0])
    h = np.zeros(len(rows), AR.HIT_DTYPE)
    for i, (rid, s, e, a, err) in enumerate(rows):
        h[i] = (rid, s, e, a, 0, err)
    off = np.zeros(n_reads + 1, np.uint64)
    for row in rows:
        off[row[0] + 1:] += 1
    return h, off


def _same_plan(read_len, adapter_len, h, off, **kw):
    want = AR.trim_plan(read_len, adapter_len, h, off, **kw)
    got = api.trim_plan(read_len, adapter_len, h, off, **kw)
    assert got[0].dtype == api.PIECE_DTYPE and got[0].tobytes() == want[0].tobytes(), (kw, got[0], want[0])
    assert np.array_equal(got[1], want[1]) and list(got[2]) == want[2], (kw, got[2], want[2])
    return [(int(p["rid"]), int(p["start"]), int(p["end"])) for p in got[0]], got[2]


def test_plan_ends_middle_and_merged_cuts():
    L, m = 2000, [28, 22]
    rows = [(0, 0, 28, 0, 0), (0, 1978, 2000, 1, 1),                        # trimmed at both ends
            (1, 0, 28, 0, 0), (1, 900, 922, 1, 0), (1, 922, 950, 0, 1), (1, 940, 960, 1, 2), (1, 1200, 1228, 0, 3),   # touching + overlapping cuts; 3 errors > 2: ignored
            (2, 500, 528, 0, 2), (2, 1000, 1022, 1, 3),                     # a middle hit at the bound; 3 > floor(22 / 10): ignored
            (3, 149, 177, 0, 7), (3, 150, 178, 0, 7), (3, 1822, 1850, 0, 7), (3, 1823, 1851, 0, 7)]   # the window's edges: start 149 < 150 <= 150; end 1851 > 1850 >= 1850
    h, off = _table(rows, 5)
    pieces, stats = _same_plan([L] * 5, m, h, off)
    assert pieces == [(0, 28, 1978), (1, 28, 900), (1, 960, 2000), (2, 0, 500), (2, 528, 2000), (3, 177, 1823), (4, 0, 2000)]
    assert tuple(stats) == (3, 2, 0, 28 + 22 + 28 + 60 + 28 + 177 + 177)
    pieces, stats = _same_plan([L] * 5, m, h, off, discard_chimeras=True)
    assert pieces == [(0, 28, 1978), (3, 177, 1823), (4, 0, 2000)] and tuple(stats) == (3, 0, 2, 50 + 2000 + 2000 + 354)
    pieces, _ = _same_plan([L] * 5, m, h, off, end_window=100, end_max_err_pm=100, mid_max_err_pm=250)
    assert [p for p in pieces if p[0] == 3] == [(3, 0, 149), (3, 178, 1822), (3, 1851, 2000)] and (2, 1022, 2000) in pieces             # read 3's hits are middle hits now (7 <= 7), read 2's second one counts


def test_plan_precedence_on_reads_shorter_than_two_windows():
    # L = 200: [60, 88) is a start hit (60 < 150) although it also ends inside the end window (88 > 50); [170, 198) is an end hit
    h, off = _table([(0, 60, 88, 0, 0), (0, 170, 198, 0, 0)], 1)
    assert _same_plan([200], [28], h, off)[0] == [(0, 88, 170)]
    # L = 100: both are start hits, lo = 98: two bases stay
    h, off = _table([(0, 0, 28, 0, 0), (0, 70, 98, 0, 0)], 1)
    assert _same_plan([100], [28], h, off)[0] == [(0, 98, 100)]
    # lo >= hi: a start hit reaching into an end hit; and an adapter dimer, nothing but adapters
    h, off = _table([(0, 100, 190, 0, 0), (0, 180, 208, 0, 0), (1, 0, 28, 0, 0), (1, 28, 56, 0, 0)], 2)
    pieces, stats = _same_plan([300, 56], [28], h, off)
    assert pieces == [] and tuple(stats) == (2, 0, 2, 356)
    # a middle hit clipped by lo and one wholly inside the trimmed end
    h, off = _table([(0, 100, 400, 0, 0), (0, 380, 420, 0, 0), (0, 160, 200, 0, 0)], 1)
    assert _same_plan([1000], [28], h, off)[0] == [(0, 420, 1000)]
    # empty reads and reads without hits
    h, off = _table([], 3)
    pieces, stats = _same_plan([0, 5, 0], [28], h, off)
    assert pieces == [(1, 0, 5)] and tuple(stats) == (0, 0, 2, 0)


def test_plan_min_length_at_the_piece_length():
    h, off = _table([(0, 0, 28, 0, 0), (0, 500, 528, 0, 0)], 1)            # pieces of 472 and 1472 bases
    for least, want in ((471, 2), (472, 2), (473, 1), (1472, 1), (1473, 0), (0, 2), (1, 2)):
        pieces, stats = _same_plan([2000], [28], h, off, min_length=least)
        assert len(pieces) == want and stats.reads_dropped == (want == 0) and stats.reads_split == (want == 2), least
    h, off = _table([], 1)
    for L, least, want in ((100, 99, 1), (100, 100, 1), (100, 101, 0)):    # the whole read at len - 1, len, len + 1
        assert len(_same_plan([L], [28], h, off, min_length=least)[0]) == want


def test_plan_equals_the_reference_on_generated_tables():
    rng = np.random.default_rng(77)
    for trial in range(120):
        n = int(rng.integers(1, 8))
        read_len = [int(x) for x in rng.choice([0, 1, 30, 120, 149, 150, 151, 299, 300, 301, 700, 2500], n)]
        adapter_len = [int(x) for x in rng.choice([8, 22, 28, 64], int(rng.integers(1, 4)))]
        rows = []
        for r, L in enumerate(read_len):
            for _ in range(int(rng.integers(0, 7)) if L else 0):
                s = int(rng.integers(0, L))
                e = min(L, s + int(rng.integers(1, 80)))
                rows.append((r, s, e, int(rng.integers(0, len(adapter_len))), int(rng.integers(0, 9))))
        h, off = _table(rows, n)
        kw = dict(end_window=int(rng.choice([0, 1, 50, 150, 400])), end_max_err_pm=int(rng.choice([0, 100, 500])),
                  mid_max_err_pm=int(rng.choice([0, 1, 250])), min_length=int(rng.choice([0, 1, 25, 200])), discard_chimeras=bool(trial % 3 == 0))
        _same_plan(read_len, adapter_len, h, off, **kw)


def test_plan_refuses_bad_tables():
    L = api.lib()
    rl, al = np.array([100, 100], np.uint32), np.array([28], np.uint32)

    def call(rows, off=None, params=None):
        h, o = _table(rows, 2)
        o = o if off is None else np.array(off, np.uint64)
        return api._trim_plan(L, rl, al, h, o, params or api.TrimParams())

    call([(0, 10, 38, 0, 0), (1, 100, 100, 0, 0)])                          # fine: a hit may end at the read's last base
    for rows, text in (([(0, 80, 101, 0, 0)], "hit 0: outside its read"), ([(0, 0, 28, 0, 0), (1, 50, 49, 0, 0)], "hit 1: start > end"),
                       ([(0, 0, 28, 1, 0)], "hit 0: adapter index out of range"), ([(1, 0, 28, 0, 0)], None)):
        if text is None:                                                    # a hit filed under another read
            h, o = _table(rows, 2)
            with pytest.raises(ValueError, match="its rid is not the read of its group"):
                api._trim_plan(L, rl, al, h, np.array([0, 1, 1], np.uint64), api.TrimParams())
            with pytest.raises(ValueError):
                AR.trim_plan(rl, al, h, [0, 1, 1])
        else:
            with pytest.raises(ValueError, match=text):
                call(rows)
            with pytest.raises(ValueError):
                AR.trim_plan(rl, al, *_table(rows, 2))
    two = [(0, 0, 28, 0, 0), (0, 50, 78, 0, 0)]
    for off in ([1, 2, 2], [0, 2, 1]):
        with pytest.raises(ValueError, match="hits_off must ascend from 0"):
            call(two, off)
        with pytest.raises(ValueError):
            AR.trim_plan(rl, al, _table(two, 2)[0], off)
    for i in range(3):
        p = api.TrimParams()
        p.reserved[i] = 1
        with pytest.raises(ValueError, match="reserved"):
            call([], params=p)
    with pytest.raises(ValueError, match="unknown flag"):
        call([], params=api.TrimParams(flags=2))
    err = api.C.create_string_buffer(64)
    assert L.herro_trim_plan(2, rl.ctypes.data, 1, al.ctypes.data, None, None, None, None, err, 64) == -1
    h = api.C.c_void_p()
    assert L.herro_trim_plan(2, rl.ctypes.data, 1, al.ctypes.data, None, None, None, api.C.byref(h), err, 64) == -1 and b"null" in err.value and not h.value
    assert L.herro_trim_n_pieces(None) == 0 and L.herro_trim_stats(None, None) == -1
    with pytest.raises(ValueError):
        api.trim_plan(rl, al, np.zeros(1, AR.HIT_DTYPE), [0, 1, 2])         # hits_off beyond the hits: refused before the library reads them


# ---- 3. herro_reads_cut -------------------------------------------------------------------------------------------------------------------
def _reads():
    seqs = [b"ACGTACGTAC", b"", b"GGGTTTCCCAAA", b"T"]
    quals = [bytes(range(40, 40 + len(s))) for s in seqs]
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    return io.Reads([b"r0", b"r1", b"r2", b"r3"], [b"first read", None, b"", None], np.frombuffer(b"".join(seqs), np.uint8),
                    np.frombuffer(b"".join(quals), np.uint8), off), seqs, quals


def _pieces(rows):
    p = np.zeros(len(rows), api.PIECE_DTYPE)
    for i, row in enumerate(rows):
        p[i] = row
    return p


def _split(r):
    o = r.off.astype(np.int64)
    return [r.seq[o[i]:o[i + 1]].tobytes() for i in range(len(r.ids))], [r.qual[o[i]:o[i + 1]].tobytes() for i in range(len(r.ids))]


def test_reads_cut_bytes_ids_and_a_table_out_of_order():
    reads, seqs, quals = _reads()
    for rows in ([(0, 2, 9), (2, 0, 12), (3, 0, 1)],                       # one piece per read: ids stay
                 [(2, 6, 12), (0, 0, 4), (2, 0, 3), (3, 1, 1), (0, 6, 10), (2, 3, 6)],   # out of order, reads 0 and 2 split, an empty piece
                 []):
        p = _pieces(rows)
        got = io.cut_reads(reads, p)
        ids, descs, s, q = AR.cut_reads(reads.ids, reads.descriptions, seqs, quals, p)
        assert got.ids == ids and got.descriptions == descs and _split(got) == (s, q), rows
        assert got.off.tolist() == np.concatenate([[0], np.cumsum([b - a for _, a, b in rows])]).astype(np.int64).tolist()
    got = io.cut_reads(reads, _pieces([(2, 6, 12), (0, 0, 4), (2, 0, 3), (0, 6, 10), (2, 3, 6)]))
    assert got.ids == [b"r2_1", b"r0_1", b"r2_2", b"r0_2", b"r2_3"] and got.descriptions == [b"", b"first read", b"", b"first read", b""]
    assert _split(got)[0] == [b"CCCAAA", b"ACGT", b"GGG", b"GTAC", b"TTT"] and _split(got)[1][3] == bytes(range(46, 50))
    for rows, text in (([(4, 0, 0)], "piece 0: rid outside the reads"), ([(0, 0, 4), (0, 5, 4)], "piece 1: start > end"), ([(3, 0, 2)], "piece 0: end beyond the read")):
        with pytest.raises(ValueError, match=text):
            io.cut_reads(reads, _pieces(rows))
        with pytest.raises(ValueError):
            AR.cut_reads(reads.ids, reads.descriptions, seqs, quals, _pieces(rows))
    L = api.lib()
    err = api.C.create_string_buffer(64)
    assert not L.herro_reads_cut(None, 0, None, err, 64) and b"null" in err.value
    assert not L.herro_reads_create(1, None, None, np.array([1, 1], np.uint64).ctypes.data, (api.C.c_char_p * 1)(b"x"), None, err, 64)


def test_the_planned_pieces_of_the_chimera_set_are_its_clean_reads():
    """the reference's scan, the library's plan and cut: the path of api.trim_reads without the device"""
    clean, raw, made_of = AC.chimera_parts()
    hits, off = AC.reference("chimera", 0)
    pieces, piece_off, stats = api.trim_plan([len(r) for r in raw], [28, 22], hits, off)
    assert np.diff(piece_off.astype(np.int64)).tolist() == [len(m) for m in made_of]
    assert tuple(stats)[:3] == (len(raw), 2, 0) and stats.bases_removed == sum(map(len, raw)) - sum(map(len, clean))
    rs = AC.as_reads(raw)
    cut = io.cut_reads(io.Reads([b"read%d" % i for i in range(len(raw))], [None] * len(raw), rs.seq, rs.qual, rs.off), pieces)
    assert _split(cut)[0] == clean
    assert cut.ids == [b"read0", b"read1", b"read2_1", b"read2_2", b"read3", b"read4", b"read5_1", b"read5_2", b"read6", b"read7"]


# ---- 4. the scan's argument checks on a context without a device -----------------------------------------------------------------------------
def test_the_scan_checks_its_arguments_before_it_asks_for_a_device():
    c = api.HostContext([100, 200])
    good = [P8, b"ACGT" * 16]

    def code(adapters, **kw):
        with pytest.raises(api.HerroError) as e:
            c.find_adapters(adapters, **kw)
        return e.value.code, str(e.value)

    assert code(good)[0] == -2 and "no device" in code(good)[1]                                     # everything valid: HERRO_E_NO_DEVICE
    assert code(good, max_err_pm=500, forward_only=True)[0] == -2
    for adapters, text in (([P8, b"ACGTACG"], "adapter 1: 8 <= length <= 64"), ([b"A" * 65], "adapter 0: 8 <= length <= 64"),
                           ([P8, P8, b"ACGTACGNACGT"], "adapter 2: base 7 is not A, C, G or T"), ([], "1 <= n_adapters <= 32"), ([P8] * 33, "1 <= n_adapters <= 32")):
        assert code(adapters) == (-1, code(adapters)[1]) and text in code(adapters)[1], adapters
    assert code([b"acgtTGCA"])[0] == -2                                                             # either case
    assert code(good, max_err_pm=501)[0] == -1 and "max_err_pm <= 500" in code(good, max_err_pm=501)[1]
    L, h = c._l, api.C.c_void_p()
    off = np.array([0, 8], np.uint64)
    for p in (api.AdapterParams(flags=2), api.AdapterParams(reserved=(0, 1)), api.AdapterParams(reserved=(1, 0))):
        assert L.herro_find_adapters(c.h, 1, P8, off.ctypes.data, api.C.byref(p), api.C.byref(h)) == -1 and not h.value
    assert L.herro_find_adapters(c.h, 1, P8, off.ctypes.data, None, api.C.byref(h)) == -2            # NULL: the defaults
    assert L.herro_find_adapters(None, 1, P8, off.ctypes.data, None, api.C.byref(h)) == -1
    assert L.herro_find_adapters(c.h, 1, P8, off.ctypes.data, None, None) == -1
    assert L.herro_find_adapters(c.h, 1, None, off.ctypes.data, None, api.C.byref(h)) == -1
    assert L.herro_adapter_hits_n(None) == 0 and not L.herro_adapter_hits_data(None) and not L.herro_adapter_hits_off(None)
    L.herro_adapter_hits_free(None)
    assert L.herro_debug_set_adapter_cap(None, 0) == -1 and L.herro_debug_set_adapter_cap(c.h, 5) == 0
    assert code(good)[0] == -2                                                                      # the hook changes no check
    c.close()
