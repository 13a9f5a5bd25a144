"""gpu: the adapter scan (herro_find_adapters) against tests/adapter_ref.py record for record on every read set of
tests/adapter_cases.py, the same bytes at every segment length and on a second call, forward_only, one adapter against 32, and the whole step
end to end: api.trim_reads on the chimeric set gives back the clean reads, and the finder sees the trimmed store as it sees a clean one."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import adapter_cases as AC  # noqa: E402
import adapter_ref as AR  # noqa: E402
import gpu_common as G  # noqa: E402
import pair_cases as PC  # noqa: E402
from herro_amd import api, io  # noqa: E402

pytestmark = pytest.mark.gpu


def _ctx_with(name):
    c = G.ctx()
    PC.load(c, AC.as_reads(AC.get(name)["reads"]))
    return c


def _same(got, want, tag):
    hits, off = got
    assert hits.dtype == AR.HIT_DTYPE == api.ADAPTER_HIT_DTYPE and off.dtype == np.uint64, tag
    if hits.tobytes() != want[0].tobytes():
        n = min(len(hits), len(want[0]))
        bad = next((i for i in range(n) if hits[i] != want[0][i]), n)
        print(tag, "hits", len(hits), "want", len(want[0]), "first difference at", bad, hits[bad:bad + 3], want[0][bad:bad + 3])
    assert len(hits) == len(want[0]) and hits.tobytes() == want[0].tobytes(), tag
    assert np.array_equal(off, want[1]), tag


# ---- 1. every case set, every segment length, twice ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,call", AC.ALL_CALLS, ids=[f"{n}-{i}" for n, i in AC.ALL_CALLS])
def test_hits_equal_the_reference_at_every_segment_length(name, call, monkeypatch):
    c = _ctx_with(name)
    adapters, kw = AC.calls(name)[call]
    want = AC.reference(name, call)
    for seg in AC.SEGS:                                                      # HERRO_ADAPT_SEG is read by every call
        if seg is None:
            monkeypatch.delenv("HERRO_ADAPT_SEG", raising=False)
        else:
            monkeypatch.setenv("HERRO_ADAPT_SEG", str(seg))
        _same(c.find_adapters(adapters, **kw), want, (name, call, seg))
    _same(c.find_adapters(adapters, **kw), want, (name, call, "again"))     # a second call: the same bytes


def test_the_segment_length_is_what_the_environment_says(monkeypatch, capfd):
    c = _ctx_with("runs")
    adapters, kw = AC.calls("runs")[0]
    monkeypatch.setenv("HERRO_ADAPT_STATS", "1")
    n_bases = [len(r) for r in AC.get("runs")["reads"]]
    for seg, used in ((None, 256), (8, 8), (33, 33), (1, 8), (1 << 20, 65536)):
        if seg is None:
            monkeypatch.delenv("HERRO_ADAPT_SEG", raising=False)
        else:
            monkeypatch.setenv("HERRO_ADAPT_SEG", str(seg))
        c.find_adapters(adapters, **kw)
        line = [x for x in capfd.readouterr().err.splitlines() if x.startswith("ADAPT ")][-1]
        assert f"seg={used} segments={sum(-(-n // used) for n in n_bases)} patterns=4 " in line, line


def test_a_hit_buffer_that_is_outgrown_gives_the_same_bytes(monkeypatch, capfd):
    """a first buffer of 1 and of 100 hits (herro_debug_set_adapter_cap): the first scan counts more hits than it holds and the scan runs again at
    the counted size"""
    c = _ctx_with("planted")
    adapters, kw = AC.calls("planted")[0]
    want = AC.reference("planted", 0)
    monkeypatch.setenv("HERRO_ADAPT_STATS", "1")
    try:
        for cap, scans in ((1, 2), (100, 2), (len(want[0]), 1), (0, 1)):
            c.adapter_cap(cap)
            _same(c.find_adapters(adapters, **kw), want, ("cap", cap))
            line = [x for x in capfd.readouterr().err.splitlines() if x.startswith("ADAPT ")][-1]
            assert f"hits={len(want[0])} scans={scans} " in line, line
    finally:
        c.adapter_cap(0)                                                      # (the context is shared by the suite)


# ---- 2. forward_only, one adapter against 32 -------------------------------------------------------------------------------------------------
def test_forward_only_is_the_strand_0_selection():
    c = _ctx_with("planted")
    adapters = AC.get("planted")["adapters"]
    full, _ = c.find_adapters(adapters, max_err_pm=150)
    fwd, off = c.find_adapters(adapters, max_err_pm=150, forward_only=True)
    assert (full["strand"] == 1).sum() > 50 and fwd.tobytes() == full[full["strand"] == 0].tobytes()
    assert off.tolist() == np.concatenate([[0], np.cumsum(np.bincount(fwd["rid"], minlength=c.n_reads))]).tolist()


def test_one_adapter_against_thirty_two():
    """adapter 17 of 32 gives the hits it gives alone; the other 31 (random 8 .. 64-mers) give theirs"""
    c = _ctx_with("planted")
    rng = np.random.default_rng(106)
    many = [AC.LC._rand(rng, int(rng.integers(8, 65))) for _ in range(32)]
    many[17] = AC.A28
    alone, _ = c.find_adapters([AC.A28], max_err_pm=150)
    got, off = c.find_adapters(many, max_err_pm=150)
    sel = got[got["adapter"] == 17].copy()
    sel["adapter"] = 0
    assert len(alone) > 50 and sel.tobytes() == alone.tobytes()
    _same((got, off), AR.find_adapters([AR.store_codes(r) for r in AC.get("planted")["reads"]], many, max_err_pm=150), "32 adapters")


# ---- 3. empty and one-base reads ---------------------------------------------------------------------------------------------------------
def test_empty_and_one_base_reads():
    c = G.ctx()
    for reads in ([b""], [b"A"], [b"", b"", AC.A22, b"", b"C", b""], [b""] * 3):
        PC.load(c, AC.as_reads(reads))
        want = AR.find_adapters([AR.store_codes(r) for r in reads], [AC.A22, b"A" * 8], max_err_pm=500)
        _same(c.find_adapters([AC.A22, b"A" * 8], max_err_pm=500), want, reads)
    assert len(want[0]) == 0
    hits, off = c.find_adapters([AC.A22])
    assert len(hits) == 0 and off.tolist() == [0] * 4


# ---- 4. errors on a context with a device ------------------------------------------------------------------------------------------------
def test_errors():
    other = api.Context(0)
    try:
        with pytest.raises(api.HerroError) as e:
            other.find_adapters([AC.A22])
        assert e.value.code == -6 and "herro_set_reads must be called first" in str(e.value)
        with pytest.raises(api.HerroError) as e:
            other.find_adapters([b"ACGT"])                                   # the adapters first
        assert e.value.code == -1 and "adapter 0" in str(e.value)
    finally:
        other.close()


# ---- 5. end to end -----------------------------------------------------------------------------------------------------------------------
def test_trim_reads_gives_back_the_clean_reads_and_the_finder_sees_them():
    clean, raw, made_of = AC.chimera_parts()
    c = G.ctx()
    rs = AC.as_reads(raw)
    reads = io.Reads([b"read%d" % i for i in range(len(raw))], [None] * len(raw), rs.seq, rs.qual, rs.off)
    cut, stats = api.trim_reads(c, reads, [AC.A28, AC.A22], max_err_pm=AC.CHIMERA_PM)
    o = cut.off.astype(np.int64)
    assert [cut.seq[o[i]:o[i + 1]].tobytes() for i in range(len(cut.ids))] == clean          # byte for byte
    assert cut.ids == [b"read0", b"read1", b"read2_1", b"read2_2", b"read3", b"read4", b"read5_1", b"read5_2", b"read6", b"read7"]
    assert tuple(stats) == (len(raw), 2, 0, sum(map(len, raw)) - sum(map(len, clean))) and c.n_reads == len(clean)
    trimmed = c.find_overlap_pairs(**PC.DEFAULTS)
    PC.load(c, AC.as_reads(clean))
    want = c.find_overlap_pairs(**PC.DEFAULTS)
    assert want.n_pairs == 4
    PC.assert_same_fields(PC.pairs_fields(trimmed), PC.pairs_fields(want), "trimmed store")   # field for field
    PC.load(c, rs)                                                            # ... and the raw store does not: the chimeras pair with four reads each
    untrimmed = c.find_overlap_pairs(**PC.DEFAULTS)
    assert PC.pairs_bytes(untrimmed) != PC.pairs_bytes(want)
    for x in (trimmed, want, untrimmed):
        x.close()
