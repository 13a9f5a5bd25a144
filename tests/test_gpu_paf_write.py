"""gpu: the PAF / .oec.zst writer on a device (herro_aligned_dev_paf, herro_pairs_paf, herro_pairs_write_alns; k_paf_len and k_paf_write of
csrc/paf_dev.hip).  The text is compared byte for byte with the host formatter's (a HostContext over the same ops) and with
tests/paf_ref.py; the text of found alignments is parsed back by the library's own parser and must give the job that
herro_job_create_paired's arguments give over the device handle — the text path (k_cigar_scan) and the binary one (k_ops_scan) meet there."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import aligned_dev_cases as AC  # noqa: E402
import gpu_common as G  # noqa: E402
import pair_cases as PC  # noqa: E402
import paf_cases as K  # noqa: E402
from herro_amd import api  # noqa: E402

pytestmark = pytest.mark.gpu

HANDLES = K.handles()
_SETS = {}


def _set(name):
    if name not in _SETS:
        _SETS[name] = dict((n, m) for n, m, _ in PC.SETS)[name]()
    return _SETS[name]


def _ctx_with(name):
    c = G.ctx()
    PC.load(c, _set(name))
    return c


def _names(c):
    return [b"read%d" % i for i in range(c.n_reads)]


def _six_reads():
    """a store of paf_cases.N_READS reads: aligned_dev_from_ops takes rows and ops as given, so ten-digit coordinates need no long read"""
    c = G.ctx()
    PC.load(c, PC.Reads([b"ACGTTGCA" * 8] * K.N_READS))
    return c


# ---- (a) the hand-made handles ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(HANDLES))
def test_hand_cases_equal_the_host_formatter_and_the_reference(name):
    c = _six_reads()
    host = api.HostContext(K.HOST_READ_LEN)
    case = HANDLES[name]
    d, h = K.build(c, case), K.build(host, case)
    for names in (K.NAMES, K.UNIQUE):
        for rec in K.selections(d.n):
            got = d.paf(names, rec)
            assert got == h.paf(names, rec), (name, rec)
            assert got == K.want(case, names, rec), (name, rec)
    with pytest.raises(api.HerroError) as e:
        d.paf(K.UNIQUE, [0, d.n])
    assert e.value.code == -1 and f"rec[1] = {d.n} is outside the {d.n} records" in str(e.value)
    for r, bad in K.BAD_NAMES.values():
        names = list(K.UNIQUE)
        names[r] = bad
        with pytest.raises(api.HerroError) as e:
            d.paf(names)
        assert e.value.code == -1 and f"read {r}: " in str(e.value)
    for x in (d, h):
        x.close()
    host.close()


# ---- (b), (d) found alignments: the text, the round trip through the parser, the files -------------------------------------------------------------
def _without_empty_targets(rids, off, rec):
    n = np.diff(off.astype(np.int64))
    return rids[n > 0], np.concatenate([[0], np.cumsum(n[n > 0])]).astype(np.uint64), rec


def _same_windows(ja, jb, tag):
    assert ja.n_windows == jb.n_windows > 0, tag
    ja.featurize(); jb.featurize()
    for w in range(ja.n_windows):
        a, b = ja.window(w), jb.window(w)
        for f, _ in api.WindowInfo._fields_:
            assert getattr(a.info, f) == getattr(b.info, f), (tag, w, f)
        for f in ("bases", "quals", "sup_pos", "sup_ins", "qids"):
            assert np.array_equal(getattr(a, f), getattr(b, f)), (tag, w, f)


def _check_found(c, p, m, tag, tmp_path, windows=False):
    names = _names(c)
    text = p.paf(m, names)
    cigars = [m.cigar(r) for r in range(m.n)]
    assert text == K.REF.paf_cigars(m.rows, cigars, names, p.rec_of_row), tag
    rids, off, rec = api.paired_job_args(p.rids, p.aln_off, p.rec_of_row, m.ok)
    assert text.count(b"\n") == len(rec)
    paf = api.Paf(names, text=text)
    want_rows = [tuple(int(v) for v in m.rows[r, :9]) + (cigars[r],) for r in rec]
    assert paf.rows() == want_rows, tag
    rids2, off2, rec2 = _without_empty_targets(rids, off, rec)
    assert paf.targets.tolist() == rids2.tolist() and paf.aln_off.tolist() == off2.tolist(), tag
    if len(rec):
        jt = c.create_job_from_paf(paf, 256)
        ja = c.create_job_aligned(rids2, off2, rec2, m, 256)
        AC.same_jobs(c, ja, jt, tag)
        if windows:
            _same_windows(ja, jt, tag)
        jt.close(); ja.close()
    # (d) both files, read back by the library's reader
    plain, oec = str(tmp_path / "a.paf"), str(tmp_path / "0.oec.zst")
    assert p.write_alns(m, names, plain) == (len(rec), len(text)) and open(plain, "rb").read() == text
    lines, size = p.write_alns(m, names, oec)
    assert lines == len(rec) and size == os.path.getsize(oec)
    back = api.Paf(names, path=oec)
    assert back.rows() == want_rows and back.targets.tolist() == rids2.tolist() and back.aln_off.tolist() == off2.tolist(), tag
    assert sorted(os.listdir(tmp_path)) == ["0.oec.zst", "a.paf"]
    back.close(); paf.close()
    return text


@pytest.mark.parametrize("name,kw", [("A", PC.DEFAULTS), ("A", PC.SMALL_K), ("D", PC.DEFAULTS), ("E", PC.DEFAULTS)],
                         ids=["A-defaults", "A-small-k", "D", "E"])
def test_found_alignments_round_trip(name, kw, tmp_path):
    c = _ctx_with(name)
    p = c.find_overlap_pairs(**kw)
    m = p.align()
    text = _check_found(c, p, m, (name, kw), tmp_path, windows=(name == "A" and kw is PC.DEFAULTS))
    if name == "E":
        assert p.n_pairs == 0 and text == b"" and os.path.getsize(tmp_path / "a.paf") == 0          # ... and the .oec.zst holds "0\n" alone
    else:
        assert p.n_pairs >= 4 and text.count(b"\n") >= p.n_pairs
    p.close(); m.close()


# ---- (e) a core mask: fewer rows than records ---------------------------------------------------------------------------------------------------
def test_a_core_handle_writes_the_rows_of_its_table_only(tmp_path):
    c = _ctx_with("A")
    mask = (np.arange(c.n_reads) % 2 == 0).astype(np.uint8)
    p = c.find_overlap_pairs(core=mask, **PC.DEFAULTS)
    m = p.align()
    assert 0 < p.n_rows < 2 * p.n_pairs == m.n
    text = _check_found(c, p, m, "core", tmp_path)
    targets = {ln.split(b"\t")[5] for ln in text.split(b"\n")[:-1]}
    assert targets and targets <= {b"read%d" % i for i in range(0, c.n_reads, 2)}
    p.close(); m.close()


# ---- (c) the scratch budget ---------------------------------------------------------------------------------------------------------------------
_CHILD = r"""
import json, os, sys
sys.path.insert(0, os.path.join(sys.argv[1], "tests")); sys.path.insert(0, sys.argv[1])
from herro_amd import api
import pair_cases as PC
import paf_cases as K
c = api.Context(0)
PC.load(c, PC.set_b())
p = c.find_overlap_pairs(**PC.SMALL_K)
m = p.align()
out = [p.paf(m, [b"read%d" % i for i in range(c.n_reads)]).hex()]
PC.load(c, PC.Reads([b"ACGTTGCA" * 8] * K.N_READS))
out.append(K.build(c, K.long_handle()).paf(K.NAMES).hex())
print(json.dumps(out))
"""


def test_a_small_scratch_budget_gives_the_same_bytes():
    """Set B at k = 15, w = 5 in a fresh process with HERRO_PAF_SCRATCH_MB=1 and at the default: the same bytes, from more than one chunk in the
    small run.  A chunk's text is a sixteenth of the budget, 64 KiB here; set B's text is 156 lines, 71 722 bytes.  The same two runs write
    paf_cases.long_handle(): ~700 KB, a dozen chunks, one of them a single line longer than a chunk."""
    runs = []
    for mb in ("1", None):
        env = dict(os.environ, HERRO_PAF_STATS="1")
        env.pop("HERRO_PAF_SCRATCH_MB", None)
        if mb:
            env["HERRO_PAF_SCRATCH_MB"] = mb
        r = subprocess.run([sys.executable, "-c", _CHILD, G.ROOT], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        stats = [[int(x) for x in s] for s in re.findall(r"PAF rows=(\d+) lines=(\d+) bytes=(\d+) chunks=(\d+)", r.stderr)]
        assert len(stats) == 2, r.stderr[-500:]
        runs.append(([bytes.fromhex(x) for x in json.loads(r.stdout.strip().splitlines()[-1])], stats))
    (small, s_small), (big, s_big) = runs
    print("PAF budget test: 1 MiB", s_small, "default", s_big)
    assert small[0] == big[0] and len(big[0]) == s_big[0][2] == s_small[0][2] and s_big[0][1] >= 80
    assert s_big[0][3] == 1 and s_small[0][3] > 1, (s_small, s_big)
    case = K.long_handle()
    assert small[1] == big[1] == K.want(case, K.NAMES)
    assert s_big[1][3] == 1 and s_small[1][3] >= 8, (s_small, s_big)
