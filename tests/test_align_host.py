"""not-gpu: the aligner's specification (tests/align_ref.py) on hand cases, against the reference's fix_cigar vectors
and against an unbanded Gotoh optimum; herro_paf_parse_coords against herro_paf_parse_indexed on the same PAF without its CIGARs."""
import json
import os
import sys

import numpy as np
import pytest

from herro_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import align_ref as A  # noqa: E402

ENC = {c: i for i, c in enumerate("ACGT")}


def _codes(s: str) -> np.ndarray:
    return np.array([ENC[c] for c in s], np.uint8)


def _one(target: str, query: str, strand: int = 0):
    """align query (as stored) against target with align_ref: reads 0 = target, 1 = query"""
    codes = [A.store_codes(target.encode()), A.store_codes(query.encode())]
    row = np.array([[1, len(query), 0, len(query), strand, 0, len(target), 0, len(target)]], np.uint32)
    out, cig, sc, ok, hend = A.align_records(codes, row)
    return out[0], cig[0], int(sc[0]), bool(ok[0]), hend[0]


def test_fix_cigar_reproduces_the_reference_vectors():
    G = json.load(open(os.path.join(HERE, "golden", "fix_cigar_vectors.json")))
    assert len(G["vectors"]) == 3
    for v in G["vectors"]:
        cig, tsh, qsh = A.fix_cigar(A.parse_cigar(v["cigar_in"].encode()), v["target"], v["query"])
        assert A.cigar_text(cig).decode() == v["cigar_out"]
        assert (tsh, qsh) == (0, 0)


def test_fix_cigar_drops_a_leading_indel_and_zero_matches():
    cig, tsh, qsh = A.fix_cigar([(0, 0), (3, 2), (5, 0), (2, 1), (4, 0)], "GGG" + "ACGTA" + "CCCC", "ACGTA" + "TT" + "CCCC")
    assert (tsh, qsh) == (3, 0) and cig == [(5, 0), (2, 1), (4, 0)]


def test_identical_sequences_give_nM():
    rng = np.random.default_rng(1)
    s = "".join(rng.choice(list("ACGT"), 500))
    out, cig, sc, ok, _ = _one(s, s)
    assert ok and cig == b"500M" and sc == 1000
    assert out[2:4].tolist() == [0, 500] and out[7:9].tolist() == [0, 500]


def test_one_substitution():
    rng = np.random.default_rng(2)
    s = list("".join(rng.choice(list("ACGT"), 300)))
    q = s.copy()
    q[150] = "A" if s[150] != "A" else "C"
    out, cig, sc, ok, _ = _one("".join(s), "".join(q))
    assert ok and cig == b"300M" and sc == 299 * 2 - 4


def test_homopolymer_deletion_ends_up_leftmost():
    t = "ACGTCAGT" + "GATTACAG" * 4 + "C" + "TTTTTT" + "G" + "CAGTGCAT" * 4 + "ACGT"
    k = t.index("TTTTTT")
    q = t[:k + 4] + t[k + 5:]        # one T of the run deleted (its last but one)
    out, cig, sc, ok, _ = _one(t, q)
    assert ok and cig == f"{k}M1D{len(t) - k - 1}M".encode(), cig
    assert sc == 2 * (len(t) - 1) - 6


def test_reverse_strand_record():
    rng = np.random.default_rng(3)
    t = "".join(rng.choice(list("ACGT"), 400))
    rc = t[::-1].translate(str.maketrans("ACGT", "TGCA"))
    out, cig, sc, ok, _ = _one(t, rc, strand=1)
    assert ok and cig == b"400M" and sc == 800
    # the same query forward on strand 0 is mostly mismatches, and still a valid alignment of the full regions
    out0, cig0, sc0, ok0, _ = _one(t, rc, strand=0)
    assert sc0 < sc


def test_net_indel_larger_than_the_band_and_empty_records():
    """The matrix edges push the band (a cell outside the matrix is -inf), so the end cell never leaves it: a gap wider than the band
    is not flagged, it comes out as a valid alignment below the unbanded optimum.  What fails is a record whose CIGAR would be
    empty: one side of zero length (nothing but an indel, which the trim drops)."""
    rng = np.random.default_rng(4)
    t = "".join(rng.choice(list("ACGT"), 600))
    q = t[:200] + t[400:]            # 200 bases deleted: wider than the band
    out, cig, sc, ok, hend = _one(t, q)
    assert ok and hend < A.gotoh_unbanded(_codes(t), _codes(q))
    T, Q = A.record_seqs([A.store_codes(t.encode()), A.store_codes(q.encode())], out)
    assert A.score_cigar(A.parse_cigar(cig), T, Q) == sc
    # a 40-base deletion fits and is found as one gap
    q2 = t[:300] + t[340:]
    out, cig, sc, ok, _ = _one(t, q2)
    assert ok and cig.count(b"D") == 1 and b"40D" in cig
    codes = [A.store_codes(t.encode()), A.store_codes(q.encode())]
    rows = np.array([[1, len(q), 5, 5, 0, 0, len(t), 0, 300], [1, len(q), 0, 100, 1, 0, len(t), 7, 7], [1, len(q), 3, 3, 0, 0, len(t), 9, 9]],
                    np.uint32)
    out, cig, sc, ok, _ = A.align_records(codes, rows)
    assert not ok.any() and cig == [b"", b"", b""] and (sc == A.INT32_MIN).all()
    assert np.array_equal(out[:, :9], rows)


def _mutate(rng, s, err):
    out = []
    for c in s:
        x = rng.random()
        if x < err / 3:
            out.append(rng.choice([b for b in "ACGT" if b != c]))
        elif x < 2 * err / 3:
            out.append(c + rng.choice(list("ACGT")))
        elif x < err:
            continue
        else:
            out.append(c)
    return "".join(out)


def test_banded_score_equals_the_unbanded_optimum():
    rng = np.random.default_rng(5)
    codes, rows, pairs = [], [], []
    for p in range(24):
        n = int(rng.integers(20, 300))
        t = "".join(rng.choice(list("ACGT"), n))
        q = _mutate(rng, t, float(rng.uniform(0.0, 0.08)))
        if not q:
            continue
        codes += [A.store_codes(t.encode()), A.store_codes(q.encode())]
        rows.append([len(codes) - 1, len(q), 0, len(q), 0, len(codes) - 2, len(t), 0, len(t)])
        pairs.append((_codes(t), _codes(q)))
    out, cig, sc, ok, hend = A.align_records(codes, np.array(rows, np.uint32))
    for r, (t, q) in enumerate(pairs):
        assert hend[r] is not None
        assert hend[r] == A.gotoh_unbanded(t, q), r
        if ok[r]:   # the normalised CIGAR re-scores to the reported score on the trimmed regions
            T, Q = A.record_seqs(codes, out[r])
            assert A.score_cigar(A.parse_cigar(cig[r]), T, Q) == sc[r]


def test_store_codes_follow_the_2bit_codec():
    rng = np.random.default_rng(6)
    for trial in range(50):
        s = bytes(rng.choice(list(b"ACGTacgtNn"), int(rng.integers(1, 100))).tolist())
        w = api.encode_2bit(s)
        want = np.array([(int(w[i >> 5]) >> (2 * (i & 31))) & 3 for i in range(len(s))], np.uint8)
        assert np.array_equal(A.store_codes(s), want)


# ---- herro_paf_parse_coords ---------------------------------------------------------------------------------------------
def _paf_lines(seed=7, n_lines=400):
    rng = np.random.default_rng(seed)
    names = [f"read{i}".encode() for i in range(40)]
    lines = []
    for _ in range(n_lines):
        q, t = int(rng.integers(0, 40)), int(rng.integers(0, 40))
        ql, tl = int(rng.integers(100, 5000)), int(rng.integers(100, 5000))
        qs, ts = int(rng.integers(0, ql // 2)), int(rng.integers(0, tl // 2))
        qe, te = int(rng.integers(qs + 1, ql)), int(rng.integers(ts + 1, tl))
        st = b"+-"[int(rng.integers(0, 2))]
        cols = [names[q] if rng.random() > 0.03 else b"unknown", str(ql).encode(), str(qs).encode(), str(qe).encode(), bytes([st]),
                names[t], str(tl).encode(), str(ts).encode(), str(te).encode(), b"500", b"600", b"60", b"tp:A:S", b"cm:i:40"]
        lines.append(cols)
    return names, lines


def test_paf_parse_coords_equals_the_cigar_parser_without_the_cigar_column():
    names, lines = _paf_lines()
    full = b"\n".join(b"\t".join(c + [b"cg:Z:%dM" % (i + 1)]) for i, c in enumerate(lines)) + b"\n"
    bare = b"\n".join(b"\t".join(c) for c in lines) + b"\n"
    ix = api.NameIndex(names)
    for threads in (1, 3):
        a = api.Paf(ix, text=full, threads=threads)
        b = api.Paf(ix, text=bare, threads=threads, cigars=False)
        c = api.Paf(names, text=bare, threads=threads, cigars=False)     # a plain list: a temporary NameIndex
        assert a.n_alns > 100
        for p in (b, c):
            assert p.targets.tolist() == a.targets.tolist()
            assert p.aln_off.tolist() == a.aln_off.tolist()
            ca, cb = a.coords(), p.coords()
            assert np.array_equal(ca[:, :9], cb[:, :9])
            assert (cb[:, 9] == 0).all()
            assert all(x.cigar is None for x in p.alns)
        # nine columns only (nothing after tend) parse as well
        nine = b"\n".join(b"\t".join(c[:9]) for c in lines) + b"\n"
        d = api.Paf(ix, text=nine, threads=threads, cigars=False)
        assert np.array_equal(d.coords(), b.coords())


def test_paf_parse_coords_keeps_the_reference_messages():
    names = [b"r0", b"r1"]
    bad_num = b"r1\t100\t0x\t90\t+\tr0\t120\t5\t95\n"
    bad_strand = b"r1\t100\t0\t90\t*\tr0\t120\t5\t95\n"
    with pytest.raises(api.HerroError, match="Character is not a valid digit"):
        api.Paf(names, text=bad_num, cigars=False)
    with pytest.raises(api.HerroError, match="Invalid strand character"):
        api.Paf(names, text=bad_strand, cigars=False)
    ok = b"r1\t100\t0\t90\t+\tr0\t120\t5\t95\nr1\t100\t1\t91\t+\tr0\t120\t6\t96\nr0\t5\t0\t5\t+\tr0\t5\t0\t5\n"
    p = api.Paf(names, text=ok, cigars=False)
    assert p.n_alns == 1 and p.coords()[0, :9].tolist() == [1, 100, 0, 90, 0, 0, 120, 5, 95]
