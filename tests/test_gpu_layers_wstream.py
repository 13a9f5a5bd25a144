"""-m gpu: the weight stream and the barriers of the encoder stack (k_layers_p / tile_gemm_p, model_h.hip).

When loads are issued and what a barrier waits for may change; the arithmetic may not.  So the logits of the stand-alone forward
are held to the BITS of tests/golden/layers_bits/ — recorded on an MI355X with the library of the commit before the weight ring
(`PYTHONPATH=. HERRO_LIB=<that library> python tests/test_gpu_layers_wstream.py tests/golden/layers_bits` writes them; outputs only, float32,
column 0 the info logit, columns 1..5 the base logits) — at the smallest shapes where the hand-over of the ring between GEMM
calls, a partial tile, the two tile heights and the sibling path can each go wrong, for every FF chunk count parity, and over
repeated and concurrent passes, where a barrier that hands over too little would show as a changed bit.

Every case reads the tile plan back (herro_debug_tile_plan_sib, the planner the forward itself calls) and asserts that the
launches it means to test are the ones that ran.  The default plan (qmode 1) moves every window of <= 32 rows of a short last
round into 32-token tiles, so in these small batches a 64-token tile has guests only behind a sibling window's last tile: batch
(c) and (d) have them there."""
import os
import sys
import threading

import numpy as np
import pytest

import gpu_common as G
from herro_amd import api, model_io

pytestmark = pytest.mark.gpu
TOL = 1e-3
GOLD = os.path.join(G.ROOT, "tests", "golden", "layers_bits")

BATCHES = {   # informative rows per window
    "a": [1, 15, 16, 17, 31, 32],                                    # 32-token tiles only: k_layers_p<., 2>
    "b": [33, 48, 63, 64, 5, 12, 30],                                # four 64-token tiles (one full, three partial), k_layers_p<., 4>; the small windows in 32-token tiles
    "c": [65, 129, 20, 9, 3, 40],                                    # sibling tiles 64 + 1 and 64 + 64 + 1, guests in both last tiles: k_layers_p<., 4, true>
    "d": [1, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 129, 7, 20],    # all three launches in one forward
}
PRECISIONS = [5, 4, 7, 8, 6]
FF_MODELS = [(d_ff, n_layers) for d_ff in (256, 512, 768) for n_layers in (1, 2)]   # 1, 2, 3 passes of the FF loop: single, even, odd (the s_ah / s_al alternation ends on the other plane)
FF_COUNTS = [40, 20]   # 40 tokens in one 64-token tile, 20 in one 32-token tile


def _batch(counts, seed):
    rng = np.random.default_rng(seed)
    B, L = len(counts), max(220, max(counts) + 40)
    win_len = rng.integers(max(counts), L + 1, B)
    win_len[0] = L
    bases = rng.integers(0, 11, (B, L, 31)).astype(np.uint8)
    quals = rng.integers(33, 90, (B, L, 31)).astype(np.uint8)
    for b in range(B):
        bases[b, win_len[b]:] = 11
        quals[b, win_len[b]:] = 126
    idx = [np.sort(rng.choice(win_len[b], size=k, replace=False)) for b, k in enumerate(counts)]
    return bases, quals, np.array(counts, np.int32), np.concatenate(idx).astype(np.int32)


def _named_batch(name):
    return _batch(BATCHES[name], 100 + ord(name))


def _plan(counts):
    """(sibling tiles, 64-token tiles, 32-token tiles, tile bounds) of the forward's launch over such windows"""
    nb, n64, n32, _, tok, _ = api.debug_tile_plan_sib(np.asarray(counts, np.uint32), packed=True, qmode=1, n_cu=256)
    return nb, n64, n32, tok


def _assert_plan(name):
    nb, n64, n32, tok = _plan(BATCHES[name])
    sizes = np.diff(tok.astype(np.int64))
    if name == "a":
        assert (nb, n64) == (0, 0) and n32 >= 3 and (sizes <= 32).all() and (sizes < 32).any() and (sizes == 32).any(), (nb, n64, n32, sizes)
    elif name == "b":
        assert nb == 0 and n64 == 4 and sorted(sizes[:4].tolist()) == [33, 48, 63, 64] and n32 >= 1, (nb, n64, n32, sizes)
    elif name == "c":
        assert nb == 5 and sizes[0] == 64 and sizes[2] == 64 and sizes[3] == 64, (nb, n64, n32, sizes)
        assert sizes[1] > 1 and sizes[4] > 1, sizes            # guests behind both windows' last token
    else:
        assert nb == 5 and n64 >= 2 and n32 >= 1 and (sizes[nb:nb + n64] < 64).any(), (nb, n64, n32, sizes)


def _logits(c, batch):
    info, base = c.model_forward(*batch)
    return np.concatenate([info[:, None], base], axis=1).astype(np.float32)


def _gold(name):
    return np.load(os.path.join(GOLD, name + ".npy"))


def _ff_model(tmpdir, d_ff, n_layers):
    hp = model_io.Hyper(d_ff=d_ff, n_layers=n_layers)
    raw = model_io.random_raw_params(hp, seed=7000 + d_ff + n_layers)
    path = os.path.join(str(tmpdir), f"ff{d_ff}_l{n_layers}.hrro")
    model_io.export(raw, hp, path)
    return hp, raw, path


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(BATCHES))
def test_same_bits_as_before_the_ring(name, precision):
    _assert_plan(name)
    c = G.ctx()
    try:
        G.select_precision(c, precision)
        assert c.precision() == precision
        got = _logits(c, _named_batch(name))
    finally:
        c.set_precision(api.DEFAULT_PRECISION)
    want = _gold(f"{name}_p{precision}")
    assert got.shape == want.shape
    assert np.array_equal(got, want), (name, precision, float(np.abs(got - want).max()), int((got != want).sum()))


@pytest.fixture(scope="module")
def ff_models(tmp_path_factory):
    import model_ref as MR
    td = tmp_path_factory.mktemp("ff_models")
    batch = _batch(FF_COUNTS, 77)
    out = {}
    for d_ff, n_layers in FF_MODELS:
        hp, raw, path = _ff_model(td, d_ff, n_layers)
        ti, tb = MR.run_batch(MR.build(raw, hp), *batch)
        out[(d_ff, n_layers)] = (path, np.concatenate([ti[:, None], tb], axis=1))
    return batch, out


@pytest.mark.parametrize("precision", [5, 4])
@pytest.mark.parametrize("d_ff,n_layers", FF_MODELS)
def test_other_chunk_counts(ff_models, d_ff, n_layers, precision):
    batch, models = ff_models
    path, twin = models[(d_ff, n_layers)]
    nb, n64, n32, tok = _plan(FF_COUNTS)
    assert (nb, n64, n32) == (0, 1, 1) and np.diff(tok.astype(np.int64)).tolist() == [40, 20]
    c = api.Context(0)
    try:
        c.load_model(path)
        assert f"d_ff {d_ff}" in c.describe_model() and f"layers {n_layers}" in c.describe_model()
        G.select_precision(c, precision)
        assert c.precision() == precision
        got = _logits(c, batch)
    finally:
        c.close()
    want = _gold(f"ff{d_ff}_l{n_layers}_p{precision}")
    err = float(np.abs(got - twin).max())
    print(f"d_ff {d_ff}, {n_layers} layer(s), precision {precision}: max abs logit error against the dense twin {err:.3e}")
    assert got.shape == want.shape and np.array_equal(got, want), (d_ff, n_layers, precision, float(np.abs(got - want).max()))
    assert err <= TOL


def _new_ctx(precision):
    c = api.Context(0)
    c.load_model(model_io.default_model_file(G.CACHE)[0])
    G.select_precision(c, precision)
    assert c.precision() == precision
    return c


@pytest.mark.parametrize("precision", [5, 4])
def test_repeated_passes_are_bit_identical(precision):
    """50 forwards back to back on one context, then on two contexts at the same time (each on its own stream): every pass has
    the bits of the first.  Repetition is where a barrier that no longer orders two LDS accesses would show (the timing of the
    waves of a tile differs from pass to pass, the data must not)."""
    _assert_plan("d")
    batch = _named_batch("d")
    want = _gold(f"d_p{precision}")
    c = _new_ctx(precision)
    try:
        first = _logits(c, batch)
        assert np.array_equal(first, want)
        for k in range(1, 50):
            assert np.array_equal(_logits(c, batch), first), f"pass {k} differs from the first"
    finally:
        c.close()
    cs = [_new_ctx(precision) for _ in range(2)]
    bad = []

    def worker(cx, tag):
        try:
            for k in range(50):
                if not np.array_equal(_logits(cx, batch), first):
                    bad.append((tag, k))
        except Exception as e:   # (a thread's exception would otherwise be lost)
            bad.append((tag, repr(e)))

    try:
        th = [threading.Thread(target=worker, args=(cx, t)) for t, cx in enumerate(cs)]
        for t in th:
            t.start()
        for t in th:
            t.join()
    finally:
        for cx in cs:
            cx.close()
    assert not bad, bad


def record(out_dir):
    """Writes the goldens with whatever library is loaded: to be run with the library of the commit before the change only."""
    import tempfile
    os.makedirs(out_dir, exist_ok=True)
    c = G.ctx()
    for name in BATCHES:
        _assert_plan(name)
        batch = _named_batch(name)
        for p in PRECISIONS:
            ok = G.select_precision(c, p)
            np.save(os.path.join(out_dir, f"{name}_p{p}.npy"), _logits(c, batch))
            print(f"batch {name}, precision {p} ({'selectable' if ok else 'forced'})")
    c.set_precision(api.DEFAULT_PRECISION)
    batch = _batch(FF_COUNTS, 77)
    with tempfile.TemporaryDirectory() as td:
        for d_ff, n_layers in FF_MODELS:
            _, _, path = _ff_model(td, d_ff, n_layers)
            cx = api.Context(0)
            cx.load_model(path)
            for p in (5, 4):
                ok = G.select_precision(cx, p)
                np.save(os.path.join(out_dir, f"ff{d_ff}_l{n_layers}_p{p}.npy"), _logits(cx, batch))
                print(f"d_ff {d_ff}, layers {n_layers}, precision {p} ({'selectable' if ok else 'forced'})")
            cx.close()


if __name__ == "__main__":
    record(sys.argv[1])
