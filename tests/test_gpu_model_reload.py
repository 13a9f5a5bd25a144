"""-m gpu: a load that fails leaves the context as it was.  herro_load_model settles the whole file on the host (csrc/model_pack.h) before it
touches the model a context holds: a file that is not a model — a tensor missing, a tensor mis-sized, the file cut short — returns
HERRO_E_NO_MODEL and the loaded model keeps serving, to the bit; a good file then replaces it, and loading the first one again gives the
first logits again."""
import numpy as np
import pytest

import gpu_common as G
import rf_cases as R
from herro_amd import api, model_io

pytestmark = pytest.mark.gpu
E_NO_MODEL = -5


def _same_bits(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def test_a_failed_load_leaves_the_loaded_model_serving(tmp_path):
    rng = np.random.default_rng(41)
    B, L, NS = 2, 48, 16
    bases = rng.integers(0, 11, (B, L, 31)).astype(np.uint8)
    quals = rng.integers(33, 90, (B, L, 31)).astype(np.uint8)
    lens = np.full(B, NS, np.int32)
    flat = np.concatenate([np.sort(rng.choice(L, NS, replace=False)) for _ in range(B)]).astype(np.int32)
    default, raw = model_io.default_model_file(G.CACHE)
    hp = model_io.Hyper()
    folded = model_io.fold(raw, hp)
    no_heads = {k: v for k, v in folded.items() if k != "heads.wt"}
    short = dict(folded)
    short["L0.ff1.wt"] = folded["L0.ff1.wt"].reshape(-1)[:-1]
    bad = []
    for name, tensors, needle in (("no_heads", no_heads, "heads.wt"), ("short", short, "L0.ff1.wt")):
        model_io.write_flat(str(tmp_path / f"{name}.hrro"), tensors, hp)
        bad.append((str(tmp_path / f"{name}.hrro"), needle))
    whole = open(default, "rb").read()
    (tmp_path / "cut.hrro").write_bytes(whole[:len(whole) // 2])
    bad.append((str(tmp_path / "cut.hrro"), "malformed"))

    c = api.Context(0)
    try:
        c.load_model(default)
        first = c.model_forward(bases, quals, lens, flat)
        mode, text = c.precision(), c.describe_model()
        assert np.isfinite(first[0]).all() and np.isfinite(first[1]).all() and np.abs(first[1]).max() > 0
        for path, needle in bad:
            with pytest.raises(api.HerroError) as e:
                c.load_model(path)
            assert e.value.code == E_NO_MODEL and needle in str(e.value), (path, str(e.value))
            assert _same_bits(c.model_forward(bases, quals, lens, flat), first), path
            assert c.precision() == mode and c.describe_model() == text, path
        other = R.export_model("kw1_f16", tmp_path)[0]
        c.load_model(other)
        assert "conv kw 1 " in c.describe_model()
        second = c.model_forward(bases, quals, lens, flat)
        assert not _same_bits(second, first)
        c.load_model(default)
        assert c.precision() == mode
        assert _same_bits(c.model_forward(bases, quals, lens, flat), first)
    finally:
        c.close()
