"""not-gpu: the host half of herro_load_model (csrc/model_pack.h) through herro_debug_model_pack — the file reader, the bf16 / f16 / e4m3
conversions, the MFMA fragment orders the weight-streaming kernels read (model_dev.h: Weight::phi, Weight::p8), the scale rule of the e4m3
copies and the slot matrix of conv1-as-GEMM.  Expected values are numpy's: the layouts as index arrays gathered from the row-major [N][K]
matrix, written from the formulas in model_dev.h's comments; the formats from numpy.float16 and integer arithmetic on the bits."""
import ctypes as C
import struct

import numpy as np
import pytest

from herro_amd import api, model_io

HP = model_io.Hyper()
E_NO_MODEL = -5
FRAG_SHAPES = [(32, 32), (64, 96), (96, 64)]          # (K, N): one fragment; several k-steps and column blocks, non-square; conv2's shape


def pack(path, tensor, K, N, form, dtype=np.uint16, room=None):
    """(array herro_debug_model_pack wrote, s8) or the negative code"""
    out = np.zeros(room if room is not None else max(K * N, 1), dtype)
    s8 = C.c_uint32(0)
    n = api.lib().herro_debug_model_pack(str(path).encode(), tensor.encode(), K, N, form, out.ctypes.data, out.nbytes, C.byref(s8))
    if n < 0:
        return int(n)
    assert n % out.itemsize == 0
    return out[:n // out.itemsize], int(s8.value)


def write(path, **tensors):
    model_io.write_flat(str(path), {k: np.ascontiguousarray(v, np.float32) for k, v in tensors.items()}, HP)
    return path


def frag16_index(K, N):
    """Weight::phi: element ((((n/32) * 2 + jt) * (K/32) + ks) * 64 + lane) * 8 + e = W[32 (n/32) + 8 (fr >> 2) + 4 jt + (fr & 3)][32 ks + 8 fg + e],
    lane = 16 fg + fr -> (row, column) of every packed element, in packed order"""
    nb, jt, ks, fg, fr, e = np.unravel_index(np.arange(K * N), (N // 32, 2, K // 32, 4, 16, 8))
    return 32 * nb + 8 * (fr >> 2) + 4 * jt + (fr & 3), 32 * ks + 8 * fg + e


def frag8_index(K, N):
    """Weight::p8: byte ((((n/32) * 2 + jt) * (K/128) + s) * 2 + half) * 1024 + lane * 16 + j = W[32 (n/32) + 8 (fr >> 2) + 4 jt + (fr & 3)][128 s + 32 fg + 16 half + j]"""
    nb, jt, s, half, fg, fr, j = np.unravel_index(np.arange(K * N), (N // 32, 2, K // 128, 2, 4, 16, 16))
    return 32 * nb + 8 * (fr >> 2) + 4 * jt + (fr & 3), 128 * s + 32 * fg + 16 * half + j


def bf16_bits(w):
    """f32 -> bf16, round to nearest even, by integer arithmetic on the bits (finite inputs)"""
    u = np.ascontiguousarray(w, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_split(w):
    hi = bf16_bits(w)
    back = (hi.astype(np.uint32) << 16).view(np.float32)
    return hi, bf16_bits(w - back)


def f16_split(w):
    with np.errstate(over="ignore", invalid="ignore"):
        hi = w.astype(np.float16)
        lo = (w - hi.astype(np.float32)).astype(np.float16)
    return hi.view(np.uint16), lo.view(np.uint16)


def weights(rng, K, N, bound=4.0):
    w = rng.normal(0, 1, (N, K))
    return (w * (bound / np.abs(w).max())).astype(np.float32)


SPECIALS = np.array([0.0, -0.0, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, 65504.0, 65519.9, 65520.0], np.float32)


@pytest.mark.parametrize("K,N", FRAG_SHAPES)
def test_fragment_order_of_the_16_bit_planes(tmp_path, K, N):
    w = weights(np.random.default_rng(K * 1000 + N), K, N)
    w[np.unravel_index(np.arange(7) * 5 % (K * N), w.shape)] *= 2.0 ** -9      # a few small ones: their bf16 / f16 remainders differ in kind
    path = write(tmp_path / "w.hrro", w=w)
    row, col = frag16_index(K, N)
    assert len(set(zip(row.tolist(), col.tolist()))) == K * N               # the order is a permutation of the matrix
    bh, bl = bf16_split(w)
    fh, _ = f16_split(w)
    for form, plane in ((0, bh), (1, bl), (2, fh)):
        got, _ = pack(path, "w", K, N, form)
        assert got.shape == (K * N,) and np.array_equal(got, plane[row, col]), (K, N, form)


def test_f16_and_bf16_hi_lo_round_to_nearest_even(tmp_path):
    K, N = 32, 32
    w = weights(np.random.default_rng(3), K, N).reshape(-1)
    w[:2 * len(SPECIALS)] = np.concatenate([SPECIALS, -SPECIALS])
    path = write(tmp_path / "w.hrro", w=w.reshape(N, K))
    fh, fl = f16_split(w)
    assert fh[:10].tolist() == [0x0000, 0x8000, 0x3C00, 0x3C02, 0x0001, 0x0000, 0x0001, 0x7BFF, 0x7BFF, 0x7C00]   # ties to even, the subnormal and the overflow edge
    for form, want in ((3, fh), (4, fl)):
        got, _ = pack(path, "w", K, N, form)
        assert np.array_equal(got, want), (form, np.flatnonzero(got != want)[:8])
    # bf16 (finite inputs: everything here but nothing above — 65520 is finite in bf16), through the identity part of the fragment order
    row, col = frag16_index(K, N)
    bh, bl = bf16_split(w.reshape(N, K))
    for form, want in ((0, bh), (1, bl)):
        got, _ = pack(path, "w", K, N, form)
        assert np.array_equal(got, want[row, col]), form
    ties = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20], np.float32)   # bf16 keeps 7 fraction bits: down to even, up to even, above the tie
    assert bf16_bits(ties).tolist() == [0x3F80, 0x3F82, 0x3F81]


E4M3_CASES = [(448.0, 127), (449.0, 128), (1e-3, 109), (0.0, 127), (2.0 ** 40, 159), (2.0 ** 45, 159)]   # (max |w|, s8 = 127 - sw); the last lies past the clamp of sw at -32


@pytest.mark.parametrize("K,N", [(128, 32), (256, 64)])
def test_e4m3_copies_and_their_scale(tmp_path, K, N):
    L = api.lib()
    row, col = frag8_index(K, N)
    for top, s8_want in E4M3_CASES:
        top = np.float32(top)
        w = weights(np.random.default_rng(int(K + s8_want)), K, N, 1.0) * top
        w = np.clip(w, -top, top).astype(np.float32)
        w[N // 2, K // 3] = -top                                               # the maximum itself, exactly
        assert np.abs(w).max() == top
        path = write(tmp_path / f"w{s8_want}_{float(top):g}.hrro", w=w)
        got, s8 = pack(path, "w", K, N, 5, np.uint8)
        assert s8 == s8_want, (float(top), s8)
        scaled = (w * np.float32(2.0 ** (127 - s8_want)))[row, col]
        vals, inv = np.unique(scaled.view(np.uint32), return_inverse=True)
        codes = np.array([L.herro_debug_e4m3(float(v)) for v in vals.view(np.float32)], np.uint8)
        assert got.shape == (K * N,) and np.array_equal(got, codes[inv]), (float(top), K, N)
        if top:
            assert (got & 0x7F).max() >= 0x76, float(top)                      # the format's range is used: the largest lands in (224, 448]


def test_conv1_as_a_gemm(tmp_path):
    rng = np.random.default_rng(9)
    t1 = rng.normal(0, 0.5, (3, 12, 64)).astype(np.float32)
    wq1 = rng.normal(0, 0.05, (3, 64)).astype(np.float32)
    b1 = rng.normal(0, 0.1, 64).astype(np.float32)
    path = write(tmp_path / "c.hrro", t1=t1, wq1=wq1, b1=b1)
    g = np.zeros((64, 96), np.uint16)                   # [channel][tap * 32 + slot]
    th, tl = f16_split(t1)
    qh, ql = f16_split(wq1)
    bh, bl = f16_split(b1)
    for tap in range(3):
        s = g[:, tap * 32:(tap + 1) * 32]
        s[:, 0:12] = th[tap].T                          # slots 0 .. 11: table, hi
        s[:, 13] = s[:, 14] = qh[tap]                   # 13, 14: quality, hi
        s[:, 16:28] = tl[tap].T                         # 16 .. 27: table, lo
        s[:, 29] = ql[tap]                              # 29: quality, lo
        if tap == 0:
            s[:, 15], s[:, 31] = bh, bl                 # 15 / 31: bias hi / lo, tap 0 only
    row, col = frag16_index(96, 64)
    got, _ = pack(path, "", 0, 0, 6, room=96 * 64)
    assert np.array_equal(got, g[row, col])
    assert (g[:, 12] == 0).all() and (g[:, 28] == 0).all() and (g[:, 30] == 0).all() and (g[:, 32 + 15] == 0).all()


def _one_tensor(nd, dims, payload, magic=model_io.MAGIC):
    head = struct.pack("<11If", magic, 1, HP.rows, HP.kw, HP.c1, HP.c2, HP.d_model, HP.n_heads, HP.d_ff, HP.n_layers, 1, HP.ln_eps)
    return head + b"w".ljust(32, b"\0") + struct.pack("<5I", nd, *dims) + payload


GOOD = np.arange(64, dtype=np.float32).tobytes()
WRAP_TO_64 = [64 * 5, 107367629, 536903681]             # 2^58 + 1 = 5 * 107367629 * 536903681
assert WRAP_TO_64[0] * WRAP_TO_64[1] * WRAP_TO_64[2] == 2 ** 64 + 64 and max(WRAP_TO_64) < 2 ** 32
MALFORMED = {
    "cut inside a tensor": _one_tensor(2, [8, 8, 0, 0], GOOD)[:-100],
    "dims beyond the file": _one_tensor(2, [1000, 1000, 0, 0], GOOD),
    "dims wrap 64 bits": _one_tensor(4, [65536, 65536, 65536, 65537], GOOD),          # 2^64 + 2^48: 2^48 after the wrap
    "dims wrap to the size": _one_tensor(3, WRAP_TO_64 + [0], GOOD),                  # ... and 2^64 + 64 -> 64, the very size that is there
    "nd = 5": _one_tensor(5, [8, 8, 1, 1], GOOD),
    "wrong magic": _one_tensor(2, [8, 8, 0, 0], GOOD, magic=model_io.MAGIC ^ 1),
    "zero length": b"",
}


@pytest.mark.parametrize("what", list(MALFORMED))
def test_malformed_files_are_refused(tmp_path, what):
    good = tmp_path / "good.hrro"
    good.write_bytes(_one_tensor(2, [8, 8, 0, 0], GOOD))
    got, _ = pack(good, "w", 8, 8, 3)                                      # the hand-written form is the format
    assert np.array_equal(got, np.arange(64, dtype=np.float16).view(np.uint16))
    bad = tmp_path / "bad.hrro"
    bad.write_bytes(MALFORMED[what])
    assert pack(bad, "w", 8, 8, 3) == E_NO_MODEL
    assert pack(good, "w", 8, 4, 3) == E_NO_MODEL and pack(good, "v", 8, 8, 3) == E_NO_MODEL   # mis-sized, missing
    assert pack(good, "w", 8, 8, 3)[0].shape == (64,)                       # (and the library is still there)
