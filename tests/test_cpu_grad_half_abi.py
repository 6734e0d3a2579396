"""CPU-side checks of the half gradient chain's entry points (include/nqa.h, "The same chain on HALF gradient maps"):
declared, exported and bound; they refuse null pointers, bad sizes and misaligned maps on the host under their own
names (an error code and a message, never a launch: no device is touched here); the packed size follows the documented
formula; and nqa_pack_conv_half writes the kRows16 row layout, restated here in numpy."""
import os
import re

import numpy as np
import pytest

NEW = ("nqa_packed_conv_half_bytes", "nqa_pack_conv_half", "nqa_conv3x3_half", "nqa_relu_mask_f16_scaled",
       "nqa_grad_exponent_half", "nqa_l2pool_backward_scaled_half", "nqa_conv1_1_backward_scaled_half")
KERNELS = ("relu_mask_f16_kernel", "absmax_partial_half_kernel", "exponent_finish_half_kernel", "l2pool_backward_half_kernel",
           "conv1_1_backward_half_kernel")
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "nqa.h")

P = [0x10000 + 0x1000 * i for i in range(8)]  # fake, 16-byte aligned device pointers: nothing below may dereference them
E_ARG, E_SHAPE, E_WORKSPACE = -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    from nerf_qa_amd import build, _lib
    build.build()
    return _lib.lib()


def _align(v, a=256):
    return (v + a - 1) // a * a


def test_exports_are_declared_bound_and_present(lib):
    from nerf_qa_amd import _lib, build
    text = open(HEADER).read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, text), name
        assert name in _lib.EXPORTS and getattr(lib, name) is not None, name
    for k in KERNELS:
        assert k in build.NO_SCRATCH, k


def test_packed_bytes_follow_the_documented_formula(lib):
    f = lib.nqa_packed_conv_half_bytes
    for cout, cin in ((64, 64), (64, 128), (256, 512), (512, 512)):
        assert f(cout, cin) == _align(cout * cin * 9 * 2) + _align(cout * 4 + 4), (cout, cin)
    assert f(64, 16) == 0 and f(32, 64) == 0  # cin = 16 is the f32s rows' granularity, cout = 32 half a weight tile
    assert f(0, 64) == 0 and f(64, 0) == 0 and f(-64, 64) == 0 and f(96, 64) == 0 and f(64, 48) == 0


def test_pack_refuses_bad_arguments(lib):
    w = np.zeros((64, 32, 3, 3), dtype=np.float32)
    blob = np.zeros(lib.nqa_packed_conv_half_bytes(64, 32), dtype=np.uint8)
    for args in ((None, 64, 32, blob.ctypes.data), (w.ctypes.data, 64, 32, None), (w.ctypes.data, 32, 32, blob.ctypes.data),
                 (w.ctypes.data, 64, 16, blob.ctypes.data), (w.ctypes.data, 0, 32, blob.ctypes.data)):
        assert lib.nqa_pack_conv_half(*args) == E_ARG, args
        assert b"pack_conv_half: bad argument" in lib.nqa_last_error()


def _row_positions(cout, cin, m16):
    """pack_rows' kRows16 indexing: element index of weight (co, ci, tap) in the rows, as halves.  Tiles [cout/64][cin/32]
    of [9 taps][64 rows][4 positions of 8 halves]; chunk c (channels 8c.. of the tile) of row n lies at position
    c ^ 2*((n>>2)&1) for the 16x16x32 MFMA, c ^ ((n>>2)&3) for the 32x32x16 one."""
    co, ci, t = np.meshgrid(np.arange(cout), np.arange(cin), np.arange(9), indexing="ij")
    ct, n = co // 64, co % 64
    cc, c, j = ci // 32, (ci % 32) // 8, ci % 8
    pos = c ^ (((n >> 2) & 1) * 2 if m16 else (n >> 2) & 3)
    return (((((ct * (cin // 32) + cc) * 9 + t) * 64 + n) * 4 + pos) * 8 + j)


@pytest.mark.parametrize("cout,cin", [(64, 32), (128, 64)], ids=["64x32-mfma32", "128x64-mfma16"])
def test_pack_writes_every_weight_once_in_the_row_layout(cout, cin, lib):
    """(64, 32): the random layer of the issue, on the 32x32x16 swizzle (cout not a multiple of 128); (128, 64): the
    other swizzle and more than one tile in both directions."""
    rng = np.random.default_rng(cout + cin)
    w = (rng.standard_normal((cout, cin, 3, 3)) * 0.03).astype(np.float32)
    nbytes = lib.nqa_packed_conv_half_bytes(cout, cin)
    blob = np.full(nbytes, 0xAB, dtype=np.uint8)
    assert lib.nqa_pack_conv_half(w.ctypes.data, cout, cin, blob.ctypes.data) == 0
    nrows = cout * cin * 9
    rows = blob[:nrows * 2].view(np.float16)
    idx = _row_positions(cout, cin, cout % 128 == 0)
    assert np.array_equal(np.sort(idx.ravel()), np.arange(nrows))  # a bijection: every weight exactly once, no gap
    want = w.reshape(cout, cin, 9).astype(np.float16)              # round to nearest even, as np.float16(w)
    assert np.array_equal(rows[idx].view(np.uint16), want.view(np.uint16))
    assert not blob[nrows * 2:].any()  # padding, the zero bias and the float behind it


def _conv(lib, inp=P[0], n=2, H=5, W=7, cin=64, cout=64, blob=P[1], out=P[2]):
    return lib.nqa_conv3x3_half(inp, n, H, W, cin, cout, blob, out, None)


def test_conv3x3_half_refuses_bad_arguments(lib):
    for kw in ({"inp": None}, {"blob": None}, {"out": None}, {"n": 0}, {"H": 0}, {"W": -1}, {"inp": P[0] + 8},
               {"out": P[2] + 2}, {"H": 1 << 12, "W": 1 << 12, "cin": 128}):  # (the last: 2^31 bytes per image)
        assert _conv(lib, **kw) == E_ARG, kw
        assert b"conv3x3_half" in lib.nqa_last_error()
    for kw in ({"cin": 16}, {"cout": 32}, {"cin": 48}, {"cout": 96}, {"cin": 0}, {"cout": -64}):
        assert _conv(lib, **kw) == E_SHAPE, kw
        assert b"conv3x3_half: cout" in lib.nqa_last_error()


def _mask(lib, g=P[0], half=0, act=P[1], split=0, n=2, pix=35, C=64, k=P[2], out=P[3]):
    return lib.nqa_relu_mask_f16_scaled(g, half, act, split, n, pix, C, k, out, None)


def test_relu_mask_f16_scaled_refuses_bad_arguments(lib):
    for kw in ({"g": None}, {"act": None}, {"k": None}, {"out": None}, {"n": 0}, {"pix": 0}, {"g": P[0] + 4, "half": 1},
               {"act": P[1] + 8}, {"out": P[3] + 2}):
        assert _mask(lib, **kw) == E_ARG, kw
        assert b"relu_mask_f16_scaled" in lib.nqa_last_error()
    for c in (0, 8, 40, -16):
        assert _mask(lib, C=c) == E_SHAPE, c
        assert b"relu_mask_f16_scaled: C" in lib.nqa_last_error()


def test_grad_exponent_half_refuses_bad_arguments(lib):
    call = lib.nqa_grad_exponent_half
    big = 1 << 20
    for args in ((None, 0, 2, 64, P[1], big, P[2], P[3]), (P[0], 0, 2, 64, None, big, P[2], P[3]),
                 (P[0], 1, 2, 64, P[1], big, None, P[3]), (P[0], 1, 0, 64, P[1], big, P[2], P[3]),
                 (P[0], 0, 1 << 16, 64, P[1], big, P[2], P[3]), (P[0], 0, 2, 0, P[1], big, P[2], P[3]),
                 (P[0] + 8, 1, 2, 64, P[1], big, P[2], P[3])):
        assert call(*args, None) == E_ARG, args
        assert b"grad_exponent_half: bad argument" in lib.nqa_last_error()
    assert call(P[0], 0, 2, 66, P[1], big, P[2], None, None) == E_SHAPE   # float: a multiple of 4
    assert call(P[0], 1, 2, 68, P[1], big, P[2], None, None) == E_SHAPE   # half: a multiple of 8
    assert b"multiple of 8" in lib.nqa_last_error()
    assert call(P[0], 1, 2, 64, P[1], 4, P[2], None, None) == E_WORKSPACE
    assert b"grad_exponent_half: workspace" in lib.nqa_last_error()


def test_half_seam_and_end_refuse_bad_arguments(lib):
    lp = lib.nqa_l2pool_backward_scaled_half
    for args in ((None, P[1], P[2], P[3], 2, 5, 7, 64, P[4]), (P[0], None, P[2], P[3], 2, 5, 7, 64, P[4]),
                 (P[0], P[1], None, P[3], 2, 5, 7, 64, P[4]), (P[0], P[1], P[2], None, 2, 5, 7, 64, P[4]),
                 (P[0], P[1], P[2], P[3], 2, 5, 7, 64, None), (P[0], P[1], P[2], P[3], 0, 5, 7, 64, P[4]),
                 (P[0], P[1], P[2], P[3], 2, 5, 0, 64, P[4]), (P[0] + 4, P[1], P[2], P[3], 2, 5, 7, 64, P[4]),
                 (P[0], P[1] + 4, P[2], P[3], 2, 5, 7, 64, P[4]), (P[0], P[1], P[2], P[3], 2, 5, 7, 64, P[4] + 8)):
        assert lp(*args, None) == E_ARG, args
        assert b"l2pool_backward_scaled_half" in lib.nqa_last_error()
    for c in (24, 0, 8):
        assert lp(P[0], P[1], P[2], P[3], 2, 5, 7, c, P[4], None) == E_SHAPE, c
        assert b"l2pool_backward_scaled_half: C" in lib.nqa_last_error()
    c1 = lib.nqa_conv1_1_backward_scaled_half
    for args in ((None, P[1], P[2], P[3], P[4], 2, 5, 7, P[5]), (P[0], P[1], None, P[3], P[4], 2, 5, 7, P[5]),
                 (P[0], P[1], P[2], None, P[4], 2, 5, 7, P[5]), (P[0], P[1], P[2], P[3], None, 2, 5, 7, P[5]),
                 (P[0], P[1], P[2], P[3], P[4], 2, 5, 7, None), (P[0], None, P[2], P[3], P[4], 0, 5, 7, P[5]),
                 (P[0], None, P[2], P[3], P[4], 2, -5, 7, P[5]), (P[0] + 1, None, P[2], P[3], P[4], 2, 5, 7, P[5])):
        assert c1(*args, None) == E_ARG, args
        assert b"conv1_1_backward_scaled_half" in lib.nqa_last_error()
