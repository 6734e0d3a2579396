"""CPU-side checks of the loss path's entry points (include/nqa.h, "DISTS as a loss": nqa_dists_stats_nhwc_backward,
nqa_grad_exponent and the scaled forms of the three chain kernels): they are declared in the header, exported by the
library, bound by _lib.py, and refuse null pointers and bad sizes on the host -- an error code and a message, never a
launch (no device is touched here)."""
import os
import re

import pytest

NEW = ("nqa_dists_stats_nhwc_backward_bytes", "nqa_dists_stats_nhwc_backward", "nqa_grad_exponent_bytes", "nqa_grad_exponent",
       "nqa_relu_mask_split16_scaled", "nqa_l2pool_backward_scaled", "nqa_conv1_1_backward_scaled")
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "nqa.h")

P = [0x10000 + 0x1000 * i for i in range(8)]  # fake, 16-byte aligned device pointers: nothing below may dereference them


@pytest.fixture(scope="module")
def lib():
    from nerf_qa_amd import build, _lib
    build.build()
    return _lib.lib()


def test_exports_are_declared_bound_and_present(lib):
    from nerf_qa_amd import _lib
    text = open(HEADER).read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, text), name
        assert name in _lib.EXPORTS and getattr(lib, name) is not None, name
    assert "NQA_K_COUNT = 7" in text  # the new launches are counted under the existing timing classes


def _stats(lib, tx=P[0], ty=P[1], B=2, H=8, W=8, C=64, g1=P[2], g2=P[3], stride=1475, ws=P[4], ws_bytes=1 << 30, gx=P[5],
           gy=P[6]):
    return lib.nqa_dists_stats_nhwc_backward(tx, ty, B, H, W, C, g1, g2, stride, ws, ws_bytes, gx, gy, None)


def test_stats_backward_bytes(lib):
    f = lib.nqa_dists_stats_nhwc_backward_bytes
    assert f(0, 8, 8, 64) == 0 and f(2, 0, 8, 64) == 0 and f(2, 8, -1, 64) == 0
    assert f(2, 8, 8, 3) == 0 and f(2, 8, 8, 48) == 0 and f(2, 8, 8, 2048) == 0  # C: a power of two in 16..1024
    assert f(1, 1 << 16, 1 << 15, 64) == 0  # more than 2^30 pixels
    for c in (64, 128, 256, 512):
        one = f(1, 40, 56, c)
        assert one >= c * (5 + 6) * 8 and one % 256 == 0  # at least one row of sums and the coefficients
        assert f(3, 40, 56, c) >= 3 * c * (5 + 6) * 8
    assert f(1, 1, 1, 64) > 0


def test_stats_backward_refuses_bad_arguments(lib):
    for kw in ({"tx": None}, {"ty": None}, {"g1": None}, {"g2": None}, {"ws": None}, {"gx": None, "gy": None}, {"B": 0},
               {"B": 1 << 16}, {"H": 0}, {"W": -2}, {"stride": 63}):
        assert _stats(lib, **kw) == -1, kw
        assert b"dists_stats_nhwc_backward: bad argument" in lib.nqa_last_error()
    for c in (3, 48, 8, 2048):
        assert _stats(lib, C=c, stride=4096) == -2, c
        assert b"power of two" in lib.nqa_last_error()
    assert _stats(lib, H=1 << 16, W=1 << 15) == -2
    assert b"2^30" in lib.nqa_last_error()
    assert _stats(lib, tx=P[0] + 4) == -1 and b"aligned" in lib.nqa_last_error()
    assert _stats(lib, gy=P[6] + 8) == -1 and b"aligned" in lib.nqa_last_error()
    need = lib.nqa_dists_stats_nhwc_backward_bytes(2, 8, 8, 64)
    assert need > 0 and _stats(lib, ws_bytes=need - 1) == -3
    assert b"workspace" in lib.nqa_last_error()


def test_grad_exponent_refuses_bad_arguments(lib):
    f = lib.nqa_grad_exponent_bytes
    assert f(0, 64) == 0 and f(2, 0) == 0 and f(2, 6) == 0 and f(-1, 64) == 0
    assert f(1, 4) >= 4 and f(1, 4) % 256 == 0 and f(3, 1 << 24) >= 3 * 4
    call = lib.nqa_grad_exponent
    for args in ((None, 2, 64, P[1], 1 << 20, P[2], P[3]), (P[0], 2, 64, None, 1 << 20, P[2], P[3]),
                 (P[0], 2, 64, P[1], 1 << 20, None, P[3]), (P[0], 0, 64, P[1], 1 << 20, P[2], P[3]),
                 (P[0], 1 << 16, 64, P[1], 1 << 20, P[2], P[3]), (P[0], 2, 0, P[1], 1 << 20, P[2], P[3])):
        assert call(*args, None) == -1, args
        assert b"grad_exponent: bad argument" in lib.nqa_last_error()
    assert call(P[0], 2, 66, P[1], 1 << 20, P[2], None, None) == -2  # elements per image not a multiple of 4
    assert call(P[0] + 4, 2, 64, P[1], 1 << 20, P[2], None, None) == -2  # not 16-byte aligned
    assert call(P[0], 2, 64, P[1], 4, P[2], None, None) == -3
    assert b"workspace" in lib.nqa_last_error()


def test_scaled_chain_kernels_refuse_bad_arguments(lib):
    rm = lib.nqa_relu_mask_split16_scaled
    for args in ((None, P[1], 0, 2, 35, 64, P[2], P[3]), (P[0], None, 0, 2, 35, 64, P[2], P[3]),
                 (P[0], P[1], 0, 2, 35, 64, None, P[3]), (P[0], P[1], 0, 2, 35, 64, P[2], None),
                 (P[0], P[1], 0, 0, 35, 64, P[2], P[3]), (P[0], P[1], 1, 2, 0, 64, P[2], P[3]),
                 (P[0], P[1], 1, 2, 35, 40, P[2], P[3]), (P[0], P[1], 1, 2, 35, 0, P[2], P[3])):
        assert rm(*args, None) == -1, args
        assert b"relu_mask_split16_scaled: bad argument" in lib.nqa_last_error()
    lp = lib.nqa_l2pool_backward_scaled
    for args in ((None, P[1], P[2], P[3], 2, 5, 7, 64, P[4]), (P[0], None, P[2], P[3], 2, 5, 7, 64, P[4]),
                 (P[0], P[1], None, P[3], 2, 5, 7, 64, P[4]), (P[0], P[1], P[2], None, 2, 5, 7, 64, P[4]),
                 (P[0], P[1], P[2], P[3], 2, 5, 7, 64, None), (P[0], P[1], P[2], P[3], 2, 5, 7, 24, P[4]),
                 (P[0], P[1], P[2], P[3], 0, 5, 7, 64, P[4]), (P[0], P[1], P[2], P[3], 2, 5, 0, 64, P[4])):
        assert lp(*args, None) == -1, args
        assert b"l2pool_backward_scaled" in lib.nqa_last_error()
    c1 = lib.nqa_conv1_1_backward_scaled
    for args in ((None, P[1], P[2], P[3], P[4], 2, 5, 7, P[5]), (P[0], P[1], None, P[3], P[4], 2, 5, 7, P[5]),
                 (P[0], P[1], P[2], None, P[4], 2, 5, 7, P[5]), (P[0], P[1], P[2], P[3], None, 2, 5, 7, P[5]),
                 (P[0], P[1], P[2], P[3], P[4], 2, 5, 7, None), (P[0], None, P[2], P[3], P[4], 0, 5, 7, P[5]),
                 (P[0], None, P[2], P[3], P[4], 2, -5, 7, P[5])):
        assert c1(*args, None) == -1, args
        assert b"conv1_1_backward_scaled" in lib.nqa_last_error()
