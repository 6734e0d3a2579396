"""CPU-side checks of the single-stage entry point of the A-DISTS window pass (include/nqa.h: nqa_adists_window_stage, and
nqa_adists_window_grid beside it): declared in the header, exported by the library, bound by _lib.py, and every refusal
happens on the host -- an error code and a message naming the function, never a launch (the pointers below are fakes that
nothing may dereference, and no device is touched).  There is no workspace argument, so a short one cannot be passed."""
import ctypes as C
import os
import re

import pytest
import torch

NEW = ("nqa_adists_window_stage", "nqa_adists_window_grid")
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "nqa.h")

P = [0x10000 + 0x1000 * i for i in range(8)]  # fake device pointers


@pytest.fixture(scope="module")
def lib():
    from nerf_qa_amd import build, _lib
    build.build()
    return _lib.lib()


def test_exports_are_declared_bound_and_present(lib):
    from nerf_qa_amd import _lib, ops
    text = open(HEADER).read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, text), name
        assert name in _lib.EXPORTS and getattr(lib, name) is not None, name
    assert callable(ops.adists_window_stage) and callable(ops.adists_window_stage_into)


def _stage(lib, fx=P[0], fy=P[1], B=2, H=40, W=56, C=64, prec=0, q=P[2], wgt=P[3], strip=0, gamma=P[4], tw=P[5], sw=P[6]):
    return lib.nqa_adists_window_stage(fx, fy, B, H, W, C, prec, q, wgt, strip, gamma, tw, sw, None)


def test_stage_refuses_bad_arguments(lib):
    for kw in ({"fx": None}, {"fy": None}, {"q": None}, {"wgt": None}, {"gamma": None}, {"tw": None}, {"sw": None}):
        assert _stage(lib, **kw) == -1, kw
        assert b"adists_window_stage: null pointer" in lib.nqa_last_error()
    for kw in ({"B": 0}, {"B": -1}, {"H": 0}, {"W": -3}, {"C": 0}, {"C": -64}, {"prec": -1}, {"prec": 4}, {"prec": 7},
               {"H": 0, "C": 5}):
        assert _stage(lib, **kw) == -1, kw
        assert b"adists_window_stage: bad size or prec" in lib.nqa_last_error()
    # strip: 0 or 1..Ho (Ho = 20 here), also where no LDS kernel would run; only its sign under the window
    for kw in ({"strip": -1}, {"strip": 21}, {"strip": 21, "C": 3}, {"strip": 21, "prec": 2}, {"strip": -2, "H": 5},
               {"strip": 21, "C": 7}):
        assert _stage(lib, **kw) == -1, kw
        assert b"adists_window_stage: strip" in lib.nqa_last_error()
    for c in (1, 4, 32, 63, 65, 192, 384, 1024):
        assert _stage(lib, C=c) == -2, c
        assert b"adists_window_stage: unsupported channel count" in lib.nqa_last_error()
    # 2^31 bytes of one image's tap: 32-bit in-image byte offsets (float 512 channels: 2^20 pixels; half: 2^21)
    for kw in ({"H": 1 << 10, "W": 1 << 10, "C": 512}, {"H": 1 << 11, "W": 1 << 10, "C": 512, "prec": 2},
               {"H": 1 << 14, "W": 11185, "C": 3}, {"H": 4, "W": 1 << 21, "C": 64, "prec": 3}):
        assert _stage(lib, **kw) == -2, kw
        assert b"adists_window_stage: map too large" in lib.nqa_last_error()


def test_grid_query(lib):
    g = (C.c_int * 3)()
    grid = lambda *a: (lib.nqa_adists_window_grid(*a, g), tuple(g))
    assert lib.nqa_adists_window_grid(1, 40, 56, 64, 0, 0, None) == -1
    assert b"adists_window_grid: null pointer" in lib.nqa_last_error()
    assert grid(1, 40, 56, 65, 0, 0)[0] == -2 and b"adists_window_grid" in lib.nqa_last_error()
    assert grid(1, 40, 56, 64, 0, 21)[0] == -1 and b"adists_window_grid: strip" in lib.nqa_last_error()
    assert grid(1, 170, 22, 64, 0, 150) == (0, (1, 1, 150))  # one strip of 150 rows: nothing left for a second
    assert grid(1, 90, 23, 128, 3, 33) == (0, (1, 3, 33))
    assert grid(2, 90, 38, 64, 0, 0) == (0, (5, 2, 35))
    assert grid(2, 1080, 1920, 64, 3, 0) == (0, (475, 7, 152))  # full size: strips taller than 64 rows by itself
    for args in ((1, 40, 56, 64, 2, 0), (1, 40, 56, 64, 1, 0), (1, 40, 56, 3, 0, 0), (1, 20, 56, 64, 0, 0)):
        assert grid(*args) == (0, (0, 0, 0)), args  # 16-bit taps, planes, the global branch: no LDS kernel
    from nerf_qa_amd import ops
    try:
        ops.set_conv_variant(ops.DEFAULT_CONV_VARIANT | 8)
        assert grid(1, 40, 56, 64, 0, 0) == (0, (0, 0, 0))
    finally:
        ops.set_conv_variant(ops.DEFAULT_CONV_VARIANT)
    assert grid(1, 40, 56, 64, 0, 0) == (0, (9, 1, 20))


def test_ops_refuse_what_the_kernels_cannot_take():
    from nerf_qa_amd import _lib, ops
    x, q, w = torch.rand(1, 24, 24, 64), torch.rand(8, 1, 64), torch.rand(1, 64)
    with pytest.raises(_lib.NqaError):
        ops.adists_window_stage(x, x, q, w, "f32")  # CPU tensors
