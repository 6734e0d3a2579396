"""CPU-side checks of the entry point of the A-DISTS back part (include/nqa.h: nqa_adists_chain, with
nqa_adists_chain_dims and nqa_adists_chain_bytes beside it): declared in the header, exported by the library, bound by
_lib.py, and every refusal happens on the host -- an error code and a message naming the function, never a launch (the
pointers below are fakes that nothing may dereference, and no device is touched)."""
import ctypes as C
import os
import re

import pytest
import torch

import chain_refs as R

NEW = ("nqa_adists_chain", "nqa_adists_chain_dims", "nqa_adists_chain_bytes")
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "nqa.h")

FAKE = 0x10000  # fake device pointers start here


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
    assert callable(ops.adists_chain) and callable(ops.adists_chain_into) and callable(ops.adists_chain_dims)


def _dims(lib, H, W):
    mh, mw = (C.c_int * 6)(), (C.c_int * 6)()
    n = lib.nqa_adists_chain_dims(H, W, mh, mw)
    return n, list(zip(mh, mw))


def test_chain_dims_against_hand_computed_plans(lib):
    one = (1, 1)
    assert _dims(lib, 20, 20) == (0, [one] * 6)
    assert _dims(lib, 20, 500) == (0, [one] * 6) and _dims(lib, 500, 20) == (0, [one] * 6)
    assert _dims(lib, 21, 21) == (2, [one] * 6)  # windowed, and one element
    assert _dims(lib, 21, 22) == (2, [(1, 2), (1, 2)] + [one] * 4)
    assert _dims(lib, 24, 21) == (2, [(4, 1), (4, 1)] + [one] * 4)
    assert _dims(lib, 41, 41) == (3, [(21, 21), (21, 21)] + [one] * 4)  # the 21 x 21 tap of stage 2: windowed 1 x 1
    assert _dims(lib, 41, 43) == (3, [(21, 23), (21, 23), (1, 2)] + [one] * 3)
    assert _dims(lib, 42, 43) == (3, [(22, 23), (22, 23), (1, 2)] + [one] * 3)
    assert _dims(lib, 43, 43) == (3, [(23, 23), (23, 23), (2, 2)] + [one] * 3)  # taps 43 22 11 6 3
    assert _dims(lib, 97, 131) == (4, [(77, 111), (77, 111), (29, 46), (5, 13), one, one])  # taps 97x131 49x66 25x33 13x17
    assert _dims(lib, 350, 340) == (6, [(330, 320), (330, 320), (155, 150), (68, 65), (24, 23), (2, 2)])
    assert _dims(lib, 533, 534)[1][0] == (513, 514)
    assert _dims(lib, 1080, 1920) == (6, [(1060, 1900), (1060, 1900), (520, 940), (250, 460), (115, 220), (48, 100)])
    for c in R.CASES:  # the replay's plan is the library's
        n, dims = _dims(lib, c.H, c.W)
        assert (dims, n) == (R.chain_dims(c.H, c.W)[0], sum(R.chain_dims(c.H, c.W)[1])), c
    mh = (C.c_int * 6)()
    assert lib.nqa_adists_chain_dims(64, 64, None, mh) == -1 and lib.nqa_adists_chain_dims(64, 64, mh, None) == -1
    assert b"adists_chain_dims: null pointer" in lib.nqa_last_error()
    for H, W in ((0, 64), (64, 0), (-1, 64), (64, -5)):
        assert _dims(lib, H, W)[0] == -1, (H, W)
        assert b"adists_chain_dims: bad size" in lib.nqa_last_error()
    assert _dims(lib, 1 << 12, 1 << 11)[0] == -1 and b"adists_chain_dims: image too large" in lib.nqa_last_error()


def test_chain_bytes(lib):
    for args in ((0, 64, 64), (-1, 64, 64), (1, 0, 64), (1, 64, -2)):
        assert lib.nqa_adists_chain_bytes(*args) == 0, args
    # 6 B accumulators of 40 bytes, B x 1024 blocks x 2 doubles of partial sums, B ones: each rounded up to 256 bytes
    up = lambda n: (n + 255) // 256 * 256
    for B in (1, 2, 3, 7):
        assert lib.nqa_adists_chain_bytes(B, 97, 131) == up(6 * B * 40) + up(B * 1024 * 16) + up(4 * B), B
    assert lib.nqa_adists_chain_bytes(2, 20, 20) == lib.nqa_adists_chain_bytes(2, 1080, 1920)  # (sized by the grid cap)


def _arr(first, null_at=None):
    a = (C.c_void_p * 6)(*[first + 0x1000 * k for k in range(6)])
    if null_at is not None:
        a[null_at] = None
    return a


def _chain(lib, B=2, H=40, W=56, ws=FAKE * 64, ws_bytes=None, d=FAKE * 65, m=FAKE * 66, **arrays):
    a = {"gamma": _arr(FAKE), "tw": _arr(2 * FAKE), "sw": _arr(3 * FAKE), "ps_prod": _arr(4 * FAKE)}
    a.update(arrays)
    if ws_bytes is None:
        ws_bytes = lib.nqa_adists_chain_bytes(max(B, 1), max(H, 1), max(W, 1))
    return lib.nqa_adists_chain(a["gamma"], a["tw"], a["sw"], B, H, W, ws, ws_bytes, a["ps_prod"], d, m, None)


def test_chain_refuses_bad_arguments(lib):
    for name in ("gamma", "tw", "sw", "ps_prod"):
        assert _chain(lib, **{name: None}) == -1, name
        assert b"adists_chain: null pointer" in lib.nqa_last_error()
        for k in (0, 3, 5):
            assert _chain(lib, **{name: _arr(FAKE, null_at=k)}) == -1, (name, k)
            assert b"adists_chain: null pointer (stage %d)" % k in lib.nqa_last_error()
    for kw in ({"ws": None}, {"d": None}):
        assert _chain(lib, **kw) == -1, kw
        assert b"adists_chain: null pointer" in lib.nqa_last_error()
    for kw in ({"B": 0}, {"B": -1}, {"H": 0}, {"W": -3}, {"H": -40, "W": -56}):
        assert _chain(lib, **kw) == -1, kw
        assert b"adists_chain: bad size" in lib.nqa_last_error()
    # nqa_adists_forward's frame limit: H * W * 64 floats reach 2^31 bytes at 2^23 pixels
    for kw in ({"H": 1 << 12, "W": 1 << 11}, {"H": 1 << 23, "W": 1}, {"H": 2897, "W": 2897}):
        assert _chain(lib, **kw) == -1, kw
        assert b"adists_chain: image too large" in lib.nqa_last_error()
    need = lib.nqa_adists_chain_bytes(2, 40, 56)
    for short in (0, 1, need - 1):
        assert _chain(lib, ws_bytes=short) == -3, short
        assert b"adists_chain: workspace" in lib.nqa_last_error()


def test_ops_refuse_what_the_kernels_cannot_take():
    from nerf_qa_amd import _lib, ops
    dims, _ = ops.adists_chain_dims(24, 25)
    assert dims == [(4, 5), (4, 5)] + [(1, 1)] * 4
    maps = [torch.rand((2,) + d) for d in dims]
    with pytest.raises(_lib.NqaError):
        ops.adists_chain(maps, maps, maps, 24, 25)  # CPU tensors
    with pytest.raises(_lib.NqaError):
        ops.adists_chain_dims(0, 25)
