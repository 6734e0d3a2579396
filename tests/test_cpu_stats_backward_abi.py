"""CPU-side checks of the backward entry points of forward_from_feats (nqa_stats_backward_bytes,
nqa_dists_stats_nchw_backward): argument validation happens on the host, before anything touches a device."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def lib():
    from nerf_qa_amd import build, _lib
    build.build()
    return _lib.lib()


CHNS = (3, 64, 128, 256, 512, 512)


def _ints(v):
    return (C.c_int * 6)(*v)


def _ptrs(v):
    return (C.c_void_p * 6)(*v)


def test_backward_bytes(lib):
    cs = _ints(CHNS)
    assert lib.nqa_stats_backward_bytes(0, cs) == 0
    assert lib.nqa_stats_backward_bytes(-3, cs) == 0
    assert lib.nqa_stats_backward_bytes(2, None) == 0
    assert lib.nqa_stats_backward_bytes(2, _ints((3, 64, 0, 256, 512, 512))) == 0
    one = lib.nqa_stats_backward_bytes(1, cs)
    assert one >= 1475 * 6 * 8 and one % 256 == 0  # six doubles per (pair, channel) plane
    assert lib.nqa_stats_backward_bytes(4, cs) >= 4 * 1475 * 6 * 8


def _call(lib, B=2, fx=None, fy=None, C_=CHNS, H=(8, 8, 4, 2, 1, 1), W=(8, 8, 4, 2, 1, 1), scratch=0x1000,
          fwd_bytes=1 << 30, g1=0x2000, g2=0x3000, coef=0x4000, coef_bytes=1 << 30, gx=None, gy=None):
    fake = [0x10000 + 0x100 * k for k in range(6)]
    fx = _ptrs(fake) if fx is None else fx
    fy = _ptrs(fake) if fy is None else fy
    gx = _ptrs([None] * 6) if gx is None else gx
    gy = _ptrs([None] * 6) if gy is None else gy
    return lib.nqa_dists_stats_nchw_backward(fx, fy, B, _ints(C_), _ints(H), _ints(W), scratch, fwd_bytes, g1, g2, coef,
                                             coef_bytes, gx, gy, None)


def test_backward_refuses_null_arguments(lib):
    for kw in ({"scratch": None}, {"g1": None}, {"g2": None}, {"coef": None}, {"B": 0}):
        assert _call(lib, **kw) == -1, kw
        assert b"bad argument" in lib.nqa_last_error()
    assert lib.nqa_dists_stats_nchw_backward(None, None, 1, None, None, None, None, 0, None, None, None, 0, None, None,
                                             None) == -1
    fx = _ptrs([0x10000, 0x10100, None, 0x10300, 0x10400, 0x10500])
    assert _call(lib, fx=fx) == -1
    assert b"bad feature 2" in lib.nqa_last_error()
    assert _call(lib, H=(8, 8, 4, 2, 0, 1)) == -1
    assert b"bad feature 4" in lib.nqa_last_error()


def test_backward_refuses_short_buffers(lib):
    cs = _ints(CHNS)
    H, W = (8, 8, 4, 2, 1, 1), (8, 8, 4, 2, 1, 1)
    need_fwd = lib.nqa_stats_scratch_bytes(2, cs, _ints(H), _ints(W))
    need_coef = lib.nqa_stats_backward_bytes(2, cs)
    assert need_fwd > 0 and need_coef > 0
    assert _call(lib, fwd_bytes=64) == -3
    assert b"forward scratch 64 <" in lib.nqa_last_error()
    assert _call(lib, fwd_bytes=need_fwd, coef_bytes=need_coef - 8) == -3
    assert b"coefficient buffer" in lib.nqa_last_error()


def test_backward_refuses_planes_beyond_32_bit_offsets(lib):
    assert _call(lib, H=(1 << 16, 8, 4, 2, 1, 1), W=(1 << 15, 8, 4, 2, 1, 1)) == -2
    assert b"feature 0" in lib.nqa_last_error()
