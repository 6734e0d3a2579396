"""CPU-side checks of the prepared-target entry points (include/nqa.h, "DISTS as a loss against a PREPARED TARGET":
nqa_dists_stats_target and nqa_dists_stats_nhwc_backward_from with their _bytes functions): declared in the header,
exported by the library, bound by _lib.py; null pointers, non-positive sizes, a C the kernels do not take and short
buffers are refused on the host with a code and a message that names the function -- never a launch (no device is
touched here); and the two buffer sizes are the two parts of nqa_dists_stats_nhwc_backward's workspace, planned alike."""
import os
import re

import pytest

NEW = ("nqa_dists_stats_target_bytes", "nqa_dists_stats_target", "nqa_dists_stats_nhwc_backward_from_bytes",
       "nqa_dists_stats_nhwc_backward_from")
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "nqa.h")
SHAPES = ((33, 47), (40, 56), (96, 112), (1, 1))  # the frames of tests/test_gpu_target_loss.py

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
    assert "NQA_K_COUNT = 7" in text  # the new launches are counted under an existing timing class (NQA_K_STATS)


def _target(lib, tx=P[0], ty=P[1], B=2, H=8, W=8, C=64, part=P[2], part_bytes=1 << 30, s1=P[3], s2=P[4], stride=1475):
    return lib.nqa_dists_stats_target(tx, ty, B, H, W, C, part, part_bytes, s1, s2, stride, None)


def _from(lib, tx=P[0], ty=P[1], B=2, H=8, W=8, C=64, part=P[2], part_bytes=1 << 30, g1=P[3], g2=P[4], stride=1475,
          coef=P[5], coef_bytes=1 << 30, gx=P[6], gy=P[7]):
    return lib.nqa_dists_stats_nhwc_backward_from(tx, ty, B, H, W, C, part, part_bytes, g1, g2, stride, coef, coef_bytes,
                                                  gx, gy, None)


def _nblk(hw, c):
    """The sums kernel's blocks per pair, as csrc/nqa_loss_backward.hip plans them (loss_sums_nblk / loss_sums_ppb)."""
    cdiv = lambda a, b: (a + b - 1) // b
    pl = 256 // (c // 4)
    ppb = cdiv(cdiv(hw, min(cdiv(hw, pl * 8), 1024)), pl) * pl
    return cdiv(hw, ppb)


def test_buffer_sizes(lib):
    tb, fb, bb = (lib.nqa_dists_stats_target_bytes, lib.nqa_dists_stats_nhwc_backward_from_bytes,
                  lib.nqa_dists_stats_nhwc_backward_bytes)
    assert tb(0, 8, 8, 64) == 0 and tb(2, 0, 8, 64) == 0 and tb(2, 8, -1, 64) == 0
    assert tb(2, 8, 8, 8) == 0 and tb(2, 8, 8, 48) == 0 and tb(2, 8, 8, 2048) == 0  # C: a power of two in 16..1024
    assert tb(1, 1 << 16, 1 << 15, 64) == 0  # more than 2^30 pixels
    assert fb(0, 64) == 0 and fb(-1, 64) == 0 and fb(2, 8) == 0 and fb(2, 48) == 0 and fb(2, 2048) == 0
    for h, w in SHAPES + ((1080, 1920),):  # (1080p: the cap of 1024 blocks is in force)
        for c in (64, 128, 512):
            for b in (1, 2, 3):
                assert tb(b, h, w, c) == b * _nblk(h * w, c) * c * 5 * 8, (b, h, w, c)
                assert fb(b, c) == b * c * 6 * 8
                assert tb(b, h, w, c) + fb(b, c) == bb(b, h, w, c), (b, h, w, c)


def test_stats_target_refuses_bad_arguments(lib):
    for kw in ({"tx": None}, {"ty": None}, {"part": None}, {"s1": None}, {"s2": None}, {"B": 0}, {"B": -3}, {"B": 1 << 16},
               {"H": 0}, {"W": -2}, {"stride": 63}):
        assert _target(lib, **kw) == -1, kw
        assert b"dists_stats_target: bad argument" in lib.nqa_last_error()
    for c in (8, 48, 2048):
        assert _target(lib, C=c, stride=4096) == -2, c
        assert b"dists_stats_target: C %d must be a power of two" % c in lib.nqa_last_error()
    assert _target(lib, H=1 << 16, W=1 << 15) == -2
    assert b"dists_stats_target" in lib.nqa_last_error() and b"2^30" in lib.nqa_last_error()
    for kw in ({"tx": P[0] + 4}, {"ty": P[1] + 8}, {"part": P[2] + 4}):
        assert _target(lib, **kw) == -1, kw
        assert b"dists_stats_target" in lib.nqa_last_error() and b"aligned" in lib.nqa_last_error()
    need = lib.nqa_dists_stats_target_bytes(2, 8, 8, 64)
    assert need > 0
    for short in (need - 1, 0):
        assert _target(lib, part_bytes=short) == -3
        assert b"dists_stats_target: partials" in lib.nqa_last_error()


def test_backward_from_refuses_bad_arguments(lib):
    for kw in ({"tx": None}, {"ty": None}, {"part": None}, {"g1": None}, {"g2": None}, {"coef": None},
               {"gx": None, "gy": None}, {"B": 0}, {"B": 1 << 16}, {"H": 0}, {"H": -1}, {"W": 0}, {"stride": 63}):
        assert _from(lib, **kw) == -1, kw
        assert b"dists_stats_nhwc_backward_from: bad argument" in lib.nqa_last_error()
    for c in (8, 48, 2048):
        assert _from(lib, C=c, stride=4096) == -2, c
        assert b"dists_stats_nhwc_backward_from: C %d must be a power of two" % c in lib.nqa_last_error()
    assert _from(lib, H=1 << 16, W=1 << 15) == -2
    assert b"dists_stats_nhwc_backward_from" in lib.nqa_last_error() and b"2^30" in lib.nqa_last_error()
    for kw in ({"tx": P[0] + 4}, {"gy": P[7] + 8}, {"gx": P[6] + 4, "gy": None}, {"coef": P[5] + 4}, {"part": P[2] + 2}):
        assert _from(lib, **kw) == -1, kw
        assert b"dists_stats_nhwc_backward_from" in lib.nqa_last_error() and b"aligned" in lib.nqa_last_error()
    need = lib.nqa_dists_stats_target_bytes(2, 8, 8, 64)
    assert _from(lib, part_bytes=need - 1) == -3
    assert b"dists_stats_nhwc_backward_from: partials" in lib.nqa_last_error()
    need = lib.nqa_dists_stats_nhwc_backward_from_bytes(2, 64)
    assert need > 0 and _from(lib, coef_bytes=need - 1) == -3
    assert b"dists_stats_nhwc_backward_from: coefficient buffer" in lib.nqa_last_error()
    # one side alone is a valid request: it gets past every check above (and would launch), so only its refusals are
    # exercised here -- with the other pointer null the remaining one is still held to its alignment
    assert _from(lib, gx=None, gy=P[7] + 4) == -1 and b"aligned" in lib.nqa_last_error()
