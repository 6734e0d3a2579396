"""CPU-side checks of nqa_dists_stats_nhwc_grad_y_add (include/nqa.h, "DISTS and A-DISTS as ONE loss against a prepared
target"): declared in the header, exported by the library and bound by _lib.py; every argument its contract refuses is
refused on the host with its code and a message that names the function -- never a launch (no device is touched here,
the pointers below are fake).  NQA_E_SHAPE = -2: C not a power of two in 16..1024, H * W > 2^30; NQA_E_ARG = -1: a null
pointer (gy_inout included), B outside 1..65535, g_stride < C, a misaligned map; NQA_E_WORKSPACE = -3: a partials or
coefficient buffer one byte short."""
import os
import re

import pytest

NAME = "nqa_dists_stats_nhwc_grad_y_add"
WHO = b"dists_stats_nhwc_grad_y_add"
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "nqa.h")

P = [0x10000 + 0x1000 * i for i in range(7)]  # fake, 16-byte aligned device pointers: nothing below may dereference them


@pytest.fixture(scope="module")
def lib():
    from nerf_qa_amd import build, _lib
    build.build()
    return _lib.lib()


def _add(lib, tx=P[0], ty=P[1], B=2, H=8, W=8, C=64, part=P[2], part_bytes=1 << 30, g1=P[3], g2=P[4], stride=1475,
         coef=P[5], coef_bytes=1 << 30, gy=P[6]):
    return getattr(lib, NAME)(tx, ty, B, H, W, C, part, part_bytes, g1, g2, stride, coef, coef_bytes, gy, None)


def test_export_is_declared_bound_and_present(lib):
    from nerf_qa_amd import _lib, build
    text = open(HEADER).read()
    assert re.search(r"\b%s\(" % NAME, text)
    assert NAME in _lib.EXPORTS and getattr(lib, NAME) is not None
    assert len(_lib._SIGNATURES[NAME][1]) == 15  # backward_from's sixteen with gx / gy folded into one in/out pointer
    assert "NQA_K_COUNT = 7" in text  # its launches are counted under an existing timing class (NQA_K_STATS)
    assert "loss_stats_grad_y_add_kernel" in build.NO_SCRATCH
    res = build.json.load(open(build.RESOURCES))
    mine = [v for k, v in res.items() if "loss_stats_grad_y_add_kernel" in k]
    assert len(mine) == 1 and mine[0]["scratch"] == 0 and mine[0]["lds"] == 0


def test_null_pointers_batch_and_stride_are_bad_arguments(lib):
    for kw in ({"tx": None}, {"ty": None}, {"part": None}, {"g1": None}, {"g2": None}, {"coef": None}, {"gy": None},
               {"B": 0}, {"B": -1}, {"B": 65536}, {"H": 0}, {"W": -2}, {"stride": 63}):
        assert _add(lib, **kw) == -1, kw
        assert WHO + b": bad argument" in lib.nqa_last_error(), kw
    assert _add(lib, C=128, stride=127) == -1 and WHO + b": bad argument" in lib.nqa_last_error()  # g_stride = C - 1


def test_channel_counts_and_frame_sizes_the_kernel_does_not_take(lib):
    for c in (8, 48, 2048):
        assert _add(lib, C=c, stride=4096) == -2, c
        assert WHO + b": C %d must be a power of two" % c in lib.nqa_last_error()
    assert _add(lib, H=1 << 16, W=1 << 15) == -2
    assert WHO in lib.nqa_last_error() and b"2^30" in lib.nqa_last_error()


def test_misaligned_maps(lib):
    for kw in ({"tx": P[0] + 4}, {"ty": P[1] + 4}, {"gy": P[6] + 4}, {"gy": P[6] + 8}, {"coef": P[5] + 4},
               {"part": P[2] + 4}):
        assert _add(lib, **kw) == -1, kw
        assert WHO in lib.nqa_last_error() and b"aligned" in lib.nqa_last_error(), kw


def test_short_buffers(lib):
    need = lib.nqa_dists_stats_target_bytes(2, 8, 8, 64)
    assert need > 0
    for short in (need - 1, 0):
        assert _add(lib, part_bytes=short) == -3
        assert WHO + b": partials" in lib.nqa_last_error()
    need = lib.nqa_dists_stats_nhwc_backward_from_bytes(2, 64)
    assert need > 0
    for short in (need - 1, 0):
        assert _add(lib, part_bytes=lib.nqa_dists_stats_target_bytes(2, 8, 8, 64), coef_bytes=short) == -3
        assert WHO + b": coefficient buffer" in lib.nqa_last_error()
