"""CPU-side checks of the single-operator entry points in the mixed modes (include/nqa.h): the new boundary pool
nqa_l2pool_f16_to_split16 is exported, declared and validates its arguments on the host, and a mixed `prec` is no
longer an argument error of nqa_conv1_1 / nqa_conv1_fused / nqa_conv3x3_relu / nqa_l2pool -- shown through the refusals
that lie BEHIND the precision check (nothing here reaches a device: every call is refused on the host)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F16, F32S, F32M, F32M2, F32M4, F16W = 0, 2, 3, 4, 5, 6, 7
MIXED = (F32M, F32M2, F32M4, F16W)
P = 0x1000  # (never dereferenced)


@pytest.fixture(scope="module")
def lib():
    from nerf_qa_amd import build, _lib
    build.build()
    return _lib.lib()


def test_boundary_pool_exported_and_declared(lib):
    from nerf_qa_amd import _lib
    assert "nqa_l2pool_f16_to_split16" in _lib.EXPORTS and hasattr(lib, "nqa_l2pool_f16_to_split16")
    hdr = open(os.path.join(ROOT, "include", "nqa.h")).read()
    assert re.search(r"\bint\s+nqa_l2pool_f16_to_split16\s*\(", hdr)
    assert "pyramid entry points only" not in hdr
    assert lib.nqa_version() == 1  # adding a function is compatible


@pytest.mark.parametrize("args", [(None, 1, 4, 4, 64, P), (P, 1, 4, 4, 64, None)], ids=["null_in", "null_out"])
def test_boundary_pool_null_pointers(lib, args):
    assert lib.nqa_l2pool_f16_to_split16(*args, None) == -1
    assert b"null" in lib.nqa_last_error()


@pytest.mark.parametrize("n,h,w", [(0, 4, 4), (-1, 4, 4), (1, 0, 4), (1, 4, -3)])
def test_boundary_pool_bad_sizes(lib, n, h, w):
    assert lib.nqa_l2pool_f16_to_split16(P, n, h, w, 64, P, None) == -1
    assert b"non-positive" in lib.nqa_last_error()


@pytest.mark.parametrize("c", [0, -16, 8, 24, 100])
def test_boundary_pool_wants_whole_split16_records(lib, c):
    assert lib.nqa_l2pool_f16_to_split16(P, 1, 4, 4, c, P, None) == -2  # NQA_E_SHAPE
    assert b"multiple of 16" in lib.nqa_last_error()


def test_boundary_pool_32bit_offsets_by_the_records_it_writes(lib):
    # 1500 x 1500 x 256 channels: 1.15 GB of halves in, 2.3 GB of 4-byte records out
    assert lib.nqa_l2pool_f16_to_split16(P, 1, 1500, 1500, 256, P, None) == -1
    assert b"32-bit" in lib.nqa_last_error() and b"4 bytes" in lib.nqa_last_error()


@pytest.mark.parametrize("prec", MIXED)
def test_a_mixed_prec_passes_the_precision_check(lib, prec):
    # nqa_l2pool: behind the precision check sits the channel-count check (NQA_E_SHAPE)
    assert lib.nqa_l2pool(P, 1, 4, 4, 12, prec, P, None) == -2
    assert b"multiple of 8" in lib.nqa_last_error()
    # nqa_conv1_fused: the fused form exists only where the pyramid takes it
    assert lib.nqa_conv1_fused(P, 1, 16, 15, P, prec, P, None) == -2
    assert b"W >= 16" in lib.nqa_last_error()
    # nqa_conv1_1 / nqa_conv3x3_relu: behind it sits the 32-bit offset bound, which names the element size it used
    assert lib.nqa_conv1_1(P, 1, 4096, 4096, P, prec, P, None) == -1
    assert b"32-bit" in lib.nqa_last_error() and b"2 bytes" in lib.nqa_last_error()
    assert lib.nqa_conv3x3_relu(P, 1, 4096, 4096, 1, P, prec, P, None) == -1
    assert b"32-bit" in lib.nqa_last_error() and b"mixed" not in lib.nqa_last_error()
    # unknown ids and the entry points that take no mixed mode still refuse
    assert lib.nqa_conv3x3_relu(P, 1, 8, 8, 1, P, 99, P, None) == -1 and b"unknown prec" in lib.nqa_last_error()
    assert lib.nqa_nhwc_to_nchw_f32(P, 1, 8, 8, 64, prec, P, None) == -1 and b"mixed" in lib.nqa_last_error()


def test_offset_bound_uses_the_stage_s_own_element_size(lib):
    """The bound counts the widest map of the layer in the element size of the layer's own stage.  conv layer 7 (256 -> 512)
    is a float layer in f32m and f32m2: its 1100 x 1100 x 512-channel output is 1.24 GB as halves -- what the mixed id alone
    counted -- and 2.48 GB in 4-byte elements, refused.  conv3_3 (layer 6, 256 -> 256) on 1500 x 1500 is 1.15 GB as halves
    in f32m (passes the bound) and 2.3 GB as a float layer of f32m2 (refused)."""
    for prec in (F32M, F32M2):
        assert lib.nqa_conv3x3_relu(P, 1, 1100, 1100, 7, P, prec, P, None) == -1
        assert b"512 channels*4 bytes" in lib.nqa_last_error()
    # conv3_3 (layer 6, 256 -> 256): a 16-bit layer in f32m, a float one in f32m2
    assert lib.nqa_conv3x3_relu(P, 1, 1500, 1500, 6, P, F32M2, P, None) == -1
    assert b"256 channels*4 bytes" in lib.nqa_last_error()
    # (1500 x 1500 in f32m passes the bound and would launch: not called without a device; 2100 x 2100 names 2 bytes)
    assert lib.nqa_conv3x3_relu(P, 1, 2100, 2100, 6, P, F32M, P, None) == -1
    assert b"256 channels*2 bytes" in lib.nqa_last_error()
