"""CPU-side checks of the windowed-moments entry points (include/nqa.h: nqa_window_moments_forward and
nqa_window_moments_backward): they are declared in the header, exported by the library, bound by _lib.py, and refuse null
pointers and bad sizes on the host -- an error code and a message naming the function, never a launch (no device is
touched here).  The kernels keep everything they need in LDS and registers, so there is no workspace argument and no
`_bytes` query: a short workspace cannot be passed.  The head on CPU tensors must not notice the new code path."""
import os
import re

import pytest
import torch

NEW = ("nqa_window_moments_forward", "nqa_window_moments_backward")
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "nqa.h")

P = [0x10000 + 0x1000 * i for i in range(10)]  # fake, 16-byte aligned device pointers: nothing below may dereference them


@pytest.fixture(scope="module")
def lib():
    from nerf_qa_amd import build, _lib
    build.build()
    return _lib.lib()


def test_exports_are_declared_bound_and_present(lib):
    from nerf_qa_amd import _lib, build
    text = open(HEADER).read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, text), name
        assert name in _lib.EXPORTS and getattr(lib, name) is not None, name
    assert "NQA_K_COUNT = 7" in text  # the new launches are counted under NQA_K_ADISTS
    assert "nqa_window_moments.hip" in build.SOURCES
    assert build.FILE_FLAGS["nqa_window_moments.hip"] == ["-fno-slp-vectorize"]
    for k in ("window_moments_fwd_kernel", "window_moments_bwd_kernel"):
        assert k in build.NO_SCRATCH


def _fwd(lib, x=P[0], y=P[1], planes=6, H=40, W=56, out=P[2]):
    return lib.nqa_window_moments_forward(x, y, planes, H, W, out, None)


def _bwd(lib, x=P[0], y=P[1], planes=6, H=40, W=56, g=(P[2], P[3], P[4], P[5], P[6]), gx=P[7], gy=P[8]):
    return lib.nqa_window_moments_backward(x, y, planes, H, W, *g, gx, gy, None)


def test_forward_refuses_bad_arguments(lib):
    for kw in ({"x": None}, {"out": None}, {"planes": 0}, {"planes": -3}):
        assert _fwd(lib, **kw) == -1, kw
        assert b"window_moments_forward: bad argument" in lib.nqa_last_error()
    for kw in ({"H": 20}, {"W": 20}, {"H": 0}, {"W": -1}, {"H": 20, "W": 20}):
        assert _fwd(lib, **kw) == -2, kw
        assert b"window_moments_forward" in lib.nqa_last_error() and b"21 x 21 window" in lib.nqa_last_error()
    assert _fwd(lib, H=1 << 16, W=(1 << 14) + 4) == -2  # a plane of more than 2^30 pixels
    assert b"window_moments_forward" in lib.nqa_last_error() and b"2^30" in lib.nqa_last_error()
    for kw in ({"x": P[0] + 4}, {"y": P[1] + 8}, {"out": P[2] + 12}):
        assert _fwd(lib, **kw) == -1, kw
        assert b"window_moments_forward" in lib.nqa_last_error() and b"aligned" in lib.nqa_last_error()
        # 16-byte accesses exist only where W % 4 == 0: with W = 85 the same pointer is not refused for its alignment
        # (the plane is made too large, which is checked AFTER the alignment, so nothing is launched here)
        assert _fwd(lib, H=1 << 24, W=84, **kw) == -1 and b"aligned" in lib.nqa_last_error()
        assert _fwd(lib, H=1 << 24, W=85, **kw) == -2, kw
        assert b"aligned" not in lib.nqa_last_error() and b"2^30" in lib.nqa_last_error()


def test_backward_refuses_bad_arguments(lib):
    none5 = (None,) * 5
    for kw in ({"x": None}, {"gx": None, "gy": None}, {"planes": 0}, {"planes": -1},
               {"y": None}, {"y": None, "gy": None}, {"y": None, "gy": None, "g": (P[2], P[3], P[4], None, None)},
               {"y": None, "gy": None, "g": (P[2], None, P[4], None, P[6])}):
        assert _bwd(lib, **kw) == -1, kw
        assert b"window_moments_backward: bad argument" in lib.nqa_last_error()
    for kw in ({"H": 20}, {"W": 20}, {"H": 1, "W": 1}, {"H": 20, "g": none5}):
        assert _bwd(lib, **kw) == -2, kw
        assert b"window_moments_backward" in lib.nqa_last_error() and b"21 x 21 window" in lib.nqa_last_error()
    assert _bwd(lib, H=1 << 15, W=(1 << 15) + 4) == -2
    assert b"window_moments_backward" in lib.nqa_last_error() and b"2^30" in lib.nqa_last_error()
    for kw in ({"x": P[0] + 4}, {"y": P[1] + 4}, {"gx": P[7] + 8}, {"gy": P[8] + 4},
               {"g": (P[2], P[3], P[4] + 4, P[5], P[6])}, {"g": (None, None, None, None, P[6] + 8)}):
        assert _bwd(lib, **kw) == -1, kw
        assert b"window_moments_backward" in lib.nqa_last_error() and b"aligned" in lib.nqa_last_error()
        assert _bwd(lib, H=1 << 24, W=84, **kw) == -1 and b"aligned" in lib.nqa_last_error()
        assert _bwd(lib, H=1 << 24, W=85, **kw) == -2, kw  # (no 16-byte access at this width: see the forward's case)
        assert b"aligned" not in lib.nqa_last_error() and b"2^30" in lib.nqa_last_error()


def test_ops_refuse_cpu_tensors():
    from nerf_qa_amd import _lib, ops
    x = torch.rand(1, 2, 24, 24)
    with pytest.raises(_lib.NqaError):
        ops.window_moments(x)
    with pytest.raises(_lib.NqaError):
        ops.window_moments(x, x)
    with pytest.raises(_lib.NqaError):
        ops.window_moments_backward(x, x, [torch.rand(1, 2, 4, 4)] * 5)


def test_head_on_cpu_is_the_slice_form():
    """CPU tensors (and float64, and other window sizes) never reach the HIP moments: "auto" and "slices" are one
    arithmetic there, bit for bit, values and gradients."""
    from nerf_qa_amd.ADISTS import head
    gen = torch.Generator().manual_seed(5)
    dims = ((3, 48, 56), (64, 48, 56), (128, 24, 28), (256, 12, 14), (512, 6, 7), (512, 3, 4))

    def feats(dtype):
        return [torch.rand((2,) + d, generator=gen).sub_(0.3).clamp_(min=0).to(dtype).requires_grad_() for d in dims]

    for dtype, ws in ((torch.float32, 21), (torch.float64, 21), (torch.float32, 11)):
        fx, fy = feats(dtype), feats(dtype)
        outs = []
        for impl in ("auto", "slices"):
            d = head.adists_d(fx, fy, ws, window_impl=impl)
            g = torch.autograd.grad(d.sum(), fx[:2] + fy[:2])
            outs.append((d.detach(), g))
        assert torch.equal(outs[0][0], outs[1][0]), (dtype, ws)
        for a, b in zip(outs[0][1], outs[1][1]):
            assert torch.equal(a, b), (dtype, ws)
    with pytest.raises(ValueError):
        head.adists_d(fx, fy, 21, window_impl="conv")
