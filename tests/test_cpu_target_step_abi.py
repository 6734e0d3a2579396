"""CPU-side checks of the prepared-target loss step at the C boundary (include/nqa.h, "the prepared-target loss step":
nqa_dists_target_step_bytes / _forward / _backward and nqa_dists_score_backward): declared in the header, exported by the
library, bound by _lib.py; the state's size is positive where the step runs, 0 where it does not, monotone in B and at
least what the step has to keep; and every refusal of the four calls is reached on the host, with its code and a message
that names the function -- never a launch (no device is touched here: the pointers below are made-up numbers)."""
import ctypes as C
import os
import re

import pytest

NEW = ("nqa_dists_target_step_bytes", "nqa_dists_target_step_forward", "nqa_dists_target_step_backward",
       "nqa_dists_score_backward")
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "nqa.h")
F32S, F16 = 3, 2  # NQA_PREC_F32S, NQA_PREC_F16: the two rungs of the gradient chain
RUNGS = (F32S, F16)
E_ARG, E_SHAPE, E_WORKSPACE = -1, -2, -3

P = [0x100000 + 0x1000 * i for i in range(40)]  # fake, 4096-byte aligned device pointers: nothing below may dereference them

CONV_COUT = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
CONV_STAGE = (0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4)
TAP_C = (64, 128, 256, 512, 512)


@pytest.fixture(scope="module")
def lib():
    from nerf_qa_amd import build, _lib
    build.build()
    return _lib.lib()


def _dims(h, w):
    d = [(h, w)]
    for _ in range(4):
        h, w = (h + 1) // 2, (w + 1) // 2
        d.append((h, w))
    return d


def _ptrs(values):
    return (C.c_void_p * len(values))(*values)


def _err(lib):
    return lib.nqa_last_error()


def test_exports_are_declared_bound_and_present(lib):
    from nerf_qa_amd import _lib
    text = open(HEADER).read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, text), name
        assert name in _lib.EXPORTS and getattr(lib, name) is not None, name
    assert "#define NQA_VERSION 1" in text and lib.nqa_version() == 1  # the ABI only grows
    assert "NQA_K_COUNT = 7" in text  # the step's launches are counted under the existing timing classes


def test_state_bytes(lib):
    nb = lib.nqa_dists_target_step_bytes
    for rung in RUNGS:
        for shape in ((1, 1, 1), (2, 33, 47), (1, 1080, 1920)):
            assert nb(*shape, rung) > 0, (shape, rung)
            assert nb(*shape, rung) % 256 == 0
        for shape in ((0, 8, 8), (-1, 8, 8), (2, 0, 8), (2, 8, 0), (2, -3, 8), (2, 8, -1), (1 << 16, 8, 8)):
            assert nb(*shape, rung) == 0, (shape, rung)
        sizes = [nb(b, 33, 47, rung) for b in (1, 2, 3, 4, 7, 8, 64)]
        assert sizes == sorted(sizes) and sizes[0] < sizes[-1]  # non-decreasing in B
    for rung in (-1, 0, 1, 4, 7, 99):  # every other precision id is no rung of the gradient chain
        assert nb(2, 33, 47, rung) == 0, rung
        assert b"dists_target_step_bytes: grad_prec" in _err(lib)
    assert nb(1, 4096, 4096, F32S) == 0 and b"2^31" in _err(lib)  # 4096 * 4096 * 64 floats: past the layers' 32-bit offsets
    assert nb(2, 33, 47, F16) <= nb(2, 33, 47, F32S)  # (the half chain's masked operand is half as large)


@pytest.mark.parametrize("b,h,w", [(1, 1, 1), (2, 33, 47), (2, 40, 56), (4, 256, 256), (1, 1080, 1920)])
def test_state_holds_at_least_what_the_step_keeps(lib, b, h, w):
    """The thirteen activations of y (4 bytes per element, float or split16) and the five taps' fp64 partials."""
    d = _dims(h, w)
    acts = sum(b * d[CONV_STAGE[l]][0] * d[CONV_STAGE[l]][1] * CONV_COUT[l] * 4 for l in range(13))
    parts = 0
    for k in range(5):
        n = lib.nqa_dists_stats_target_bytes(b, d[k][0], d[k][1], TAP_C[k])
        assert n > 0
        parts += n
    for rung in RUNGS:
        assert lib.nqa_dists_target_step_bytes(b, h, w, rung) >= acts + parts, (b, h, w, rung)


B, H, W = 2, 33, 47


def _forward(lib, x=P[0], taps=tuple(P[1:6]), y=P[6], b=B, h=H, w=W, packed=P[7], rung=F32S, state=P[8],
             state_bytes=1 << 40, s1=P[9], s2=P[10]):
    return lib.nqa_dists_target_step_forward(x, None if taps is None else _ptrs(taps), y, b, h, w, packed, rung, state,
                                             state_bytes, s1, s2, None)


def _backward(lib, x=P[0], taps=tuple(P[1:6]), y=P[6], b=B, h=H, w=W, g1=P[9], g2=P[10], layers=tuple(P[11:23]), w0=P[23],
              rung=F32S, state=P[8], state_bytes=1 << 40, gy=P[24]):
    return lib.nqa_dists_target_step_backward(x, None if taps is None else _ptrs(taps), y, b, h, w, g1, g2,
                                              None if layers is None else _ptrs(layers), w0, rung, state, state_bytes, gy, None)


def _without(values, i):
    return tuple(None if j == i else v for j, v in enumerate(values))


def _shifted(values, i, by):
    return tuple(v + by if j == i else v for j, v in enumerate(values))


def _common_refusals(lib, call, who):
    """What the forward and the backward refuse alike."""
    for kw in [{"x": None}, {"y": None}, {"state": None}, {"taps": None}] + [{"taps": _without(P[1:6], k)} for k in range(5)]:
        assert call(lib, **kw) == E_ARG, kw
        assert who + b": null pointer" in _err(lib), _err(lib)
    for kw in ({"b": 0}, {"b": -2}, {"h": 0}, {"h": -1}, {"w": 0}, {"w": -7}, {"b": 1 << 16}):
        assert call(lib, **kw) == E_ARG, kw
        assert who + b": non-positive size or more than 65535 pairs" in _err(lib), _err(lib)
    for rung in (-1, 0, 1, 4, 7):
        assert call(lib, rung=rung) == E_ARG
        assert who + b": grad_prec %d is neither" % rung in _err(lib), _err(lib)
    assert call(lib, b=1, h=4096, w=4096) == E_SHAPE
    assert who in _err(lib) and b"2^31 bytes" in _err(lib)
    assert call(lib, b=40000, h=2048, w=2048) == E_SHAPE
    assert who in _err(lib) and b"2^36" in _err(lib)
    for kw in [{"x": P[0] + 2}, {"y": P[6] + 1}, {"state": P[8] + 128}, {"state": P[8] + 16}] + \
              [{"taps": _shifted(P[1:6], k, 4)} for k in range(5)]:
        assert call(lib, **kw) == E_ARG, kw
        assert who + b": misaligned buffer" in _err(lib), _err(lib)
    for rung in RUNGS:
        need = lib.nqa_dists_target_step_bytes(B, H, W, rung)
        assert need > 0
        for short in (need - 1, need // 2, 0):
            assert call(lib, rung=rung, state_bytes=short) == E_WORKSPACE
            assert who + b": state %d < %d bytes" % (short, need) in _err(lib), _err(lib)
    # the f32s state is the larger one: a state sized for the half chain is short for it
    assert call(lib, rung=F32S, state_bytes=lib.nqa_dists_target_step_bytes(B, H, W, F16)) == E_WORKSPACE
    # the order of the checks: a null pointer before a bad size, a bad size before a bad shape, the shape before
    # alignment, alignment before the state's size
    assert call(lib, x=None, b=0) == E_ARG and b"null pointer" in _err(lib)
    assert call(lib, b=0, h=4096, w=4096) == E_ARG and b"non-positive" in _err(lib)
    assert call(lib, b=1, h=4096, w=4096, state=P[8] + 4) == E_SHAPE
    assert call(lib, state=P[8] + 4, state_bytes=0) == E_ARG and b"misaligned" in _err(lib)


def test_forward_refuses_bad_arguments(lib):
    who = b"dists_target_step_forward"
    _common_refusals(lib, _forward, who)
    for kw in ({"packed": None}, {"s1": None}, {"s2": None}):
        assert _forward(lib, **kw) == E_ARG, kw
        assert who + b": null pointer" in _err(lib)
    for kw in ({"packed": P[7] + 8}, {"s1": P[9] + 2}, {"s2": P[10] + 3}):
        assert _forward(lib, **kw) == E_ARG, kw
        assert who + b": misaligned buffer" in _err(lib)


def test_backward_refuses_bad_arguments(lib):
    who = b"dists_target_step_backward"
    _common_refusals(lib, _backward, who)
    for kw in [{"g1": None}, {"g2": None}, {"w0": None}, {"gy": None}, {"layers": None}] + \
              [{"layers": _without(P[11:23], l)} for l in range(12)]:
        assert _backward(lib, **kw) == E_ARG, kw
        assert who + b": null pointer" in _err(lib)
    for kw in [{"g1": P[9] + 2}, {"g2": P[10] + 1}, {"w0": P[23] + 2}, {"gy": P[24] + 3}] + \
              [{"layers": _shifted(P[11:23], l, 8)} for l in range(12)]:
        assert _backward(lib, **kw) == E_ARG, kw
        assert who + b": misaligned buffer" in _err(lib)


def test_score_backward_refuses_bad_arguments(lib):
    def call(alpha=P[0], beta=P[1], g=P[2], b=3, g1=P[3], g2=P[4]):
        return lib.nqa_dists_score_backward(alpha, beta, g, b, g1, g2, None)

    for kw in ({"alpha": None}, {"beta": None}, {"g": None}, {"g1": None}, {"g2": None}):
        assert call(**kw) == E_ARG, kw
        assert b"dists_score_backward: null pointer" in _err(lib)
    for b in (0, -1):
        assert call(b=b) == E_ARG
        assert b"dists_score_backward: non-positive B=%d" % b in _err(lib)
    for kw in ({"alpha": P[0] + 1}, {"beta": P[1] + 2}, {"g": P[2] + 3}, {"g1": P[3] + 2}, {"g2": P[4] + 1}):
        assert call(**kw) == E_ARG, kw
        assert b"dists_score_backward: misaligned buffer" in _err(lib)
