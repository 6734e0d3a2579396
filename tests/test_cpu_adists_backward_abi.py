"""CPU-side checks of the one-stage A-DISTS backward entry (include/nqa.h: nqa_adists_ts_backward and
nqa_adists_ts_backward_bytes): declared in the header, exported by the library, bound by _lib.py, built from
csrc/nqa_adists_backward.hip, and every refusal happens on the host -- an error code and a message naming the function,
never a launch (no device is touched here; the pointers are fake)."""
import os
import re

import pytest
import torch

NEW = ("nqa_adists_ts_backward", "nqa_adists_ts_backward_bytes")
KERNELS = ("adists_ts_coef_kernel", "adists_ts_dot_kernel", "adists_ts_fold_kernel", "adists_ts_apply_kernel",
           "adists_ts_apply_nhwc_kernel", "adists_ts_global_kernel")
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "nqa.h")

P = [0x10000 + 0x1000 * i for i in range(10)]  # fake, 16-byte aligned device pointers: nothing below may dereference them
BIG = 1 << 40  # a workspace size no stage below needs more than


@pytest.fixture(scope="module")
def lib():
    from nerf_qa_amd import build, _lib
    build.build()
    return _lib.lib()


def _call(lib, x=P[0], y=P[1], B=2, C=64, H=40, W=56, q=P[2], wgt=P[3], ctot=None, coff=0, ps=P[4], u=P[5], mask=1,
          nhwc=0, ws=P[6], ws_bytes=0, gy=P[7]):
    """Every call here ends in a refusal: the default workspace size 0 is short for every size the entry accepts."""
    return lib.nqa_adists_ts_backward(x, y, B, C, H, W, q, wgt, C if ctot is None else ctot, coff, ps, u, mask, nhwc, ws,
                                      ws_bytes, gy, None)


def test_exports_are_declared_bound_and_built(lib):
    from nerf_qa_amd import _lib, build
    text = open(HEADER).read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, text), name
        assert name in _lib.EXPORTS and getattr(lib, name) is not None, name
    assert "NQA_K_COUNT = 7" in text  # the new launches are counted under NQA_K_ADISTS
    assert "nqa_adists_backward.hip" in build.SOURCES
    for k in KERNELS:
        assert k in build.NO_SCRATCH, k
    src = open(os.path.join(build.CSRC, "nqa_adists_backward.hip")).read()
    for k in KERNELS:
        assert re.search(r"void %s\(" % k, src), k


def test_null_pointers_are_refused(lib):
    for name in ("x", "y", "q", "wgt", "ps", "u", "ws", "gy"):
        assert _call(lib, ws_bytes=BIG, **{name: None}) == -1, name
        assert b"adists_ts_backward: bad argument (null pointer)" in lib.nqa_last_error()


def test_bad_sizes_are_refused(lib):
    for kw in ({"B": 0}, {"B": -1}, {"C": 0}, {"H": 0}, {"W": -3}, {"ctot": 0}, {"coff": -1}, {"ctot": 64, "coff": 1},
               {"ctot": 1475, "coff": 1475 - 63}, {"B": 65536}):
        assert _call(lib, ws_bytes=BIG, **kw) == -1, kw
        assert b"adists_ts_backward: bad argument" in lib.nqa_last_error()
    # plane-size limits, as the window-moments entries have them
    for kw in ({"H": 1 << 16, "W": (1 << 14) + 4}, {"H": (1 << 20) + 1, "W": 21}, {"B": 1, "C": 3, "H": 1 << 24, "W": 85}):
        assert _call(lib, ws_bytes=BIG, **kw) == -2, kw
        assert b"adists_ts_backward" in lib.nqa_last_error() and b"2^30" in lib.nqa_last_error()
    assert _call(lib, ws_bytes=BIG, B=65535, C=512, H=1 << 10, W=1 << 10) == -2  # more blocks than one launch takes
    assert b"adists_ts_backward" in lib.nqa_last_error() and b"2^31" in lib.nqa_last_error()
    assert _call(lib, ws_bytes=BIG, C=3, nhwc=1) == -2  # the NHWC tile kernel works on groups of 32 channels
    assert b"adists_ts_backward" in lib.nqa_last_error() and b"C % 32" in lib.nqa_last_error()


def test_short_workspace_is_refused_and_bytes_is_zero_for_refused_sizes(lib):
    for b, c, h, w in ((2, 64, 40, 56), (1, 3, 21, 21), (1, 64, 22, 37), (2, 512, 13, 17), (1, 512, 3, 4)):
        need = lib.nqa_adists_ts_backward_bytes(b, c, h, w)
        assert need >= 16 and need % 16 == 0, (b, c, h, w)
        if h >= 21 and w >= 21:  # five moment maps, P, and at least one fp64 partial and one fp64 scalar per plane
            assert need >= 4 * b * c * (5 * (h - 20) * (w - 20) + h * w) + 16 * b * c
        for short in (0, need - 1):
            assert _call(lib, B=b, C=c, H=h, W=w, ws_bytes=short) == -3, (b, c, h, w, short)
            assert b"adists_ts_backward: workspace" in lib.nqa_last_error()
    for args in ((0, 64, 40, 56), (2, 0, 40, 56), (2, 64, 0, 56), (2, 64, 40, -1), (65536, 64, 40, 56),
                 (1, 3, 1 << 16, (1 << 14) + 4), (65535, 512, 1 << 10, 1 << 10)):
        assert lib.nqa_adists_ts_backward_bytes(*args) == 0, args


def test_alignment_rule_of_the_window_kernels(lib):
    """Rows move as 16-byte accesses only on a windowed stage with W % 4 == 0; the workspace holds doubles and is always
    asked to be aligned.  The workspace size is checked LAST, so an aligned call with a short one ends there (-3) and
    nothing is ever launched on the fake pointers."""
    for kw in ({"x": P[0] + 4}, {"y": P[1] + 8}, {"ps": P[4] + 12}, {"gy": P[7] + 4}):
        assert _call(lib, **kw) == -1, kw
        assert b"adists_ts_backward" in lib.nqa_last_error() and b"aligned" in lib.nqa_last_error()
        assert _call(lib, W=57, **kw) == -3, kw            # no 16-byte access at this width
        assert _call(lib, H=16, W=16, **kw) == -3, kw      # nor in the global branch
    for kw in ({}, {"W": 57}, {"H": 16, "W": 16}):
        assert _call(lib, ws=P[6] + 8, **kw) == -1, kw
        assert b"aligned" in lib.nqa_last_error()
    for kw in ({"q": P[2] + 4}, {"wgt": P[3] + 4}, {"u": P[5] + 4}):  # scalars per channel and pair: floats
        assert _call(lib, **kw) == -3, kw


def test_op_refuses_cpu_tensors():
    from nerf_qa_amd import _lib, ops
    x = torch.rand(1, 3, 24, 24)
    q, wgt, ps, u = torch.rand(8, 1, 3), torch.rand(1, 3), torch.rand(1, 4, 4), torch.rand(1)
    with pytest.raises(_lib.NqaError):
        ops.adists_ts_backward(x, x, q, wgt, ps, u, mask=False)


def test_loss_head_option_and_old_pickles(monkeypatch):
    import pickle
    from nerf_qa_amd import autograd
    from nerf_qa_amd.ADISTS import ADISTS
    assert hasattr(autograd, "AdistsLossY") and hasattr(autograd, "adists_backward_y")
    monkeypatch.delenv("NQA_ADISTS_LOSS_HEAD", raising=False)
    m = ADISTS(vgg16_path="synth:1234")
    assert m.loss_head in ("auto", "torch")
    assert ADISTS(vgg16_path="synth:1234", loss_head="torch").loss_head == "torch"
    with pytest.raises(ValueError):
        ADISTS(vgg16_path="synth:1234", loss_head="eager")
    monkeypatch.setenv("NQA_ADISTS_LOSS_HEAD", "torch")
    assert ADISTS(vgg16_path="synth:1234").loss_head == "torch"
    monkeypatch.delenv("NQA_ADISTS_LOSS_HEAD")
    state = m.__getstate__()
    state.pop("loss_head")  # a module pickled before the option existed
    old = ADISTS.__new__(ADISTS)
    old.__setstate__(state)
    assert old.loss_head == m.loss_head
    assert pickle.loads(pickle.dumps(ADISTS(vgg16_path="synth:1234", loss_head="torch"))).loss_head == "torch"
