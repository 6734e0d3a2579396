"""CPU-side checks of the generic-n entry points (include/nqa.h: nqa_window_moments_forward_n, nqa_window_moments_backward_n,
nqa_adists_ts_backward_bytes_n, nqa_adists_ts_backward_n) and of what Python builds on them: declared, exported, bound;
every refusal comes back from the host with its code and a message naming the function, never a launch (no device is
touched here: the pointers are fake).  ops raises ValueError for a bad window and NqaError for CPU tensors;
ADISTS(loss_head="hip") constructs, pickles and reads NQA_ADISTS_LOSS_HEAD; the head on CPU tensors does not notice
window_impl="hip"."""
import os
import pickle
import re

import pytest
import torch

NEW = ("nqa_window_moments_forward_n", "nqa_window_moments_backward_n", "nqa_adists_ts_backward_bytes_n",
       "nqa_adists_ts_backward_n")
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "nqa.h")
P = [0x10000 + 0x1000 * i for i in range(10)]  # fake, 16-byte aligned device pointers: nothing below may dereference them
E_ARG, E_SHAPE, E_WORKSPACE = -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    from nerf_qa_amd import build, _lib
    build.build()
    return _lib.lib()


def test_exports_are_declared_bound_and_listed(lib):
    from nerf_qa_amd import _lib, build
    text = open(HEADER).read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, text), name
        assert name in _lib.EXPORTS and getattr(lib, name) is not None, name
    assert "nqa_window_moments_n.hip" in build.SOURCES
    assert build.FILE_FLAGS["nqa_window_moments_n.hip"] == ["-fno-slp-vectorize"]
    for k in ("window_moments_n_fwd_kernel", "window_moments_n_bwd_kernel"):
        assert k in build.NO_SCRATCH
    import json
    res = json.load(open(os.path.join(os.path.dirname(build.__file__), "kernel_resources.json")))
    mine = {k: v for k, v in res.items() if "window_moments_n_" in k}
    assert len(mine) == 3 and all(v["scratch"] == 0 for v in mine.values()), mine  # fwd<pair>, fwd<x only>, bwd
    # the 21-tap kernels keep their entries
    assert sum("window_moments_fwd_kernel" in k or "window_moments_bwd_kernel" in k for k in res) == 3


def _fwd(lib, x=P[0], y=P[1], planes=6, H=40, W=56, window=7, out=P[2]):
    return lib.nqa_window_moments_forward_n(x, y, planes, H, W, window, out, None)


def _bwd(lib, x=P[0], y=P[1], planes=6, H=40, W=56, window=7, g=(P[2], P[3], P[4], P[5], P[6]), gx=P[7], gy=P[8]):
    return lib.nqa_window_moments_backward_n(x, y, planes, H, W, window, *g, gx, gy, None)


@pytest.mark.parametrize("call,who", [(_fwd, b"window_moments_forward_n"), (_bwd, b"window_moments_backward_n")])
def test_moments_refuse_bad_arguments(lib, call, who):
    for kw in ({"x": None}, {"planes": 0}, {"planes": -3}):
        assert call(lib, **kw) == E_ARG, kw
        assert who + b": bad argument" in lib.nqa_last_error()
    for win in (2, 0, -1, 64, 1 << 20):
        assert call(lib, window=win) == E_ARG, win
        err = lib.nqa_last_error()
        assert who in err and b"[3, 63]" in err and str(win).encode() in err
    for kw in ({"H": 6}, {"W": 6}, {"H": 0}, {"W": -1}, {"H": 62, "W": 100, "window": 63}, {"H": 20, "window": 21},
               {"H": 3, "W": 3, "window": 4}):
        assert call(lib, **kw) == E_SHAPE, kw
        n = kw.get("window", 7)
        assert who in lib.nqa_last_error() and b"%d x %d window" % (n, n) in lib.nqa_last_error()
    assert call(lib, H=1 << 16, W=(1 << 14) + 4) == E_SHAPE  # a plane of more than 2^30 pixels
    assert who in lib.nqa_last_error() and b"2^30" in lib.nqa_last_error()
    for kw in ({"x": P[0] + 4}, {"y": P[1] + 8}):
        assert call(lib, **kw) == E_ARG, kw
        assert who in lib.nqa_last_error() and b"aligned" in lib.nqa_last_error()
        # 16-byte accesses exist only where W % 4 == 0 (the too-large plane is checked AFTER the alignment: no launch)
        assert call(lib, H=1 << 24, W=84, **kw) == E_ARG and b"aligned" in lib.nqa_last_error()
        assert call(lib, H=1 << 24, W=85, **kw) == E_SHAPE, kw
        assert b"aligned" not in lib.nqa_last_error() and b"2^30" in lib.nqa_last_error()


def test_forward_and_backward_specifics(lib):
    assert _fwd(lib, out=None) == E_ARG and b"window_moments_forward_n: bad argument" in lib.nqa_last_error()
    assert _fwd(lib, out=P[2] + 12) == E_ARG and b"aligned" in lib.nqa_last_error()
    for kw in ({"gx": None, "gy": None}, {"y": None}, {"y": None, "gy": None},
               {"y": None, "gy": None, "g": (P[2], P[3], P[4], None, None)},
               {"y": None, "gy": None, "g": (P[2], None, P[4], None, P[6])}):
        assert _bwd(lib, **kw) == E_ARG, kw
        assert b"window_moments_backward_n: bad argument" in lib.nqa_last_error()
    for kw in ({"gx": P[7] + 8}, {"gy": P[8] + 4}, {"g": (P[2], P[3], P[4] + 4, P[5], P[6])},
               {"g": (None, None, None, None, P[6] + 8)}):
        assert _bwd(lib, **kw) == E_ARG, kw
        assert b"window_moments_backward_n" in lib.nqa_last_error() and b"aligned" in lib.nqa_last_error()


def _ts(lib, x=P[0], y=P[1], B=2, C=64, H=40, W=56, window=7, q=P[2], wgt=P[3], ctot=64, coff=0, ps=P[4], u=P[5], mask=1,
        nhwc=0, ws=P[6], ws_bytes=1 << 40, gy=P[7]):
    return lib.nqa_adists_ts_backward_n(x, y, B, C, H, W, window, q, wgt, ctot, coff, ps, u, mask, nhwc, ws, ws_bytes, gy,
                                        None)


def test_stage_backward_refuses_bad_arguments(lib):
    who = b"adists_ts_backward_n"
    for name in ("x", "y", "q", "wgt", "ps", "u", "ws", "gy"):
        assert _ts(lib, **{name: None}) == E_ARG, name
        assert who + b": bad argument (null pointer)" in lib.nqa_last_error()
    for win in (2, 64, -5):
        assert _ts(lib, window=win) == E_ARG
        assert who in lib.nqa_last_error() and b"[3, 63]" in lib.nqa_last_error()
    for kw in ({"B": 0}, {"C": 0}, {"H": 0}, {"W": -1}, {"ctot": 0}, {"coff": -1}, {"coff": 1}, {"B": 65536}):
        assert _ts(lib, **kw) == E_ARG, kw
        assert who in lib.nqa_last_error()
    assert _ts(lib, H=1 << 16, W=(1 << 14) + 4) == E_SHAPE and b"2^30" in lib.nqa_last_error()
    # an NHWC gradient of a WINDOWED stage needs C % 32 == 0; the same map under the window (global branch) does not
    assert _ts(lib, C=3, ctot=3, nhwc=1) == E_SHAPE and b"C % 32" in lib.nqa_last_error()
    assert _ts(lib, C=3, ctot=3, nhwc=1, H=6, ws_bytes=0) == E_WORKSPACE  # (global at n = 7: passes that check)
    assert _ts(lib, C=3, ctot=3, nhwc=1, H=20, window=21, ws_bytes=0) == E_WORKSPACE
    assert _ts(lib, C=3, ctot=3, nhwc=1, H=21, W=24, window=21) == E_SHAPE
    # alignment: the workspace always; the maps on a windowed stage with W % 4 == 0
    assert _ts(lib, ws=P[6] + 8) == E_ARG and b"aligned" in lib.nqa_last_error()
    for name in ("x", "y", "ps", "gy"):
        assert _ts(lib, **{name: P[0] + 4}) == E_ARG and b"aligned" in lib.nqa_last_error(), name
        assert _ts(lib, W=57, ws_bytes=0, **{name: P[0] + 4}) == E_WORKSPACE, name        # odd width: scalar path
        assert _ts(lib, H=6, ws_bytes=0, **{name: P[0] + 4}) == E_WORKSPACE, name         # global branch
    # ps is read in 16-byte pieces only where mh * mw is a multiple of 4 (always at 21): 35 x 50 is not
    assert _ts(lib, H=41, ps=P[4] + 8, ws_bytes=0) == E_WORKSPACE
    assert _ts(lib, H=41, x=P[0] + 8, ws_bytes=0) == E_ARG and b"aligned" in lib.nqa_last_error()
    need = lib.nqa_adists_ts_backward_bytes_n(2, 64, 40, 56, 7)
    assert _ts(lib, ws_bytes=need - 1) == E_WORKSPACE
    assert who in lib.nqa_last_error() and str(need).encode() in lib.nqa_last_error()


def test_bytes_query(lib):
    f = lib.nqa_adists_ts_backward_bytes_n
    assert f(2, 64, 40, 56, 21) == lib.nqa_adists_ts_backward_bytes(2, 64, 40, 56)
    for n in (3, 7, 12, 33, 40):
        sizes = [f(b, 64, 40, 56, n) for b in (1, 2, 3, 8)]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and len(set(sizes)) == 4, (n, sizes)
    assert f(2, 64, 40, 56, 7) > f(2, 64, 40, 56, 21) > f(2, 64, 40, 56, 33)  # more windows, more moments
    assert f(2, 64, 40, 56, 63) == 16 == f(2, 64, 6, 56, 7)  # the global branch keeps nothing (0 is the refusal)
    for args in ((0, 64, 40, 56, 7), (2, 0, 40, 56, 7), (2, 64, 0, 56, 7), (2, 64, 40, 56, 2), (2, 64, 40, 56, 64),
                 (65536, 64, 40, 56, 7), (2, 64, 1 << 16, (1 << 14) + 4, 7)):
        assert f(*args) == 0, args


def test_variant_bit_4096_is_its_own(lib):
    from nerf_qa_amd import ops
    assert ops.CONV_MOMENTS_GENERIC == 4096 != ops.CONV_WINDOW_GENERIC
    try:
        for v in (4096 + 1, 4096 + 2048 + 1, 4096 + 2048 + 8 + 1):
            assert lib.nqa_set_conv_variant(v) == 0, v
        assert lib.nqa_set_conv_variant(4096 + 3) == E_ARG and b"4099" in lib.nqa_last_error()
        assert lib.nqa_set_conv_variant(8192 + 1) == E_ARG
        assert lib.nqa_set_conv_variant(4096) == E_ARG and b"unknown variant 4096" in lib.nqa_last_error()  # as before
    finally:
        assert lib.nqa_set_conv_variant(ops.DEFAULT_CONV_VARIANT) == 0


def test_ops_refuse_bad_windows_and_cpu_tensors():
    from nerf_qa_amd import _lib, ops
    x = torch.rand(1, 2, 24, 24)
    g5 = [torch.rand(1, 2, 18, 18)] * 5
    for bad in (2, 64, 0, -7, 7.0, "7", None, True):
        with pytest.raises(ValueError, match=r"3\.\.63"):
            ops.window_moments(x, window=bad)
        with pytest.raises(ValueError, match=r"3\.\.63"):
            ops.window_moments_backward(x, x, g5, window=bad)
        with pytest.raises(ValueError, match=r"3\.\.63"):
            ops.adists_ts_backward(x, x, torch.rand(8, 1, 2), torch.rand(1, 2), torch.rand(1, 18, 18), torch.rand(1),
                                   mask=True, window=bad)
    for n in (7, 21):
        with pytest.raises(_lib.NqaError):
            ops.window_moments(x, window=n)
        with pytest.raises(_lib.NqaError):
            ops.window_moments(x, x, window=n)
        with pytest.raises(_lib.NqaError):
            ops.window_moments_backward(x, x, [torch.rand(1, 2, 25 - n, 25 - n)] * 5, window=n)
        with pytest.raises(_lib.NqaError):
            ops.adists_ts_backward(x, x, torch.rand(8, 1, 2), torch.rand(1, 2), torch.rand(1, 25 - n, 25 - n), torch.rand(1),
                                   mask=True, window=n)


def test_loss_head_hip_constructs_pickles_and_reads_the_env(monkeypatch):
    from nerf_qa_amd import autograd, ops
    from nerf_qa_amd.ADISTS import ADISTS
    import importlib
    A = importlib.import_module("nerf_qa_amd.ADISTS.ADISTS")
    assert A.LOSS_HEADS == ("auto", "torch", "hip") and A.DEFAULT_LOSS_HEAD == "auto"
    m = ADISTS(window_size=7, vgg16_path="synth:1234", loss_head="hip")
    assert m.loss_head == "hip" and m._window() == 7
    m2 = pickle.loads(pickle.dumps(m))
    assert m2.loss_head == "hip" and m2.window_size == 7
    with pytest.raises(ValueError, match="loss_head"):
        ADISTS(vgg16_path="synth:1234", loss_head="eager")
    monkeypatch.setenv("NQA_ADISTS_LOSS_HEAD", "hip")
    assert ADISTS(vgg16_path="synth:1234").loss_head == "hip"
    assert ADISTS(vgg16_path="synth:1234", loss_head="torch").loss_head == "torch"
    # a pickle from before the field existed takes the default (here: the environment's)
    state = m.__getstate__()
    state.pop("loss_head")
    old = ADISTS.__new__(ADISTS)
    old.__setstate__(state)
    assert old.loss_head == "hip"
    monkeypatch.delenv("NQA_ADISTS_LOSS_HEAD")
    old = ADISTS.__new__(ADISTS)
    old.__setstate__(state)
    assert old.loss_head == "auto"
    monkeypatch.setenv("NQA_ADISTS_LOSS_HEAD", "eager")
    with pytest.raises(ValueError, match="loss_head"):
        ADISTS(vgg16_path="synth:1234")
    # who may differentiate a prepared target at which window
    monkeypatch.delenv("NQA_ADISTS_LOSS_HEAD")
    autograd.check_target_window(m)
    autograd.check_target_window(ADISTS(vgg16_path="synth:1234"))
    for head_kind in ("auto", "torch"):
        with pytest.raises(ValueError, match=r"adists\(x, y\)") as e:
            autograd.check_target_window(ADISTS(window_size=7, vgg16_path="synth:1234", loss_head=head_kind))
        assert 'loss_head="hip"' in str(e.value)
    assert autograd._backward_window(m) == 7
    assert autograd._backward_window(ADISTS(window_size=7, vgg16_path="synth:1234")) == ops.WINDOW


def test_head_on_cpu_does_not_notice_window_impl_hip():
    """CPU tensors never reach the HIP moments: "hip" and "slices" are one arithmetic there, bit for bit."""
    from nerf_qa_amd.ADISTS import head
    gen = torch.Generator().manual_seed(5)
    dims = ((3, 24, 28), (64, 24, 28), (128, 12, 14), (256, 6, 7), (512, 3, 4), (512, 2, 2))
    for dtype, ws in ((torch.float32, 7), (torch.float64, 21), (torch.float32, 4)):
        fx, fy = ([torch.rand((2,) + d, generator=gen).sub_(0.3).clamp_(min=0).to(dtype).requires_grad_() for d in dims]
                  for _ in range(2))
        outs = []
        for impl in ("hip", "slices"):
            d = head.adists_d(fx, fy, ws, window_impl=impl)
            outs.append((d.detach(), torch.autograd.grad(d.sum(), fx[:2] + fy[:2])))
        assert torch.equal(outs[0][0], outs[1][0]), (dtype, ws)
        assert all(torch.equal(a, b) for a, b in zip(outs[0][1], outs[1][1])), (dtype, ws)
    assert all(torch.equal(a, b) for a, b in zip(head.texture_probabilities(fx, 4, "hip"), head.texture_probabilities(fx, 4)))
    with pytest.raises(ValueError, match="hip"):
        head.adists_d(fx, fy, 21, window_impl="conv")
