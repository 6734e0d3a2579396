"""CPU-side checks of the A-DISTS entry points that take an explicit window size (include/nqa.h: the `_n` forms of the
workspace sizes, the forwards, the single-stage window pass and the chain, for pairs and for groups): declared in the
header, exported by the library, bound by _lib.py; the window-21 forms return what the old names return; map dims are
H-n+1 x W-n+1 or 1 x 1; and every refusal happens on the host -- an error code and a message naming the function and,
for the window, its range, never a launch (the pointers below are fakes that nothing may dereference, and no device is
touched)."""
import ctypes as C
import os
import re

import pytest
import torch

NEW = ("nqa_adists_workspace_bytes_n", "nqa_adists_forward_n", "nqa_adists_forward_map_n", "nqa_adists_dists_forward_n",
       "nqa_adists_group_workspace_bytes_n", "nqa_adists_forward_group_n", "nqa_adists_window_stage_n",
       "nqa_adists_window_stage_group_n", "nqa_adists_chain_dims_n", "nqa_adists_chain_bytes_n", "nqa_adists_chain_n",
       "nqa_adists_chain_group_bytes_n", "nqa_adists_chain_group_n")
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "nqa.h")

P = [0x10000 + 0x1000 * i for i in range(10)]  # fake device pointers
BAD_WINDOWS = (2, 64, 0, -1)
RANGE = b"outside [3, 63]"
SHAPES = [(h, w) for h in (1, 20, 21, 40, 97, 350) for w in (1, 21, 43, 131, 340)] + [(1080, 1920)]


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
        assert re.search(r"\b%s\([^)]*\bint window\b" % name, text), name  # the window is an explicit argument
        assert name in _lib.EXPORTS and getattr(lib, name) is not None, name
    assert (ops.WINDOW_MIN, ops.WINDOW_MAX, ops.WINDOW) == (3, 63, 21)


def _dims(lib, H, W, n):
    mh, mw = (C.c_int * 6)(), (C.c_int * 6)()
    k = lib.nqa_adists_chain_dims_n(H, W, n, mh, mw)
    return k, list(zip(mh, mw))


def _dims21(lib, H, W):
    mh, mw = (C.c_int * 6)(), (C.c_int * 6)()
    k = lib.nqa_adists_chain_dims(H, W, mh, mw)
    return k, list(zip(mh, mw))


def test_window_21_forms_are_the_old_names(lib):
    for H, W in SHAPES:
        assert _dims(lib, H, W, 21) == _dims21(lib, H, W), (H, W)
        for B in (1, 3):
            assert lib.nqa_adists_chain_bytes_n(B, H, W, 21) == lib.nqa_adists_chain_bytes(B, H, W) > 0
            assert lib.nqa_adists_chain_group_bytes_n(B, 2, H, W, 21) == lib.nqa_adists_chain_group_bytes(B, 2, H, W) > 0
            for prec in (0, 1, 2, 3):
                assert lib.nqa_adists_workspace_bytes_n(B, H, W, 21, prec) == lib.nqa_adists_workspace_bytes(B, H, W, prec) > 0
                assert (lib.nqa_adists_group_workspace_bytes_n(B, 2, H, W, 21, prec)
                        == lib.nqa_adists_group_workspace_bytes(B, 2, H, W, prec) > 0)


def test_dims_are_valid_windows_or_one_by_one(lib):
    from nerf_qa_amd import ops
    for n in (3, 4, 7, 12, 21, 33, 62, 63):
        for H, W in SHAPES:
            h, w, want, nwin = H, W, [], 0
            for k in range(6):
                if k >= 2:
                    h, w = (h + 1) // 2, (w + 1) // 2
                windowed = h >= n and w >= n
                nwin += windowed
                want.append((h - n + 1, w - n + 1) if windowed else (1, 1))
            got = _dims(lib, H, W, n)
            assert got == (nwin, want), (n, H, W)
            assert ops.adists_chain_dims(H, W, n) == (want, got[0])
    # a smaller window leaves larger maps and a larger workspace; the plan's other areas do not depend on it
    small, big = (lib.nqa_adists_workspace_bytes_n(2, 97, 131, n, 0) for n in (3, 63))
    assert small > lib.nqa_adists_workspace_bytes_n(2, 97, 131, 21, 0) > big > 0
    assert _dims(lib, 63, 63, 63) == (2, [(1, 1)] * 6) and _dims(lib, 62, 63, 63) == (0, [(1, 1)] * 6)
    assert _dims(lib, 3, 3, 3) == (2, [(1, 1)] * 6) and _dims(lib, 40, 40, 5)[1][:4] == [(36, 36), (36, 36), (16, 16), (6, 6)]


def _stage(lib, fx=P[0], fy=P[1], B=2, H=40, W=56, n=7, C_=64, prec=0, q=P[2], wgt=P[3], strip=0, gamma=P[4], tw=P[5],
           sw=P[6]):
    return lib.nqa_adists_window_stage_n(fx, fy, B, H, W, n, C_, prec, q, wgt, strip, gamma, tw, sw, None)


def _stage_group(lib, fx=P[0], fy=P[1], R=2, K=3, H=40, W=56, n=7, C_=64, prec=0, q=P[2], wgt=P[3], strip=0, gamma=P[4],
                 tw=P[5], sw=P[6]):
    return lib.nqa_adists_window_stage_group_n(fx, fy, R, K, H, W, n, C_, prec, q, wgt, strip, gamma, tw, sw, None)


def _arr(first):
    return (C.c_void_p * 6)(*[first + 0x1000 * k for k in range(6)])


def test_bad_windows_are_refused_with_the_range(lib):
    mh = (C.c_int * 6)()
    big = 1 << 40
    for n in BAD_WINDOWS:
        calls = {
            "adists_window_stage": lambda: _stage(lib, n=n),
            "adists_window_stage_group": lambda: _stage_group(lib, n=n),
            "adists_forward": lambda: lib.nqa_adists_forward_n(P[0], P[1], 2, 40, 56, n, P[2], 0, P[3], big, P[4], None),
            "adists_forward#map": lambda: lib.nqa_adists_forward_map_n(P[0], P[1], 2, 40, 56, n, P[2], 0, P[3], big, P[4],
                                                                         P[5], None),
            "adists_forward#dists": lambda: lib.nqa_adists_dists_forward_n(P[0], P[1], 2, 40, 56, n, P[2], 0, P[3], big, P[4],
                                                                           P[5], P[6], None, None),
            "adists_forward_group": lambda: lib.nqa_adists_forward_group_n(P[0], P[1], 2, 3, 40, 56, n, P[2], 0, P[3], big,
                                                                           P[4], None, None, None),
            "adists_chain_dims": lambda: lib.nqa_adists_chain_dims_n(40, 56, n, mh, mh),
            "adists_chain": lambda: lib.nqa_adists_chain_n(_arr(P[0]), _arr(P[1]), _arr(P[2]), 2, 40, 56, n, P[3], big,
                                                           _arr(P[4]), P[5], None, None),
            "adists_chain_group": lambda: lib.nqa_adists_chain_group_n(_arr(P[0]), _arr(P[1]), _arr(P[2]), 2, 3, 40, 56, n,
                                                                       P[3], big, _arr(P[4]), P[5], None),
        }
        for who, call in calls.items():
            assert call() == -1, (who, n)
            err = lib.nqa_last_error()
            assert who.split("#")[0].encode() + b": window %d " % n in err and RANGE in err, (who, n, err)
        sizes = {
            "adists_workspace_bytes_n": lambda: lib.nqa_adists_workspace_bytes_n(2, 40, 56, n, 0),
            "adists_group_workspace_bytes_n": lambda: lib.nqa_adists_group_workspace_bytes_n(2, 3, 40, 56, n, 0),
            "adists_chain_bytes_n": lambda: lib.nqa_adists_chain_bytes_n(2, 40, 56, n),
            "adists_chain_group_bytes_n": lambda: lib.nqa_adists_chain_group_bytes_n(2, 3, 40, 56, n),
        }
        for who, call in sizes.items():
            assert call() == 0, (who, n)
            err = lib.nqa_last_error()
            assert who.encode() in err and RANGE in err, (who, n, err)
    for n in (3, 63):  # the ends of the range are inside it
        assert lib.nqa_adists_workspace_bytes_n(2, 40, 56, n, 0) > 0 and _dims(lib, 40, 56, n)[0] >= 0


def test_stage_refuses_bad_arguments(lib):
    for kw in ({"fx": None}, {"fy": None}, {"q": None}, {"wgt": None}, {"gamma": None}, {"tw": None}, {"sw": None}):
        assert _stage(lib, **kw) == -1, kw
        assert b"adists_window_stage: null pointer" in lib.nqa_last_error()
        assert _stage_group(lib, **kw) == -1, kw
        assert b"adists_window_stage_group: null pointer" in lib.nqa_last_error()
    for kw in ({"B": 0}, {"H": 0}, {"W": -3}, {"C_": 0}, {"prec": -1}, {"prec": 4}):
        assert _stage(lib, **kw) == -1, kw
        assert b"adists_window_stage: bad size or prec" in lib.nqa_last_error()
    for kw in ({"R": 0}, {"K": 0}, {"R": 256, "K": 256}):
        assert _stage_group(lib, **kw) == -1, kw
        assert b"adists_window_stage_group: bad group" in lib.nqa_last_error()
    # strip: 0 or 1 .. H-n+1 (34 here), for planes as well; only its sign under the window
    for kw in ({"strip": -1}, {"strip": 35}, {"strip": 35, "C_": 3}, {"strip": -2, "H": 5}):
        assert _stage(lib, **kw) == -1, kw
        assert b"adists_window_stage: strip" in lib.nqa_last_error()
    for c in (1, 4, 32, 63, 65, 192, 1024):
        assert _stage(lib, C_=c) == -2, c
        assert b"adists_window_stage: unsupported channel count" in lib.nqa_last_error()
    assert _stage(lib, H=1 << 10, W=1 << 10, C_=512) == -2 and b"adists_window_stage: map too large" in lib.nqa_last_error()


def test_forwards_and_chain_refuse_bad_arguments(lib):
    big = 1 << 40
    fwd = lambda **kw: lib.nqa_adists_forward_n(kw.get("x", P[0]), kw.get("y", P[1]), kw.get("B", 2), kw.get("H", 40),
                                                kw.get("W", 56), 7, kw.get("packed", P[2]), kw.get("prec", 0),
                                                kw.get("ws", P[3]), kw.get("bytes", big), kw.get("d", P[4]), None)
    for kw in ({"x": None}, {"y": None}, {"packed": None}, {"ws": None}, {"d": None}):
        assert fwd(**kw) == -1 and b"adists_forward: null pointer" in lib.nqa_last_error(), kw
    for kw in ({"B": 0}, {"H": -1}, {"prec": 9}):
        assert fwd(**kw) == -1 and b"adists_forward: bad size or prec" in lib.nqa_last_error(), kw
    need = lib.nqa_adists_workspace_bytes_n(2, 40, 56, 7, 0)
    assert need > lib.nqa_adists_workspace_bytes(2, 40, 56, 0)
    assert fwd(bytes=need - 1) == -3 and b"adists_forward: workspace" in lib.nqa_last_error()
    assert lib.nqa_adists_forward_map_n(P[0], P[1], 2, 40, 56, 7, P[2], 0, P[3], big, P[4], None, None) == -1
    assert b"adists_forward_map: null map pointer" in lib.nqa_last_error()
    assert lib.nqa_adists_dists_forward_n(P[0], P[1], 2, 40, 56, 7, P[2], 0, P[3], big, P[4], None, P[6], None, None) == -1
    assert b"adists_dists_forward: null similarity pointer" in lib.nqa_last_error()
    assert lib.nqa_adists_forward_group_n(None, P[1], 2, 3, 40, 56, 7, P[2], 0, P[3], big, P[4], None, None, None) == -1
    assert b"adists_forward_group: null pointer" in lib.nqa_last_error()
    gneed = lib.nqa_adists_group_workspace_bytes_n(2, 3, 40, 56, 7, 0)
    assert lib.nqa_adists_forward_group_n(P[0], P[1], 2, 3, 40, 56, 7, P[2], 0, P[3], gneed - 1, P[4], None, None, None) == -3
    assert lib.nqa_adists_chain_n(None, _arr(P[1]), _arr(P[2]), 2, 40, 56, 7, P[3], big, _arr(P[4]), P[5], None, None) == -1
    assert b"adists_chain: null pointer" in lib.nqa_last_error()
    cneed = lib.nqa_adists_chain_bytes_n(2, 40, 56, 7)
    assert lib.nqa_adists_chain_n(_arr(P[0]), _arr(P[1]), _arr(P[2]), 2, 40, 56, 7, P[3], cneed - 1, _arr(P[4]), P[5], None,
                                  None) == -3
    assert lib.nqa_adists_chain_group_n(_arr(P[0]), _arr(P[1]), _arr(P[2]), 2, 0, 40, 56, 7, P[3], big, _arr(P[4]), P[5],
                                        None) == -1
    assert b"adists_chain_group: bad group" in lib.nqa_last_error()
    mh = (C.c_int * 6)()
    assert lib.nqa_adists_chain_dims_n(40, 56, 7, None, mh) == -1 and b"adists_chain_dims: null pointer" in lib.nqa_last_error()


def test_variant_bit_for_the_generic_kernels(lib):
    from nerf_qa_amd import ops
    g = (C.c_int * 3)()
    try:
        ops.set_conv_variant(ops.DEFAULT_CONV_VARIANT | ops.CONV_WINDOW_GENERIC)
        assert lib.nqa_adists_window_grid(1, 40, 56, 64, 0, 0, g) == 0 and tuple(g) == (0, 0, 0)  # no LDS kernel runs
        for bad in (2048 | 1024, 2048 | 3, 4096):
            assert lib.nqa_set_conv_variant(bad) == -1 and b"unknown variant %d" % bad in lib.nqa_last_error()
    finally:
        ops.set_conv_variant(ops.DEFAULT_CONV_VARIANT)
    assert lib.nqa_adists_window_grid(1, 40, 56, 64, 0, 0, g) == 0 and tuple(g) == (9, 1, 20)


def test_python_surface_refuses_bad_windows():
    from nerf_qa_amd import _lib, ops
    for bad in (2, 64, 0, -1, 21.5, "21", None, True):
        with pytest.raises(ValueError, match=r"3\.\.63"):
            ops.check_window(bad)
        with pytest.raises(ValueError, match=r"3\.\.63"):
            ops.adists_chain_dims(40, 56, bad)
    assert ops.check_window(21) == 21 and ops.check_window(torch.tensor(7).item()) == 7
    x, q, w = torch.rand(1, 24, 24, 64), torch.rand(8, 1, 64), torch.rand(1, 64)
    with pytest.raises(_lib.NqaError):
        ops.adists_window_stage(x, x, q, w, "f32", window=7)  # CPU tensors
    with pytest.raises(ValueError, match=r"3\.\.63"):
        ops.adists_window_stage(x, x, q, w, "f32", window=64)
