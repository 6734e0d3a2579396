"""CPU-side checks of the entry point of the A-DISTS front part (include/nqa.h: nqa_adists_front, with
nqa_adists_front_bytes and nqa_adists_front_grid beside it): declared in the header, exported by the library, bound by
_lib.py; every refusal happens on the host -- an error code and a message naming the function, never a launch (the
pointers below are fakes that nothing may dereference, and no device is touched); the workspace grows with every tap;
and the grid query reports the block counts of the planning functions as tests/front_refs.py ports them."""
import ctypes as C
import os
import re

import pytest
import torch

import front_refs as R

NEW = ("nqa_adists_front", "nqa_adists_front_bytes", "nqa_adists_front_grid")
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "nqa.h")
PREC = {"f32": 0, "bf16": 1, "f16": 2, "f32s": 3}
FAKE = 0x10000  # fake device pointers start here
DIMS = ((7, 9), (9, 33), (13, 19), (5, 7), (9, 13), (3, 3))


@pytest.fixture(scope="module")
def lib():
    from nerf_qa_amd import build, _lib
    build.build()
    return _lib.lib()


def _hw(dims):
    return (C.c_int * 6)(*[d[0] for d in dims]), (C.c_int * 6)(*[d[1] for d in dims])


def _bytes(lib, B=2, dims=DIMS, prec=0):
    return lib.nqa_adists_front_bytes(B, *_hw(dims), prec)


def _grid(lib, B, dims, prec):
    g = (C.c_int * 24)()
    rc = lib.nqa_adists_front_grid(B, *_hw(dims), prec, g)
    return rc, [tuple(g[4 * k:4 * k + 4]) for k in range(6)]


def test_exports_are_declared_bound_and_present(lib):
    from nerf_qa_amd import _lib, ops
    text = open(HEADER).read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, text), name
        assert name in _lib.EXPORTS and getattr(lib, name) is not None, name
    assert callable(ops.adists_front) and callable(ops.adists_front_into) and callable(ops.adists_front_grid)
    assert "hsum" in text and "NON-NEGATIVE" in text  # the reused row and the contract are on record


def test_grid_is_the_planning_functions(lib):
    for c in R.CASES:
        rc, got = _grid(lib, c.B, c.dims, PREC[c.prec])
        assert rc == 0 and got == R.plan(c.B, c.dims, c.prec), (R.case_id(c), got, R.plan(c.B, c.dims, c.prec))
        for k, want in c.expect.items():
            assert all(w is None or w == g for w, g in zip(want, got[k])), (R.case_id(c), k, want, got[k])
    # sizes of the forward's own plans: a 1080p frame and a 256 x 256 one, where the block targets and caps act
    for B, (H, W) in ((1, (1080, 1920)), (8, (256, 256)), (32, (540, 960))):
        dims = [(H, W), (H, W)]
        for _ in range(4):
            dims.append(((dims[-1][0] + 1) // 2, (dims[-1][1] + 1) // 2))
        for prec in PREC:
            assert _grid(lib, B, dims, PREC[prec]) == (0, R.plan(B, dims, prec)), (B, H, W, prec)
    from nerf_qa_amd import ops
    assert ops.adists_front_grid(2, DIMS, "f16") == R.plan(2, DIMS, "f16")


def test_bytes_grow_with_every_tap(lib):
    base = _bytes(lib)
    assert base > 0 and base % 256 == 0
    for k in range(6):
        for grow in ((8, 0), (0, 8)):
            dims = [(h + grow[0], w + grow[1]) if j == k else (h, w) for j, (h, w) in enumerate(DIMS)]
            assert _bytes(lib, dims=dims) > base, (k, grow)
    assert _bytes(lib, B=3) > base
    for prec in PREC.values():
        assert _bytes(lib, prec=prec) > 0
    for kw in ({"B": 0}, {"B": -2}, {"prec": 4}, {"prec": -1}, {"dims": ((0, 9),) + DIMS[1:]},
               {"dims": DIMS[:5] + ((3, -3),)}):
        assert _bytes(lib, **kw) == 0, kw
    assert lib.nqa_adists_front_bytes(2, None, _hw(DIMS)[1], 0) == 0


def _front(lib, B=2, dims=DIMS, prec=0, x=FAKE, y=2 * FAKE, taps="ok", null_tap=None, ws=FAKE * 64, ws_bytes=None,
           q=FAKE * 65, wgt=FAKE * 66, hk="ok", wk="ok"):
    h, w = _hw(dims)
    if taps == "ok":
        taps = (C.c_void_p * 5)(*[3 * FAKE + 0x1000 * k for k in range(5)])
        if null_tap is not None:
            taps[null_tap] = None
    if ws_bytes is None:
        ws_bytes = max(_bytes(lib, max(B, 1), DIMS, 0), _bytes(lib, 2, dims, prec)) + (1 << 20)
    return lib.nqa_adists_front(x, y, taps, B, h if hk == "ok" else hk, w if wk == "ok" else wk, prec, ws, ws_bytes, q, wgt,
                                None)


def test_front_refuses_bad_arguments(lib):
    for kw in ({"x": None}, {"y": None}, {"taps": None}, {"ws": None}, {"q": None}, {"wgt": None}, {"hk": None},
               {"wk": None}):
        assert _front(lib, **kw) == -1, kw
        assert b"adists_front: null pointer" in lib.nqa_last_error()
    for k in range(5):
        assert _front(lib, null_tap=k) == -1, k
        assert b"adists_front: null pointer (tap %d)" % (k + 1) in lib.nqa_last_error()
    for kw in ({"B": 0}, {"B": -1}, {"prec": 4}, {"prec": 7}, {"prec": -1}):
        assert _front(lib, **kw) == -1, kw
        assert b"adists_front: bad size or prec" in lib.nqa_last_error()
    for k in range(6):
        for bad in ((0, 5), (5, 0), (-3, 5), (5, -1)):
            assert _front(lib, dims=DIMS[:k] + (bad,) + DIMS[k + 1:]) == -1, (k, bad)
            assert b"adists_front: bad size or prec (tap %d" % k in lib.nqa_last_error()
    # a tap of H * W * C elements reaching 2^31 bytes: 2^23 pixels of 64 floats, 2^20 of 512, 2^21 of 512 halves, 2^27
    # of the padded 4-float image; one pixel less passes this check (and stops at the short workspace)
    for k, prec, px in ((1, 0, 1 << 23), (4, 3, 1 << 20), (5, 0, 1 << 20), (5, 2, 1 << 21), (2, 1, 1 << 23), (0, 0, 1 << 27)):
        big = DIMS[:k] + ((px // 1024, 1024),) + DIMS[k + 1:]
        assert _front(lib, dims=big, prec=prec, ws_bytes=1) == -1, (k, prec)
        assert b"adists_front: tap %d too large" % k in lib.nqa_last_error()
        less = DIMS[:k] + ((px // 1024 - 1, 1024),) + DIMS[k + 1:]
        assert _front(lib, dims=less, prec=prec, ws_bytes=1) == -3, (k, prec)
    need = _bytes(lib)
    for short in (0, 1, need - 1):
        assert _front(lib, ws_bytes=short) == -3, short
        assert b"adists_front: workspace" in lib.nqa_last_error()
    g = (C.c_int * 24)()
    assert lib.nqa_adists_front_grid(2, *_hw(DIMS), 0, None) == -1 and b"adists_front_grid: null pointer" in lib.nqa_last_error()
    assert lib.nqa_adists_front_grid(2, None, _hw(DIMS)[1], 0, g) == -1
    assert lib.nqa_adists_front_grid(0, *_hw(DIMS), 0, g) == -1 and b"adists_front_grid: bad size" in lib.nqa_last_error()
    assert lib.nqa_adists_front_grid(2, *_hw(DIMS), 5, g) == -1


def test_ops_refuse_what_the_kernels_cannot_take():
    from nerf_qa_amd import _lib, ops
    B = 2
    x = torch.rand(B, 3, *DIMS[0])
    taps = [torch.rand(2 * B, h, w, c) for (h, w), c in zip(DIMS[1:], R.CHNS[1:])]
    with pytest.raises(_lib.NqaError):
        ops.adists_front(x, x, taps, "f32")  # CPU tensors
    bad = [(x, x, taps[:4], "f32"), (x, x[:1], taps, "f32"), (x[:, :2], x[:, :2], taps, "f32"), (x, x, taps, "f16"),
           (x, x, taps, "f32m"), (x.double(), x.double(), taps, "f32"), (x, x, [t[:3] for t in taps], "f32"),
           (x, x, taps[:1] + taps[:1] + taps[2:], "f32"), (x, x, [taps[0].transpose(1, 2)] + taps[1:], "f32"),
           (x, x, [t[:, :0] for t in taps], "f32"), (x, x, None, "f32"), (x.transpose(2, 3), x.transpose(2, 3), taps, "f32")]
    for args in bad:
        with pytest.raises(ValueError):
            ops.adists_front(*args)
    q, wgt = torch.empty(8, B, 1475), torch.empty(B, 1475)
    for outs in ((q[:7], wgt), (q, wgt[:1]), (q.double(), wgt), (q, None), (q.transpose(0, 1), wgt)):
        with pytest.raises(ValueError):
            ops.adists_front_into(x, x, taps, "f32", *outs)
    with pytest.raises(ValueError):
        ops.adists_front_grid(2, DIMS[:5], "f32")
    with pytest.raises(_lib.NqaError):
        ops.adists_front_grid(0, DIMS, "f32")
