"""CPU-side checks of the pair path's single-operator statistics entries (include/nqa.h: nqa_pool_stats,
nqa_pool_stats_f16_to_split16, nqa_stats_nhwc, their two size queries and two grid queries): declared in the header,
exported by the library, bound by _lib.py; every refusal happens on the host -- an error code and a message naming the
function, never a launch (the pointers below are fakes that nothing may dereference, and no device is touched); the
workspace covers B * blocks * C * 5 doubles; the grid queries' tiles cover the pooled map and the strips cover the pixels."""
import ctypes as C
import os
import re

import pytest
import torch

NEW = ("nqa_pool_stats_workspace_bytes", "nqa_stats_nhwc_workspace_bytes", "nqa_pool_stats_grid", "nqa_stats_nhwc_grid",
       "nqa_pool_stats", "nqa_pool_stats_f16_to_split16", "nqa_stats_nhwc")
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "nqa.h")
PREC = {"f32": 0, "bf16": 1, "f16": 2, "f32s": 3}
MIXED = (4, 5, 6, 7)
FAKE = 0x10000  # fake device pointers start here
E_ARG, E_SHAPE, E_WORKSPACE = -1, -2, -3
BIG = 1 << 40


@pytest.fixture(scope="module")
def lib():
    from nerf_qa_amd import build, _lib
    build.build()
    return _lib.lib()


def _cpc(prec):
    return 4 if prec in (0, 3) else 8


def test_exports_are_declared_bound_and_present(lib):
    from nerf_qa_amd import _lib, ops
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(nqa_[a-z0-9_]+)\s*\(", text))
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    for name in NEW:
        assert re.search(r"\b%s\(" % name, text), name
        assert name in _lib.EXPORTS and getattr(lib, name) is not None, name
    doc = text.split("size_t nqa_pool_stats_workspace_bytes(")[0][-3000:]
    assert "DISTS_pt.py:22-25" in doc and "DISTS_pt.py:131-139" in doc  # the lines they replace
    assert lib.nqa_version() == 1  # adding a function is compatible
    for fn in (ops.pool_stats, ops.stats_nhwc, ops.pool_stats_grid, ops.stats_nhwc_grid):
        assert callable(fn)


def _pool(lib, B=2, H=9, W=11, C_=64, prec=0, feat=FAKE, pooled=2 * FAKE, sums=3 * FAKE, ws=4 * FAKE, nbytes=BIG, split=False):
    if split:
        return lib.nqa_pool_stats_f16_to_split16(feat, B, H, W, C_, pooled, sums, ws, nbytes, None)
    return lib.nqa_pool_stats(feat, B, H, W, C_, prec, pooled, sums, ws, nbytes, None)


def _stats(lib, B=2, HW=35, C_=64, prec=0, feat=FAKE, sums=3 * FAKE, ws=4 * FAKE, nbytes=BIG):
    return lib.nqa_stats_nhwc(feat, B, HW, C_, prec, sums, ws, nbytes, None)


def _grid(lib, B, H, W, C_, prec):
    g = (C.c_int * 5)()
    assert lib.nqa_pool_stats_grid(B, H, W, C_, prec, g) == 0, lib.nqa_last_error()
    return tuple(g)


def _sgrid(lib, B, HW, C_, prec):
    g = (C.c_int * 3)()
    assert lib.nqa_stats_nhwc_grid(B, HW, C_, prec, g) == 0, lib.nqa_last_error()
    return tuple(g)


@pytest.mark.parametrize("split", [False, True], ids=["pool_stats", "pool_stats_f16_to_split16"])
def test_pool_stats_refuses_bad_arguments(lib, split):
    who = b"pool_stats_f16_to_split16: " if split else b"pool_stats: "
    for kw in ({"feat": None}, {"pooled": None}, {"sums": None}, {"ws": None}):
        assert _pool(lib, split=split, **kw) == E_ARG, kw
        assert who + b"null pointer" in lib.nqa_last_error()
    for kw in ({"B": 0}, {"B": -1}, {"H": 0}, {"W": 0}, {"H": -3}, {"W": -9}, {"C_": 0}, {"C_": -64}):
        assert _pool(lib, split=split, **kw) == E_ARG, kw
        assert who + b"non-positive size" in lib.nqa_last_error()
    if not split:
        for prec in MIXED:
            assert _pool(lib, prec=prec) == E_ARG and b"pool_stats: takes no mixed mode" in lib.nqa_last_error()
        for prec in (8, -1, 100):
            assert _pool(lib, prec=prec) == E_ARG and b"pool_stats: unknown prec" in lib.nqa_last_error()
    assert _pool(lib, split=split, B=65536) == E_ARG and who + b"B = 65536 pairs" in lib.nqa_last_error()
    # a map of H * W * C elements reaching 2^31 bytes; one pixel less passes this check and stops at the short workspace
    cases = ((64, 2, 1 << 24),) if split else ((64, 0, 1 << 23), (512, 3, 1 << 20), (512, 2, 1 << 21), (128, 1, 1 << 23))
    for c, prec, px in cases:
        assert _pool(lib, split=split, B=1, H=px // 1024, W=1024, C_=c, prec=prec, nbytes=1) == E_ARG, (c, prec)
        assert who + b"map too large" in lib.nqa_last_error()
        assert _pool(lib, split=split, B=1, H=px // 1024 - 1, W=1024, C_=c, prec=prec, nbytes=1) == E_WORKSPACE, (c, prec)
    assert _pool(lib, split=split, B=1, H=1 << 30, W=1 << 30, C_=1 << 30, prec=2) == E_ARG  # (no overflow in the check itself)
    # channel counts the kernel does not take: not whole 16-byte groups, not a power-of-two number of them, more than 256
    # of them, or (split16 out) not whole 16-channel records
    bad_c = ((4, 2), (24, 2), (96, 2), (4096, 2), (8, 2)) if split else \
        ((3, 0), (6, 0), (12, 0), (4, 2), (24, 2), (96, 0), (2048, 0), (4096, 1), (4, 3), (8, 3), (96, 3))
    for c, prec in bad_c:
        assert _pool(lib, split=split, C_=c, prec=prec) == E_SHAPE, (c, prec)
        assert who + b"no kernel for C=%d" % c in lib.nqa_last_error()
        if not split:
            assert lib.nqa_pool_stats_workspace_bytes(2, 9, 11, c, prec) == 0
    for c, prec in ((16, 2), (64, 2), (2048, 2)) if split else ((4, 0), (8, 2), (8, 1), (16, 3), (64, 0), (1024, 0), (2048, 2)):
        need = lib.nqa_pool_stats_workspace_bytes(2, 9, 11, c, prec)
        nblk = _grid(lib, 2, 9, 11, c, prec)[3]
        assert need >= 2 * nblk * c * 5 * 8 and need % 256 == 0 and need - 2 * nblk * c * 5 * 8 < 256
        for short in (0, 1, 2 * nblk * c * 5 * 8 - 1):
            assert _pool(lib, split=split, C_=c, prec=prec, nbytes=short) == E_WORKSPACE, (c, prec, short)
            assert who + b"workspace" in lib.nqa_last_error()


def test_stats_nhwc_refuses_bad_arguments(lib):
    for kw in ({"feat": None}, {"sums": None}, {"ws": None}):
        assert _stats(lib, **kw) == E_ARG, kw
        assert b"stats_nhwc: null pointer" in lib.nqa_last_error()
    for kw in ({"B": 0}, {"B": -2}, {"HW": 0}, {"HW": -7}, {"C_": 0}, {"C_": -64}):
        assert _stats(lib, **kw) == E_ARG, kw
        assert b"stats_nhwc: non-positive size" in lib.nqa_last_error()
        assert lib.nqa_stats_nhwc_workspace_bytes(kw.get("B", 2), kw.get("HW", 35), kw.get("C_", 64), 0) == 0
    for prec in MIXED:
        assert _stats(lib, prec=prec) == E_ARG and b"stats_nhwc: takes no mixed mode" in lib.nqa_last_error()
    for prec in (8, -1):
        assert _stats(lib, prec=prec) == E_ARG and b"stats_nhwc: unknown prec" in lib.nqa_last_error()
    assert _stats(lib, B=65536) == E_ARG and b"stats_nhwc: B = 65536 pairs" in lib.nqa_last_error()
    for c, prec, hw in ((64, 0, 1 << 23), (512, 3, 1 << 20), (512, 2, 1 << 21), (128, 1, 1 << 23)):
        assert _stats(lib, B=1, HW=hw, C_=c, prec=prec, nbytes=1) == E_ARG, (c, prec)
        assert b"stats_nhwc: map too large" in lib.nqa_last_error()
        assert _stats(lib, B=1, HW=hw - 1, C_=c, prec=prec, nbytes=1) == E_WORKSPACE, (c, prec)
    for c, prec in ((3, 0), (6, 0), (12, 0), (4, 2), (24, 2), (96, 0), (2048, 0), (4096, 1)):
        assert _stats(lib, C_=c, prec=prec) == E_SHAPE, (c, prec)
        assert b"stats_nhwc: no kernel for C=%d" % c in lib.nqa_last_error()
        assert lib.nqa_stats_nhwc_workspace_bytes(2, 35, c, prec) == 0
    for c, prec in ((4, 0), (4, 3), (8, 2), (64, 0), (512, 2), (128, 1), (256, 3), (1024, 0), (2048, 1)):
        need = lib.nqa_stats_nhwc_workspace_bytes(2, 35, c, prec)
        nblk = _sgrid(lib, 2, 35, c, prec)[1]
        assert need >= 2 * nblk * c * 5 * 8 and need % 256 == 0 and need - 2 * nblk * c * 5 * 8 < 256
        for short in (0, 1, 2 * nblk * c * 5 * 8 - 1):
            assert _stats(lib, C_=c, prec=prec, nbytes=short) == E_WORKSPACE, (c, prec, short)
            assert b"stats_nhwc: workspace" in lib.nqa_last_error()


def test_grid_queries_refuse_like_the_calls(lib):
    g5, g3 = (C.c_int * 5)(), (C.c_int * 3)()
    assert lib.nqa_pool_stats_grid(1, 8, 8, 64, 0, None) == E_ARG and b"pool_stats_grid: null pointer" in lib.nqa_last_error()
    assert lib.nqa_stats_nhwc_grid(1, 64, 64, 0, None) == E_ARG and b"stats_nhwc_grid: null pointer" in lib.nqa_last_error()
    for args, code in (((0, 8, 8, 64, 0), E_ARG), ((1, 8, 0, 64, 0), E_ARG), ((1, 8, 8, 64, 4), E_ARG), ((1, 8, 8, 64, 9), E_ARG),
                       ((1, 8, 8, 96, 0), E_SHAPE), ((1, 8, 8, 8, 3), E_SHAPE), ((1, 1 << 12, 1 << 12, 64, 2), E_ARG)):
        assert lib.nqa_pool_stats_grid(*args, g5) == code, args
        assert b"pool_stats_grid: " in lib.nqa_last_error()
    for args, code in (((0, 64, 64, 0), E_ARG), ((1, 0, 64, 0), E_ARG), ((1, 64, 64, 5), E_ARG), ((1, 64, 96, 0), E_SHAPE),
                       ((1, 1 << 24, 64, 2), E_ARG)):
        assert lib.nqa_stats_nhwc_grid(*args, g3) == code, args
        assert b"stats_nhwc_grid: " in lib.nqa_last_error()


SWEEP_B = (1, 2, 3, 8, 32, 200)
SWEEP_HW = ((1, 1), (2, 2), (1, 9), (9, 1), (3, 3), (5, 7), (4, 6), (37, 67), (37, 131), (36, 64), (96, 80), (128, 120),
            (163, 153), (222, 221), (270, 480), (540, 960), (1080, 1920))


def test_pool_stats_tiles_cover_the_pooled_map(lib):
    """For a sweep of (B, H, W, C, prec): TR x TC tiles, tiles_x across, cover Ho x Wo with none to spare; TC is one pass of
    the block, 256 / (C / channels per 16 bytes); a thread walks at least 4 and at most 16 rows unless the map is shorter."""
    seen_tr = set()
    for name, prec in PREC.items():
        for c in (64, 128, 256, 512):
            for b in SWEEP_B:
                for h, w in SWEEP_HW:
                    if h * w * c * (16 // _cpc(prec)) >= 1 << 31:
                        continue
                    tr, tc, tiles_x, nblk, grid = _grid(lib, b, h, w, c, prec)
                    ho, wo = (h + 1) // 2, (w + 1) // 2
                    key = (name, c, b, h, w)
                    assert tc == 256 // (c // _cpc(prec)), key
                    assert tiles_x == -(-wo // tc) and tiles_x * tc >= wo > (tiles_x - 1) * tc, key
                    tiles_y, rem = divmod(nblk, tiles_x)
                    assert rem == 0 and tiles_y * tr >= ho > (tiles_y - 1) * tr, key
                    assert grid == nblk * b, key
                    assert 1 <= tr <= ho and (tr >= 4 or tr == ho), key
                    # (past max(4096 / B, 16) blocks per pair the planner lengthens the strips instead: no upper bound there)
                    if -(-(ho * wo) // (16 * tc)) <= max(4096 // b, 16):
                        assert tr <= 16, key
                    seen_tr.add(tr)
                    assert lib.nqa_pool_stats_workspace_bytes(b, h, w, c, prec) >= b * nblk * c * 5 * 8, key
    assert {1, 2, 3, 4, 5, 16} <= seen_tr


def test_stats_nhwc_strips_cover_the_pixels(lib):
    for name, prec in PREC.items():
        for c in (64, 128, 256, 512):
            for b in SWEEP_B:
                for hw in (1, 35, 77, 299, 1551, 6007, 24589, 32400, 129600):
                    upb, nblk, pl = _sgrid(lib, b, hw, c, prec)
                    key = (name, c, b, hw)
                    assert pl == 256 // (c // _cpc(prec)) and upb % pl == 0 and upb >= 4 * pl, key
                    assert nblk * upb >= hw > (nblk - 1) * upb, key
                    assert lib.nqa_stats_nhwc_workspace_bytes(b, hw, c, prec) >= b * nblk * c * 5 * 8, key


def test_ops_refuse_on_the_host():
    """CPU tensors: NqaError before any launch; the grid queries run without a device and raise the library's refusals."""
    from nerf_qa_amd import _lib, ops
    with pytest.raises(_lib.NqaError):
        ops.pool_stats(torch.rand(4, 9, 11, 64), 2, "f32")
    with pytest.raises(_lib.NqaError):
        ops.stats_nhwc(torch.rand(4, 35, 64), 2, "f32")
    assert ops.pool_stats_grid(3, 37, 67, 64, "f32") == (4, 16, 3, 15, 45)
    assert ops.stats_nhwc_grid(1, 1, 64, "f16")[2] == 32
    with pytest.raises(_lib.NqaError):
        ops.pool_stats_grid(1, 8, 8, 96, "f32")
    with pytest.raises(_lib.NqaError):
        ops.stats_nhwc_grid(1, 8, 64, "f32m")
