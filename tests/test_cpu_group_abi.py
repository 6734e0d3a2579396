"""CPU-side checks of the group entry points (include/nqa.h: nqa_dists_forward_group, nqa_dists_group_stats, their two
size queries, and the tests' and tools' nqa_dists_group_sums / nqa_dists_group_stats_grid): declared in the header, exported by the library, bound by _lib.py; every refusal happens on the host
-- an error code and a message naming the function, never a launch (the pointers below are fakes that nothing may
dereference, and no device is touched); the workspace covers R + R * K images and the partial sums of R * K pairs."""
import os
import re

import pytest
import torch

NEW = ("nqa_dists_group_workspace_bytes", "nqa_dists_forward_group", "nqa_dists_group_stats_bytes", "nqa_dists_group_stats",
       "nqa_dists_group_sums", "nqa_dists_group_stats_grid")
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "nqa.h")
PREC = {"f32": 0, "bf16": 1, "f16": 2, "f32s": 3, "f32m": 4, "f32m2": 5, "f32m4": 6, "f16w": 7}
FAKE = 0x10000  # fake device pointers start here
E_ARG, E_SHAPE, E_WORKSPACE = -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    from nerf_qa_amd import build, _lib
    build.build()
    return _lib.lib()


def test_exports_are_declared_bound_and_present(lib):
    from nerf_qa_amd import _lib, build, ops, video
    from nerf_qa_amd.DISTS_pytorch import DISTS
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(nqa_[a-z0-9_]+)\s*\(", text))
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    for name in NEW:
        assert re.search(r"\b%s\(" % name, text), name
        assert name in _lib.EXPORTS and getattr(lib, name) is not None, name
    assert "DISTS_pt.py:105-141" in text.split("nqa_dists_group_workspace_bytes(int R")[0][-2500:]  # the lines it replaces
    assert "nqa_group_stats.hip" in build.SOURCES
    for k in ("group_stats_nhwc_kernel", "group_stats_nchw_kernel"):
        assert k in build.NO_SCRATCH
    assert callable(ops.dists_forward_group) and callable(ops.dists_group_stats)
    assert callable(ops.dists_group_sums) and callable(ops.dists_group_stats_grid)
    doc = text.split("int nqa_dists_group_sums(")[0][-1500:]
    assert "for tests and tools" in doc and "sum x, sum y, sum x^2, sum y^2, sum xy" in doc
    assert callable(DISTS.forward_group) and callable(video.score_videos)


def test_group_kernels_are_in_the_tracked_resource_report():
    """Float, f16 and bf16 instances of the NHWC kernel and the plane kernel, none with scratch."""
    import json
    from nerf_qa_amd import build as b
    res = json.load(open(b.RESOURCES))
    nhwc = [k for k in res if "group_stats_nhwc_kernel" in k]
    assert len(nhwc) == 3 and {t for k in nhwc for t in ("PrecF32", "PrecF16", "PrecBF16") if t in k} == {"PrecF32", "PrecF16", "PrecBF16"}
    assert len([k for k in res if "group_stats_nchw_kernel" in k]) == 1
    for k in res:
        if "group_stats" in k:
            assert res[k]["scratch"] == 0, (k, res[k])


def test_workspace_covers_the_images_and_the_pairs(lib):
    for prec in PREC.values():
        for R, K, H, W in ((1, 1, 17, 23), (2, 3, 33, 47), (1, 8, 256, 256), (4, 2, 8, 8), (1, 1, 1, 1)):
            n = R + R * K
            got = lib.nqa_dists_group_workspace_bytes(R, K, H, W, prec)
            assert got > 0 and got % 256 == 0
            esz = 4 if prec in (0, 3) else 2
            assert got >= 2 * n * H * W * 64 * esz + R * K * 1475 * 5 * 8, (prec, R, K, H, W)
            assert lib.nqa_dists_group_workspace_bytes(R, K + 1, H, W, prec) > got
            assert lib.nqa_dists_group_workspace_bytes(R + 1, K, H, W, prec) > got
    for bad in ((0, 1, 8, 8, 0), (1, 0, 8, 8, 0), (-1, 2, 8, 8, 0), (1, 1, 0, 8, 0), (1, 1, 8, -8, 0), (1, 1, 8, 8, 8),
                (1, 1, 8, 8, -1), (256, 256, 8, 8, 0)):
        assert lib.nqa_dists_group_workspace_bytes(*bad) == 0, bad


def _forward(lib, R=2, K=3, H=33, W=47, prec=3, ref=FAKE, ren=2 * FAKE, packed=3 * FAKE, ws=4 * FAKE, ws_bytes=None,
             s1=5 * FAKE, s2=6 * FAKE):
    if ws_bytes is None:
        ws_bytes = lib.nqa_dists_group_workspace_bytes(max(R, 1), max(K, 1), 33, 47, 3) + (1 << 20)
    return lib.nqa_dists_forward_group(ref, ren, R, K, H, W, packed, prec, ws, ws_bytes, s1, s2, None)


def test_forward_group_refuses_bad_arguments(lib):
    for kw in ({"ref": None}, {"ren": None}, {"packed": None}, {"ws": None}, {"s1": None}, {"s2": None}):
        assert _forward(lib, **kw) == E_ARG, kw
        assert b"dists_forward_group: null pointer" in lib.nqa_last_error()
    for kw in ({"R": 0}, {"R": -1}, {"K": 0}, {"K": -3}, {"H": 0}, {"W": 0}, {"H": -5}):
        assert _forward(lib, ws_bytes=1 << 30, **kw) == E_ARG, kw
        assert b"dists_forward_group: non-positive size" in lib.nqa_last_error()
    assert _forward(lib, R=256, K=256, ws_bytes=1 << 40) == E_ARG
    assert b"dists_forward_group: R*K = 65536 pairs" in lib.nqa_last_error()
    for prec in (8, -1, 100):
        assert _forward(lib, prec=prec) == E_ARG, prec
        assert b"dists_forward_group: unknown prec" in lib.nqa_last_error()
    # the pairwise path's limit: H * W * 64 elements of the mode's type reaching 2^31 bytes; one row less passes this
    # check and stops at the short workspace
    for prec, px in ((0, 1 << 23), (3, 1 << 23), (2, 1 << 24), (4, 1 << 24)):
        assert _forward(lib, R=1, K=1, H=px // 1024, W=1024, prec=prec, ws_bytes=1) == E_ARG, prec
        assert b"dists_forward_group: map too large" in lib.nqa_last_error()
        assert _forward(lib, R=1, K=1, H=px // 1024 - 1, W=1024, prec=prec, ws_bytes=1) == E_WORKSPACE, prec
    for prec in PREC.values():  # every mode of the pairwise forward is taken, the mixed ones included
        need = lib.nqa_dists_group_workspace_bytes(2, 3, 33, 47, prec)
        for short in (0, 1, need - 1):
            assert _forward(lib, prec=prec, ws_bytes=short) == E_WORKSPACE, (prec, short)
            assert b"dists_forward_group: workspace" in lib.nqa_last_error()


def _stats(lib, R=2, K=3, HW=35, C=64, prec=0, nchw=0, feat=FAKE, scratch=2 * FAKE, nbytes=None, s1=3 * FAKE, s2=4 * FAKE):
    if nbytes is None:
        nbytes = 1 << 30
    return lib.nqa_dists_group_stats(feat, R, K, HW, C, prec, nchw, scratch, nbytes, s1, s2, None)


def _sums(lib, R=2, K=3, HW=35, C=64, prec=0, nchw=0, feat=FAKE, scratch=2 * FAKE, nbytes=None, sums=3 * FAKE):
    if nbytes is None:
        nbytes = 1 << 30
    return lib.nqa_dists_group_sums(feat, R, K, HW, C, prec, nchw, scratch, nbytes, sums, None)


def test_group_sums_refuses_what_group_stats_refuses(lib):
    """Every refusal of nqa_dists_group_stats under the name dists_group_sums, and a null sums."""
    for kw in ({"feat": None}, {"scratch": None}, {"sums": None}):
        assert _sums(lib, **kw) == E_ARG, kw
        assert b"dists_group_sums: null pointer" in lib.nqa_last_error()
    for kw in ({"R": 0}, {"K": 0}, {"R": -2}, {"K": -1}, {"HW": 0}, {"HW": -7}, {"C": 0}, {"C": -64}):
        assert _sums(lib, **kw) == E_ARG, kw
        assert b"dists_group_sums: non-positive size" in lib.nqa_last_error()
    assert _sums(lib, R=65536, K=1) == E_ARG and b"dists_group_sums: R*K = 65536 pairs" in lib.nqa_last_error()
    for prec in (4, 5, 6, 7):
        assert _sums(lib, prec=prec) == E_ARG and b"dists_group_sums: takes no mixed mode" in lib.nqa_last_error()
    for prec in (8, -1):
        assert _sums(lib, prec=prec) == E_ARG and b"dists_group_sums: unknown prec" in lib.nqa_last_error()
    for C, prec, nchw, hw in ((64, 0, 0, 1 << 23), (512, 3, 0, 1 << 20), (512, 2, 0, 1 << 21), (3, 2, 1, (1 << 29) // 3 + 1)):
        assert _sums(lib, HW=hw, C=C, prec=prec, nchw=nchw, nbytes=1) == E_ARG, (C, prec, nchw)
        assert b"dists_group_sums: map too large" in lib.nqa_last_error()
        assert _sums(lib, HW=hw - 1, C=C, prec=prec, nchw=nchw, nbytes=1) == E_WORKSPACE, (C, prec, nchw)
    for C, prec in ((3, 0), (6, 0), (12, 0), (4, 2), (24, 2), (96, 0), (2048, 0)):
        assert _sums(lib, C=C, prec=prec) == E_SHAPE, (C, prec)
        assert b"dists_group_sums: no NHWC kernel for C=%d" % C in lib.nqa_last_error()
    for C, prec, nchw in ((64, 0, 0), (512, 2, 0), (128, 1, 0), (256, 3, 0), (3, 0, 1), (5, 2, 1)):
        need = lib.nqa_dists_group_stats_bytes(2, 3, 35, C, prec, nchw)  # (the same scratch as nqa_dists_group_stats)
        for short in (0, 1, 6 * C * 5 * 8 - 1):
            assert _sums(lib, C=C, prec=prec, nchw=nchw, nbytes=short) == E_WORKSPACE, (C, prec, nchw, short)
            assert b"dists_group_sums: scratch" in lib.nqa_last_error()
        assert need >= 6 * C * 5 * 8


def test_group_stats_grid_reports_the_plan_and_refuses_on_the_host(lib):
    import ctypes
    g = (ctypes.c_int * 4)()
    assert lib.nqa_dists_group_stats_grid(2, 3, 35, 64, 0, 0, None) == E_ARG
    assert b"dists_group_stats_grid: null pointer" in lib.nqa_last_error()
    for args, code in (((0, 1, 35, 64, 0, 0), E_ARG), ((1, 0, 35, 64, 0, 0), E_ARG), ((65536, 1, 35, 64, 0, 0), E_ARG),
                       ((1, 1, 0, 64, 0, 0), E_ARG), ((1, 1, 35, 0, 0, 1), E_ARG), ((1, 1, 35, 64, 4, 0), E_ARG),
                       ((1, 1, 35, 64, 8, 0), E_ARG), ((1, 1, 35, 96, 0, 0), E_SHAPE), ((1, 1, 35, 4, 2, 0), E_SHAPE)):
        assert lib.nqa_dists_group_stats_grid(*args, g) == code, args
        assert b"dists_group_stats_grid: " in lib.nqa_last_error()
        assert lib.nqa_dists_group_stats_bytes(*args) == 0, args
    # the scratch holds exactly the plan's partials; a thread never holds more than 16 items, and the blocks cover the map
    for prec in (0, 1, 2, 3):
        for nchw in (0, 1):
            for C in ((3, 64) if nchw else (64, 128, 256, 512)):
                for R, K, HW in ((1, 1, 1), (2, 3, 35), (3, 2, 1551), (1, 2, 24589), (1, 1, 262144), (4, 1, 1 << 18), (1, 1, 1 << 20)):
                    key = (prec, nchw, C, R, K, HW)
                    assert lib.nqa_dists_group_stats_grid(R, K, HW, C, prec, nchw, g) == 0, key
                    ppb, nblk, pl, items = tuple(g)
                    assert pl == (256 if nchw else 256 // (C // (4 if prec in (0, 3) else 8))), key
                    assert ppb % pl == 0 or (nchw and ppb == HW), key
                    assert 1 <= items <= 16 and items == -(-min(ppb, HW) // pl), key
                    assert (nblk - 1) * ppb < HW <= nblk * ppb, key
                    need = lib.nqa_dists_group_stats_bytes(R, K, HW, C, prec, nchw)
                    assert need == -(-(R * K * nblk * C * 5 * 8) // 256) * 256, key
    from nerf_qa_amd import ops
    assert ops.dists_group_stats_grid(2, 3, 35, 64, "f32") == (64, 1, 16, 3)
    assert ops.dists_group_stats_grid(2, 3, 4097, 3, "f16", nchw=True) == (4096, 2, 256, 16)


def test_group_stats_refuses_bad_arguments(lib):
    for kw in ({"feat": None}, {"scratch": None}, {"s1": None}, {"s2": None}):
        assert _stats(lib, **kw) == E_ARG, kw
        assert b"dists_group_stats: null pointer" in lib.nqa_last_error()
    for kw in ({"R": 0}, {"K": 0}, {"R": -2}, {"K": -1}, {"HW": 0}, {"HW": -7}, {"C": 0}, {"C": -64}):
        assert _stats(lib, **kw) == E_ARG, kw
        assert b"dists_group_stats: non-positive size" in lib.nqa_last_error()
        assert lib.nqa_dists_group_stats_bytes(kw.get("R", 2), kw.get("K", 3), kw.get("HW", 35), kw.get("C", 64), 0, 0) == 0
    assert _stats(lib, R=65536, K=1) == E_ARG and b"dists_group_stats: R*K = 65536 pairs" in lib.nqa_last_error()
    for prec in (4, 5, 6, 7):
        assert _stats(lib, prec=prec) == E_ARG and b"dists_group_stats: takes no mixed mode" in lib.nqa_last_error()
    for prec in (8, -1):
        assert _stats(lib, prec=prec) == E_ARG and b"dists_group_stats: unknown prec" in lib.nqa_last_error()
    # a map of HW * C elements reaching 2^31 bytes (planes are float whatever prec says)
    for C, prec, nchw, hw in ((64, 0, 0, 1 << 23), (512, 3, 0, 1 << 20), (512, 2, 0, 1 << 21), (3, 2, 1, (1 << 29) // 3 + 1)):
        assert _stats(lib, HW=hw, C=C, prec=prec, nchw=nchw, nbytes=1) == E_ARG, (C, prec, nchw)
        assert b"dists_group_stats: map too large" in lib.nqa_last_error()
        assert _stats(lib, HW=hw - 1, C=C, prec=prec, nchw=nchw, nbytes=1) == E_WORKSPACE, (C, prec, nchw)
    # channel counts the NHWC kernel does not take: not whole 16-byte groups, or not a power-of-two number of them
    for C, prec in ((3, 0), (6, 0), (12, 0), (4, 2), (24, 2), (96, 0), (2048, 0)):
        assert _stats(lib, C=C, prec=prec) == E_SHAPE, (C, prec)
        assert b"dists_group_stats: no NHWC kernel for C=%d" % C in lib.nqa_last_error()
        assert lib.nqa_dists_group_stats_bytes(2, 3, 35, C, prec, 0) == 0
        assert lib.nqa_dists_group_stats_bytes(2, 3, 35, C, prec, 1) > 0  # the plane kernel takes any C
    for C, prec, nchw in ((64, 0, 0), (512, 2, 0), (128, 1, 0), (256, 3, 0), (3, 0, 1), (5, 2, 1)):
        need = lib.nqa_dists_group_stats_bytes(2, 3, 35, C, prec, nchw)
        assert need >= 6 * C * 5 * 8 and need % 256 == 0
        for short in (0, 1, 6 * C * 5 * 8 - 1):
            assert _stats(lib, C=C, prec=prec, nchw=nchw, nbytes=short) == E_WORKSPACE, (C, prec, nchw, short)
            assert b"dists_group_stats: scratch" in lib.nqa_last_error()


def test_ops_and_module_refuse_on_the_host():
    """Shape mismatches and images that require grad: ValueError; CPU tensors: NqaError -- all before any launch."""
    import warnings
    from nerf_qa_amd import _lib, ops, video
    from nerf_qa_amd.DISTS_pytorch import DISTS
    ref, ren = torch.rand(2, 3, 16, 20), torch.rand(2, 3, 3, 16, 20)
    blob = torch.zeros(16, dtype=torch.uint8)
    with pytest.raises(_lib.NqaError):
        ops.dists_forward_group(ref, ren, blob, "f32")
    with pytest.raises(_lib.NqaError):
        ops.dists_group_stats(torch.rand(8, 35, 64), 2, 3, "f32")
    with pytest.raises(_lib.NqaError):
        ops.dists_group_sums(torch.rand(8, 35, 64), 2, 3, "f32")
    with pytest.raises(_lib.NqaError):
        ops.dists_group_stats_grid(2, 3, 35, 96, "f32")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = DISTS(precision="f32s")
    with pytest.raises(_lib.NqaError):
        model.forward_group(ref, ren)
    for a, b in ((ref, ren[:1]), (ref, ren[:, :, :2]), (ref, ren[..., :19]), (ref, ren[:, 0]), (ref[0], ren), (ref, ren[:, :0]),
                 (ref[:, :, :0], ren[:, :, :, :0]), (ref, None)):
        with pytest.raises(ValueError):
            model.forward_group(a, b)
    with pytest.raises(ValueError):
        model.forward_group(ref.clone().requires_grad_(True), ren)
    with pytest.raises(ValueError):
        model.forward_group(ref, ren.clone().requires_grad_(True))
    with torch.no_grad(), pytest.raises(_lib.NqaError):  # (without autograd the images' flag does not matter: the CPU refusal)
        model.forward_group(ref.clone().requires_grad_(True), ren)
    with pytest.raises(ValueError):
        video.score_videos(ref, [ref, ref[:1]], model)
    with pytest.raises(ValueError):
        video.score_videos(ref, [], model)
