"""CPU-side checks of the A-DISTS group entry points (include/nqa.h: nqa_adists_forward_group with its size query,
nqa_adists_window_stage_group, nqa_adists_chain_group with its size query): declared in the header, exported by the
library, bound by _lib.py; every refusal happens on the host -- an error code and a message naming the function, never a
launch (the pointers below are fakes that nothing may dereference, and no device is touched); the new kernels stand in
the tracked resource report without scratch, the one admitted exception of the LDS window kernel aside."""
import ctypes as C
import inspect
import json
import os
import re

import pytest
import torch

NEW = ("nqa_adists_group_workspace_bytes", "nqa_adists_forward_group", "nqa_adists_window_stage_group",
       "nqa_adists_chain_group_bytes", "nqa_adists_chain_group")
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "nqa.h")
PREC = {"f32": 0, "bf16": 1, "f16": 2, "f32s": 3}
MIXED = (4, 5, 6, 7)
FAKE = 0x10000  # fake device pointers start here
E_ARG, E_SHAPE, E_WORKSPACE = -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    from nerf_qa_amd import build, _lib
    build.build()
    return _lib.lib()


def test_exports_are_declared_bound_and_present(lib):
    from nerf_qa_amd import _lib, ops, pair, video
    from nerf_qa_amd.ADISTS import ADISTS
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(nqa_[a-z0-9_]+)\s*\(", text))
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    for name in NEW:
        assert re.search(r"\b%s\(" % name, text), name
        assert name in _lib.EXPORTS and getattr(lib, name) is not None, name
    comment = text.split("size_t nqa_adists_group_workspace_bytes(int R")[0].rsplit("/*", 1)[1]
    assert "ADISTS.py:137-197" in comment  # the lines the call replaces
    assert callable(ops.adists_forward_group) and callable(ops.adists_window_stage_group)
    assert callable(ops.adists_chain_group)
    assert callable(ADISTS.forward_group) and callable(pair.score_group) and callable(video.score_videos)


def test_group_kernels_are_in_the_tracked_resource_report():
    """Every group instance next to its pairwise parent: the LDS window kernel for float taps at the four channel counts,
    the first form for the three storage types, the planar and the global kernel, and the two chain kernels.  No
    scratch, but for the 8 bytes per lane the C >= 128 instances of the LDS kernel are allowed like their parents."""
    from nerf_qa_amd import build as b
    res = json.load(open(b.RESOURCES))
    lds = {k: v for k, v in res.items() if "adists_window_lds_group_kernel" in k}
    assert len(lds) == 4 and all("PrecF32" in k for k in lds)
    for k, v in lds.items():
        parent = res[k.replace("30adists_window_lds_group_kernel", "24adists_window_lds_kernel")[:-1]]
        assert v["scratch"] <= (0 if "Li64E" in k else 8) and v["scratch"] == parent["scratch"], (k, v, parent)
        assert v["occupancy"] == parent["occupancy"] == 3, (k, v)
    lanes = [k for k in res if "adists_window_lanes_group_kernel" in k]
    assert len(lanes) == 12 and {t for k in lanes for t in ("PrecF32", "PrecF16", "PrecBF16") if t in k} == {
        "PrecF32", "PrecF16", "PrecBF16"}
    for name in ("adists_window_planar_group_kernel", "adists_global_group_kernel", "chain_final_group_kernel",
                 "chain_global_group_kernel"):
        assert len([k for k in res if name in k]) == 1, name
    for k, v in res.items():
        if "_group_kernel" in k and "adists_window_lds_group_kernel" not in k:
            assert v["scratch"] == 0, (k, v)
    planar = next(v for k, v in res.items() if "adists_window_planar_group_kernel" in k)
    assert planar["occupancy"] == 3  # three waves per SIMD, like the pairwise planar kernel
    assert "adists_window_lds_group_kernel" in b.NO_SCRATCH and "adists_window_planar_group_kernel" in b.NO_SCRATCH
    assert b.SCRATCH_ALLOWED["adists_window_lds_group_kernel"] == b.SCRATCH_ALLOWED["adists_window_lds_kernel"]


def test_workspace_query(lib):
    q = lib.nqa_adists_group_workspace_bytes
    for prec in PREC.values():
        esz = 4 if prec in (0, 3) else 2
        for R, K, H, W in ((1, 1, 17, 23), (2, 3, 33, 47), (1, 8, 256, 256), (4, 2, 8, 8), (1, 1, 1, 1)):
            n, got = R + R * K, q(R, K, H, W, prec)
            assert got > 0 and got % 256 == 0
            # two ping-pong buffers and tap 1 of n images, the pairs' partial sums and scalars
            assert got >= 3 * n * H * W * 64 * esz + R * K * 1475 * (5 * 8 + 8 * 4), (prec, R, K, H, W)
            assert q(R, K + 1, H, W, prec) > got and q(R + 1, K, H, W, prec) > got
        # R = K = 1 is one pair.  The pairwise workspace holds two pyramids (x and y: half of every per-image buffer
        # each); the group call cannot need less than that workspace less the second pyramid's share, and it holds the
        # taps of both of its images
        for H, W in ((17, 23), (64, 96), (130, 95), (256, 256)):
            pairwise, group = lib.nqa_adists_workspace_bytes(1, H, W, prec), q(1, 1, H, W, prec)
            taps = sum(2 * -(-H // s) * -(-W // s) * c * esz for s, c in ((1, 64), (2, 128), (4, 256), (8, 512), (16, 512)))
            assert group >= pairwise - pairwise // 2, (prec, H, W, pairwise, group)
            assert group >= 2 * 2 * H * W * 64 * esz + taps, (prec, H, W, group)
    for bad in ((0, 1, 8, 8, 0), (1, 0, 8, 8, 0), (-1, 2, 8, 8, 0), (1, 1, 0, 8, 0), (1, 1, 8, -8, 0), (1, 1, 8, 8, 8),
                (1, 1, 8, 8, -1), (256, 256, 8, 8, 0), (1, 1, 8192, 1024, 0), (1, 1, 8192, 1024, 3), (1, 1, 16384, 1024, 2)):
        assert q(*bad) == 0, bad
    for prec in MIXED:  # the mixed modes are DISTS modes
        assert q(2, 3, 33, 47, prec) == 0, prec
    assert q(1, 1, 8191, 1024, 0) > 0 and q(255, 257, 8, 8, 0) > 0  # (one row, one pair under the limits)


def _forward(lib, R=2, K=3, H=33, W=47, prec=3, ref=FAKE, ren=2 * FAKE, packed=3 * FAKE, ws=4 * FAKE, ws_bytes=None,
             d=5 * FAKE, s1=6 * FAKE, s2=7 * FAKE):
    if ws_bytes is None:
        ws_bytes = 1 << 40
    return lib.nqa_adists_forward_group(ref, ren, R, K, H, W, packed, prec, ws, ws_bytes, d, s1, s2, None)


def test_forward_group_refuses_bad_arguments(lib):
    for kw in ({"ref": None}, {"ren": None}, {"packed": None}, {"ws": None}, {"d": None}):
        assert _forward(lib, **kw) == E_ARG, kw
        assert b"adists_forward_group: null pointer" in lib.nqa_last_error()
    for kw in ({"s1": None}, {"s2": None}):  # both or neither
        assert _forward(lib, **kw) == E_ARG, kw
        assert b"adists_forward_group: s1 and s2" in lib.nqa_last_error()
    for kw in ({"R": 0}, {"R": -1}, {"K": 0}, {"K": -3}, {"H": 0}, {"W": 0}, {"H": -5}):
        assert _forward(lib, **kw) == E_ARG, kw
        assert b"adists_forward_group: non-positive size" in lib.nqa_last_error()
    assert _forward(lib, R=256, K=256) == E_ARG
    assert b"adists_forward_group: R*K = 65536 pairs" in lib.nqa_last_error()
    for prec in (8, -1, 100):
        assert _forward(lib, prec=prec) == E_ARG, prec
        assert b"adists_forward_group: unknown prec" in lib.nqa_last_error()
    for prec in MIXED:
        assert _forward(lib, prec=prec) == E_ARG, prec
        assert b"adists_forward_group: the mixed modes are DISTS modes" in lib.nqa_last_error()
    # nqa_adists_forward's limit: H * W * 64 elements of the mode's type reaching 2^31 bytes; one row less passes this check
    # and stops at the short workspace
    for prec, px in ((0, 1 << 23), (3, 1 << 23), (2, 1 << 24), (1, 1 << 24)):
        assert _forward(lib, R=1, K=1, H=px // 1024, W=1024, prec=prec, ws_bytes=1) == E_ARG, prec
        assert b"adists_forward_group: image too large" in lib.nqa_last_error()
        assert _forward(lib, R=1, K=1, H=px // 1024 - 1, W=1024, prec=prec, ws_bytes=1) == E_WORKSPACE, prec
    for prec in PREC.values():
        need = lib.nqa_adists_group_workspace_bytes(2, 3, 33, 47, prec)
        for short in (0, 1, need - 1):
            for kw in ({}, {"s1": None, "s2": None}):
                assert _forward(lib, prec=prec, ws_bytes=short, **kw) == E_WORKSPACE, (prec, short)
                assert b"adists_forward_group: workspace" in lib.nqa_last_error()


def test_window_stage_group_refuses_bad_arguments(lib):
    def stage(R=2, K=3, H=41, W=37, C=64, prec=0, strip=0, **ptrs):
        p = {n: (i + 1) * FAKE for i, n in enumerate(("fx", "fy", "q", "wgt", "gamma", "tw", "sw"))}
        p.update(ptrs)
        return lib.nqa_adists_window_stage_group(p["fx"], p["fy"], R, K, H, W, C, prec, p["q"], p["wgt"], strip, p["gamma"],
                                                 p["tw"], p["sw"], None)
    for name in ("fx", "fy", "q", "wgt", "gamma", "tw", "sw"):
        assert stage(**{name: None}) == E_ARG, name
        assert b"adists_window_stage_group: null pointer" in lib.nqa_last_error()
    for kw in ({"R": 0}, {"K": 0}, {"R": -2}, {"R": 256, "K": 256}):
        assert stage(**kw) == E_ARG, kw
        assert b"adists_window_stage_group: bad group" in lib.nqa_last_error()
    for kw in ({"H": 0}, {"W": -1}, {"C": 0}, {"prec": 4}, {"prec": 9}):
        assert stage(**kw) == E_ARG, kw
        assert b"adists_window_stage_group: bad size or prec" in lib.nqa_last_error()
    for kw in ({"strip": -1}, {"strip": 22}):
        assert stage(**kw) == E_ARG, kw
        assert b"adists_window_stage_group: strip" in lib.nqa_last_error()
    assert stage(C=96) == E_SHAPE and b"adists_window_stage_group: unsupported channel count" in lib.nqa_last_error()
    assert stage(H=4096, W=2048, C=64) == E_SHAPE and b"adists_window_stage_group: map too large" in lib.nqa_last_error()


def test_chain_group_refuses_bad_arguments(lib):
    arr = lambda first, null_at=None: (C.c_void_p * 6)(*[None if k == null_at else first + 0x1000 * k for k in range(6)])

    def chain(R=2, K=3, H=40, W=56, ws=FAKE * 64, ws_bytes=None, d=FAKE * 65, **arrays):
        a = {"gamma": arr(FAKE), "tw": arr(2 * FAKE), "sw": arr(3 * FAKE), "ps_prod": arr(4 * FAKE)}
        a.update(arrays)
        if ws_bytes is None:
            ws_bytes = 1 << 40
        return lib.nqa_adists_chain_group(a["gamma"], a["tw"], a["sw"], R, K, H, W, ws, ws_bytes, a["ps_prod"], d, None)
    for name in ("gamma", "tw", "sw", "ps_prod"):
        assert chain(**{name: None}) == E_ARG, name
        assert b"adists_chain_group: null pointer" in lib.nqa_last_error()
        assert chain(**{name: arr(FAKE, null_at=4)}) == E_ARG, name
        assert b"adists_chain_group: null pointer (stage 4)" in lib.nqa_last_error()
    for kw in ({"ws": None}, {"d": None}):
        assert chain(**kw) == E_ARG and b"adists_chain_group: null pointer" in lib.nqa_last_error()
    for kw in ({"R": 0}, {"K": 0}, {"K": -1}, {"R": 65536, "K": 1}):
        assert chain(**kw) == E_ARG, kw
        assert b"adists_chain_group: bad group" in lib.nqa_last_error()
        assert lib.nqa_adists_chain_group_bytes(kw.get("R", 2), kw.get("K", 3), 40, 56) == 0
    for kw in ({"H": 0}, {"W": -3}):
        assert chain(**kw) == E_ARG and b"adists_chain_group: bad size" in lib.nqa_last_error()
    assert chain(H=1 << 12, W=1 << 11) == E_ARG and b"adists_chain_group: image too large" in lib.nqa_last_error()
    need = lib.nqa_adists_chain_group_bytes(2, 3, 40, 56)
    up = lambda n: (n + 255) // 256 * 256
    # accumulators of 40 bytes per (stage, reference) and per (stage, pair), 1024 block partials per pair, R ones
    assert need == up(6 * 2 * 40) + up(6 * 6 * 40) + up(6 * 1024 * 8) + up(2 * 4)
    assert lib.nqa_adists_chain_group_bytes(3, 1, 40, 56) == up(6 * 3 * 40) * 2 + up(2 * 3 * 1024 * 8) + up(3 * 4)  # K = 1
    for short in (0, 1, need - 1):
        assert chain(ws_bytes=short) == E_WORKSPACE and b"adists_chain_group: workspace" in lib.nqa_last_error()


def test_ops_and_modules_refuse_on_the_host():
    """Shape mismatches and images that require grad: ValueError; CPU tensors: NqaError -- all before any launch."""
    import warnings
    from nerf_qa_amd import _lib, ops, pair, video
    from nerf_qa_amd.ADISTS import ADISTS
    from nerf_qa_amd.DISTS_pytorch import DISTS
    ref, ren = torch.rand(2, 3, 16, 20), torch.rand(2, 3, 3, 16, 20)
    blob = torch.zeros(16, dtype=torch.uint8)
    with pytest.raises(_lib.NqaError):
        ops.adists_forward_group(ref, ren, blob, "f32")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        am, dm = ADISTS(), DISTS()
    for call in (am.forward_group, lambda a, b: pair.score_group(dm, am, a, b)):
        with pytest.raises(_lib.NqaError):
            call(ref, ren)
        for a, b in ((ref, ren[:1]), (ref, ren[:, :, :2]), (ref, ren[..., :19]), (ref, ren[:, 0]), (ref[0], ren),
                     (ref, ren[:, :0]), (ref[:, :, :0], ren[:, :, :, :0]), (ref, None)):
            with pytest.raises(ValueError):
                call(a, b)
        for a, b in ((ref.clone().requires_grad_(True), ren), (ref, ren.clone().requires_grad_(True))):
            with pytest.raises(ValueError, match="forward"):
                call(a, b)
        with torch.no_grad(), pytest.raises(_lib.NqaError):  # (without autograd the flag does not matter: the CPU refusal)
            call(ref.clone().requires_grad_(True), ren)
    with pytest.raises(ValueError):
        video.score_videos(ref, [ref, ref], dm, shared_pyramid=True)  # one pyramid for both metrics needs both models


def test_score_videos_new_arguments_are_keyword_only_and_off():
    from nerf_qa_amd import video
    sig = inspect.signature(video.score_videos)
    names = list(sig.parameters)
    assert names[-2:] == ["adists_model", "shared_pyramid"]
    assert names[:-2] == ["ref", "renders", "dists_model", "batch_size", "group", "policy", "keep_aspect_ratio", "suffix",
                          "with_frame_bias", "return_frame_scores"]
    for n, default in (("adists_model", None), ("shared_pyramid", False)):
        p = sig.parameters[n]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is default, n
    assert all(sig.parameters[n].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for n in names[:-2])
