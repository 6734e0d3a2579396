"""CPU-side checks of the score-map entry point at the C boundary (include/nqa.h: nqa_score_maps_workspace_bytes,
nqa_score_maps): declared in the header, exported by the library, bound by _lib.py, built from its own source; the
workspace's size is positive where the call runs and 0 where it refuses; and every refusal is reached on the host, with
its code and a message under the function's name -- never a launch (no device is touched here: the pointers below are
made-up numbers)."""
import json
import os
import re

import pytest

NEW = ("nqa_score_maps_workspace_bytes", "nqa_score_maps")
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "nqa.h")
E_ARG, E_WORKSPACE = -1, -3
P = [0x100000 + 0x1000 * i for i in range(4)]  # fake device pointers: nothing below may dereference them
F, K, H, W = 3, 4, 37, 53

# (F, K, H, W) the call refuses with NQA_E_ARG, and what its message says
BAD_SIZES = [((0, K, H, W), b"non-positive size"), ((-1, K, H, W), b"non-positive size"), ((F, 0, H, W), b"non-positive size"),
             ((F, -2, H, W), b"non-positive size"), ((F, K, 0, W), b"non-positive size"), ((F, K, H, -5), b"non-positive size"),
             ((1, 257, 8, 8), b"more than 256"), ((1, 1 << 20, 8, 8), b"more than 256"),
             ((256, 256, 8, 8), b"more than 65535"), ((65536, 1, 8, 8), b"more than 65535"), ((16384, 4, 8, 8), b"more than 65535"),
             ((1, 1, 1 << 15, 1 << 15), b"2^31"), ((1, 8, 9473, 9473), b"2^31"), ((1, 1, 26755, 26755), b"2^31"),
             ((65535, 1, 105, 105), b"2^31"), ((1, 1, 1 << 16, 1 << 16), b"2^31")]


@pytest.fixture(scope="module")
def lib():
    from nerf_qa_amd import build, _lib
    build.build()
    return _lib.lib()


def _err(lib):
    return lib.nqa_last_error()


def _call(lib, maps=P[0], f=F, k=K, h=H, w=W, ws=P[1], ws_bytes=1 << 40, rgb=P[2], logs=P[3]):
    return lib.nqa_score_maps(maps, f, k, h, w, ws, ws_bytes, rgb, logs, None)


def test_exports_are_declared_bound_built_and_present(lib):
    from nerf_qa_amd import _lib, build
    text = open(HEADER).read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, text), name
        assert name in _lib.EXPORTS and getattr(lib, name) is not None, name
    assert "#define NQA_VERSION 1" in text and lib.nqa_version() == 1  # the ABI only grows
    assert "NQA_K_COUNT = 7" in text  # the three launches are counted under the existing NQA_K_PREP
    assert "nqa_score_maps.hip" in build.SOURCES
    res = json.load(open(build.RESOURCES))
    for kernel in ("score_maps_moments_kernel", "score_maps_fold_kernel", "score_maps_quantise_kernel"):
        hit = [r for name, r in res.items() if kernel in name]
        assert len(hit) == 1 and hit[0]["scratch"] == 0, kernel


def test_workspace_bytes(lib):
    nb = lib.nqa_score_maps_workspace_bytes
    for shape in ((1, 1, 1, 1), (1, 1, 8, 8), (1, 2, 24, 31), (1, 5, 67, 131), (3, 4, 37, 53), (1, 8, 756, 1344),
                  (1, 256, 8, 8), (255, 256, 1, 1), (65535, 1, 8, 8)):
        f, k, h, w = shape
        assert nb(*shape) > 0, shape
        assert nb(*shape) % 256 == 0
        assert nb(*shape) >= 2 * f * h * w * 8 + f * (k + 2) * 2 * 8, shape  # the two fp64 maps and one partial pair per quantity
    sizes = [nb(f, 4, 37, 53) for f in (1, 2, 3, 8, 64)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1]
    for shape, msg in BAD_SIZES:
        assert nb(*shape) == 0, shape
        assert b"score_maps_workspace_bytes: " in _err(lib) and msg in _err(lib), (shape, _err(lib))


def test_refuses_bad_arguments(lib):
    who = b"score_maps: "
    for kw in ({"maps": None}, {"ws": None}, {"rgb": None}, {"logs": None}):
        assert _call(lib, **kw) == E_ARG, kw
        assert who + b"null pointer" in _err(lib), _err(lib)
    for (f, k, h, w), msg in BAD_SIZES:
        assert _call(lib, f=f, k=k, h=h, w=w) == E_ARG, (f, k, h, w)
        assert _err(lib).startswith(who) and msg in _err(lib), _err(lib)
    need = lib.nqa_score_maps_workspace_bytes(F, K, H, W)
    assert need > 0
    for short in (need - 1, need // 2, 0):
        assert _call(lib, ws_bytes=short) == E_WORKSPACE
        assert who + b"workspace %d < %d bytes" % (short, need) in _err(lib), _err(lib)
    # a workspace sized for fewer frames is short
    assert _call(lib, ws_bytes=lib.nqa_score_maps_workspace_bytes(F - 1, K, H, W)) == E_WORKSPACE
    # the order of the checks: a null pointer before a bad size, a bad size before the workspace
    assert _call(lib, maps=None, f=0) == E_ARG and b"null pointer" in _err(lib)
    assert _call(lib, f=0, ws_bytes=0) == E_ARG and b"non-positive" in _err(lib)
    assert _call(lib, k=257, ws_bytes=0) == E_ARG and b"more than 256" in _err(lib)


def test_the_largest_accepted_sizes_sit_at_the_stated_limits(lib):
    nb = lib.nqa_score_maps_workspace_bytes
    assert nb(1, 256, 8, 8) > 0 and nb(1, 257, 8, 8) == 0               # K <= 256
    assert nb(255, 257, 1, 1) == 0 and nb(257, 255, 1, 1) > 0           # (K first), F * K = 65535
    assert nb(256, 256, 1, 1) == 0                                       # F * K = 65536
    # F * K * H * W * 3 < 2^31: 715827882 * 3 = 2^31 - 2, 715827883 * 3 = 2^31 + 1
    assert nb(1, 1, 2, 357913941) > 0 and nb(1, 2, 1, 357913941) > 0
    assert nb(1, 1, 1, 715827883) == 0 and b"2^31" in _err(lib)
