"""The entry points without a window and their _n forms at a window of 21 are one implementation each (csrc/nqa_api.hip):
nqa_window_moments_forward / _backward, nqa_adists_ts_backward and nqa_adists_ts_backward_bytes against
nqa_window_moments_forward_n / _backward_n, nqa_adists_ts_backward_n and nqa_adists_ts_backward_bytes_n.  One table of
argument sets per operation goes through both names of a pair: the return code is the same, and so is nqa_last_error()
once the _n is taken out of the function's name.  Every case is a REFUSAL (its expected code stands in the table): the
pointers are fake, so no case may get past the host's checks, and no device is touched."""
import pytest

P = [0x10000 + 0x1000 * i for i in range(10)]  # fake, 16-byte aligned device pointers: nothing below may dereference them
E_ARG, E_SHAPE, E_WORKSPACE = -1, -2, -3
BIG = 1 << 40


@pytest.fixture(scope="module")
def lib():
    from nerf_qa_amd import build, _lib
    build.build()
    return _lib.lib()


def _both(lib, old, new, who, cases):
    """Runs every (arguments, expected code) through old(lib, **kw) and new(lib, **kw); who: the old name in messages."""
    for kw, code in cases:
        got = []
        for call, name in ((old, who), (new, who + b"_n")):
            rc = call(lib, **kw)
            err = lib.nqa_last_error()
            assert rc == code and rc != 0, (name, kw, rc, err)
            assert err.startswith(name + b": "), (name, kw, err)
            got.append((rc, who + err[len(name):]))
        assert got[0] == got[1], (kw, got)


# ---- window moments: planes, H, W and the maps; the forward's `out` and the backward's g0 .. g4, gx, gy on top ----
MOMENTS = [
    ({"x": None}, E_ARG),
    ({"planes": 0}, E_ARG), ({"planes": -3}, E_ARG),
    ({"H": 20}, E_SHAPE), ({"W": 20}, E_SHAPE), ({"H": 20, "W": 20}, E_SHAPE), ({"H": 0}, E_SHAPE), ({"W": -1}, E_SHAPE),
    # misaligned maps are refused where rows move as 16-byte accesses (W % 4 == 0) ...
    ({"x": P[0] + 4}, E_ARG), ({"y": P[1] + 8}, E_ARG), ({"x": P[0] + 4, "H": 1 << 24, "W": 84}, E_ARG),
    # ... and accepted elsewhere, up to the next refusal (the plane's size, checked after the alignment)
    ({"x": P[0] + 4, "H": 1 << 24, "W": 85}, E_SHAPE), ({"y": P[1] + 8, "H": 1 << 24, "W": 85}, E_SHAPE),
    ({"H": (1 << 20) + 1, "W": 24}, E_SHAPE), ({"H": (1 << 20) + 1, "W": 21}, E_SHAPE),   # H > 2^20
    ({"H": 1 << 16, "W": (1 << 14) + 4}, E_SHAPE), ({"H": 1 << 15, "W": (1 << 15) + 1}, E_SHAPE),  # > 2^30 pixels
]
FORWARD = MOMENTS + [({"out": None}, E_ARG), ({"out": P[2] + 12}, E_ARG),
                     ({"out": P[2] + 12, "H": 1 << 24, "W": 85}, E_SHAPE), ({"y": None, "out": P[2] + 4}, E_ARG)]
BACKWARD = MOMENTS + [
    ({"gx": None, "gy": None}, E_ARG), ({"y": None}, E_ARG), ({"y": None, "gy": None}, E_ARG),
    ({"y": None, "gy": None, "g": (P[2], P[3], P[4], None, None)}, E_ARG),
    ({"y": None, "gy": None, "g": (P[2], None, P[4], None, P[6])}, E_ARG),
    ({"gx": P[7] + 8}, E_ARG), ({"gy": P[8] + 4}, E_ARG), ({"g": (P[2], P[3], P[4] + 4, P[5], P[6])}, E_ARG),
    ({"g": (None, None, None, None, P[6] + 8)}, E_ARG),
    ({"y": None, "gy": None, "g": (P[2] + 4, None, None, None, None)}, E_ARG),
    ({"gx": P[7] + 8, "H": 1 << 24, "W": 85}, E_SHAPE),
    ({"g": (P[2] + 4, None, None, None, None), "H": 1 << 24, "W": 85}, E_SHAPE),
]


def _fwd(n):
    def call(lib, x=P[0], y=P[1], planes=6, H=40, W=56, out=P[2]):
        if n:
            return lib.nqa_window_moments_forward_n(x, y, planes, H, W, 21, out, None)
        return lib.nqa_window_moments_forward(x, y, planes, H, W, out, None)
    return call


def _bwd(n):
    def call(lib, x=P[0], y=P[1], planes=6, H=40, W=56, g=(P[2], P[3], P[4], P[5], P[6]), gx=P[7], gy=P[8]):
        if n:
            return lib.nqa_window_moments_backward_n(x, y, planes, H, W, 21, *g, gx, gy, None)
        return lib.nqa_window_moments_backward(x, y, planes, H, W, *g, gx, gy, None)
    return call


def test_moments_forward_names_agree(lib):
    _both(lib, _fwd(False), _fwd(True), b"window_moments_forward", FORWARD)


def test_moments_backward_names_agree(lib):
    _both(lib, _bwd(False), _bwd(True), b"window_moments_backward", BACKWARD)


# ---- the stage backward: the default workspace size 0 is short for every size the entry accepts ----
STAGE = [({name: None}, E_ARG) for name in ("x", "y", "q", "wgt", "ps", "u", "ws", "gy")] + [
    ({"B": 0}, E_ARG), ({"B": -1}, E_ARG), ({"C": 0}, E_ARG), ({"H": 0}, E_ARG), ({"W": -3}, E_ARG), ({"ctot": 0}, E_ARG),
    ({"coff": -1}, E_ARG), ({"ctot": 64, "coff": 1}, E_ARG), ({"ctot": 1475, "coff": 1475 - 63}, E_ARG),  # channels outside q
    ({"B": 65536}, E_ARG),                                                                               # > 65535 pairs
    ({"H": (1 << 20) + 1, "W": 21}, E_SHAPE), ({"H": 1 << 16, "W": (1 << 14) + 4}, E_SHAPE),
    ({"B": 1, "C": 3, "H": 1 << 24, "W": 85}, E_SHAPE),
    ({"B": 65535, "C": 512, "H": 1 << 10, "W": 1 << 10}, E_SHAPE),  # more blocks than one launch takes
    # NHWC with C % 32 != 0: refused on a windowed stage, accepted on a global one (H or W of 20) up to the workspace
    ({"C": 3, "nhwc": 1}, E_SHAPE), ({"C": 3, "nhwc": 1, "H": 21, "W": 24}, E_SHAPE),
    ({"C": 3, "nhwc": 1, "H": 20}, E_WORKSPACE), ({"C": 3, "nhwc": 1, "W": 20}, E_WORKSPACE),
    # the workspace always, the maps on a windowed stage with W % 4 == 0
    ({"ws": P[6] + 8}, E_ARG), ({"ws": P[6] + 8, "W": 57}, E_ARG), ({"ws": P[6] + 8, "H": 16, "W": 16}, E_ARG),
] + [c for name, p in (("x", P[0] + 4), ("y", P[1] + 8), ("ps", P[4] + 12), ("gy", P[7] + 4)) for c in (
    ({name: p}, E_ARG), ({name: p, "W": 57}, E_WORKSPACE), ({name: p, "H": 16, "W": 16}, E_WORKSPACE),
    ({name: p, "H": 20}, E_WORKSPACE))] + [
    ({"q": P[2] + 4}, E_WORKSPACE), ({"wgt": P[3] + 4}, E_WORKSPACE), ({"u": P[5] + 4}, E_WORKSPACE),
    ({}, E_WORKSPACE), ({"short_by": 1}, E_WORKSPACE), ({"B": 1, "C": 3, "H": 21, "W": 21, "short_by": 1}, E_WORKSPACE),
    ({"B": 1, "C": 512, "H": 3, "W": 4, "short_by": 1}, E_WORKSPACE), ({"W": 57, "short_by": 16}, E_WORKSPACE),
]


def _ts(n):
    def call(lib, x=P[0], y=P[1], B=2, C=64, H=40, W=56, q=P[2], wgt=P[3], ctot=None, coff=0, ps=P[4], u=P[5], mask=1, nhwc=0,
             ws=P[6], short_by=None, gy=P[7]):
        ctot = C if ctot is None else ctot
        # short_by: a workspace that many bytes under what the stage needs (each name asked by its own query)
        need = lib.nqa_adists_ts_backward_bytes_n(B, C, H, W, 21) if n else lib.nqa_adists_ts_backward_bytes(B, C, H, W)
        ws_bytes = 0 if short_by is None else need - short_by
        assert short_by is None or 0 <= ws_bytes < need
        if n:
            return lib.nqa_adists_ts_backward_n(x, y, B, C, H, W, 21, q, wgt, ctot, coff, ps, u, mask, nhwc, ws, ws_bytes, gy,
                                                None)
        return lib.nqa_adists_ts_backward(x, y, B, C, H, W, q, wgt, ctot, coff, ps, u, mask, nhwc, ws, ws_bytes, gy, None)
    return call


def test_stage_backward_names_agree(lib):
    _both(lib, _ts(False), _ts(True), b"adists_ts_backward", STAGE)


def test_stage_backward_bytes_names_agree(lib):
    old, new = lib.nqa_adists_ts_backward_bytes, lib.nqa_adists_ts_backward_bytes_n
    windowed = [(40, 56), (21, 21), (22, 37), (21, 64), (57, 21)]
    glob = [(20, 56), (40, 20), (20, 20), (13, 17), (3, 4)]
    for B in (1, 2, 7):
        for C in (3, 64, 512):
            for H, W in windowed + glob:
                a, b = old(B, C, H, W), new(B, C, H, W, 21)
                assert a == b, (B, C, H, W, a, b)
                assert (a > 16 and a % 16 == 0) if (H, W) in windowed else a == 16, (B, C, H, W, a)
    for args in ((0, 64, 40, 56), (2, 0, 40, 56), (2, 64, 0, 56), (2, 64, 40, -1), (65536, 64, 40, 56),
                 (1, 3, 1 << 16, (1 << 14) + 4), (1, 3, (1 << 20) + 1, 21), (65535, 512, 1 << 10, 1 << 10)):
        assert old(*args) == 0 == new(*args, 21), args
