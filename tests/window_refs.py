"""Plain-torch replay of ONE stage of the A-DISTS heavy pass (nqa_adists_window_stage, include/nqa.h), the inputs and
the case list of tests/test_gpu_adists_window.py, the check both test files share, and deliberately wrong replays.

`stage` follows win_row of nqa_adists.hip, which is ADISTS.py:84-86,165-183 with F.normalize folded into the per-channel
scalars inv_x, inv_y: window means of the RAW maps, then
    gamma = mean_c (m2 - m0^2) / (m0 + 1e-12),   tw = sum_c w_c T_c,   sw = sum_c w_c S_c,
    T = (2 mx my + 1e-6) / (mx^2 + my^2 + 1e-6),  S = (2 cov + 1e-6) / (vx + vy + 1e-6),
    mx = inv_x m0, my = inv_y m1, vx = inv_x^2 m2 - mx^2, vy = inv_y^2 m3 - my^2, cov = inv_x inv_y m4 - mx my.
float64 is the reference; float32 is the yardstick whose own distance from the reference sets the GPU test's bound."""
import math
import zlib
from collections import namedtuple

import torch

WIN = 21
FLOOR = 16 * 2.0 ** -24  # 16 float32 roundings of the map's maximum: the floor tests/test_gpu_grad_chain.py uses (~1e-6)
YARD = 8                 # a HIP chain may sit this many times as far from float64 as the float32 replay does (ibid.)

# the kernels' compile-time taps (kG of nqa_adists.hip); taps() must rebuild them bit for bit
KG_HEX = ("0x1.8453aep-6", "0x1.d76892p-6", "0x1.185a34p-5", "0x1.46b8bap-5", "0x1.75117ap-5", "0x1.a16246p-5",
          "0x1.c987c2p-5", "0x1.eb6810p-5", "0x1.02907ep-4", "0x1.0a9a20p-4", "0x1.0d5620p-4")


def taps(dtype):
    """gaussian(21, 7) as make_gauss builds it: float32(exp), a float32-rounded sum, float32 quotients; then cast."""
    v = torch.tensor([math.exp(-((i - 10) ** 2) / (2.0 * 7.0 * 7.0)) for i in range(WIN)], dtype=torch.float64).float()
    s = v.double().sum().float()
    return (v / s).to(dtype)


def window_mean(t, gv, gh):
    """Valid correlation of (B,C,H,W) with the outer product gv gh^T: a column pass and a row pass of shifted slices (the
    form of head._window_mean, with the two 1-D windows kept apart so that a mutant can disturb one)."""
    n = gv.numel()
    h, w = t.shape[2] - n + 1, t.shape[3] - n + 1
    col = gv[0] * t[:, :, 0:h, :]
    for i in range(1, n):
        col = col + gv[i] * t[:, :, i:i + h, :]
    out = gh[0] * col[:, :, :, 0:w]
    for i in range(1, n):
        out = out + gh[i] * col[:, :, :, i:i + w]
    return out


def _shift_left(t):
    """Every window one column to the right of its place; the last one reads column W-1 twice (the clamped pixel)."""
    return torch.cat([t[..., 1:], t[..., -1:]], dim=-1)


MUTANTS = {
    "a": "vertical taps rotated by one ring phase",
    "b": "window shifted one column",
    "c": "last live column computed from the clamped pixel",
    "d": "image b > 0 uses image 0's q / wgt",
    "e": "channels >= 64 dropped",
    "f": "gamma divided by 64 instead of C",
    "g": "rows >= 64 of a strip keep only the last channel block",
    "h": "y taps read from x",
    "i": "one output row of a strip's last group left unwritten",
}


def mutant_applies(m, case):
    windowed = case.H >= WIN and case.W >= WIN
    if m == "d":
        return case.B > 1
    if m in ("e", "f"):
        return case.C > 64
    if m == "g":
        return windowed and case.C > 64 and case.strip > 64
    if m == "h":
        return True
    return windowed


def stage(x, y, q, wgt, dtype, mutant=None, strip=0):
    """(gamma, tw, sw), each (B, H-20, W-20) -- (B, 1, 1) from rows 3..7 of q when H or W is under 21 -- in `dtype`.
    x, y: (B,C,H,W) holding the values the kernel reads (16-bit taps as their rounded values); q (8,B,C), wgt (B,C).
    `mutant`: one of MUTANTS, a one-line departure; `strip` (0 = the whole map) is the strip height g and i refer to."""
    x, y, q, wgt = x.to(dtype), y.to(dtype), q.to(dtype), wgt.to(dtype)
    B, C, H, W = x.shape
    if mutant == "d":
        q, wgt = q[:, :1].expand_as(q), wgt[:1].expand_as(wgt)
    if mutant == "h":
        y = x
        q = torch.cat([q[:4], q[3:4], q[5:6], q[5:6], q[5:6]])  # (the global branch's y moments are x's too)
    ix, iy, w = q[0][:, :, None, None], q[1][:, :, None, None], wgt[:, :, None, None]
    windowed = H >= WIN and W >= WIN

    def terms(x, y, gv, gh):
        if windowed:
            m0, m1, m2, m3, m4 = (window_mean(t, gv, gh) for t in (x, y, x * x, y * y, x * y))
            gt = (m2 - m0 * m0) / (m0 + 1e-12)
            mx, my = ix * m0, iy * m1
            vx, vy, cov = ix * ix * m2 - mx * mx, iy * iy * m3 - my * my, ix * iy * m4 - mx * my
        else:
            rmx, rmy, rvx, rvy, rcov = (q[j][:, :, None, None] for j in range(3, 8))
            gt = rvx / (rmx + 1e-12)
            mx, my = ix * rmx, iy * rmy
            vx, vy, cov = ix * ix * rvx, iy * iy * rvy, ix * iy * rcov
        return gt, w * ((2 * mx * my + 1e-6) / (mx * mx + my * my + 1e-6)), w * ((2 * cov + 1e-6) / (vx + vy + 1e-6))

    def reduce(gt, tt, ss, lo=0):
        keep = slice(lo, 64 if mutant == "e" else None)
        return (gt[:, keep].sum(1) / (64 if mutant == "f" else C), tt[:, keep].sum(1), ss[:, keep].sum(1))

    g = taps(dtype)
    gv = torch.roll(g, 1) if mutant == "a" else g
    if mutant == "b" and windowed:
        out = reduce(*terms(_shift_left(x), _shift_left(y), gv, g))
    else:
        out = reduce(*terms(x, y, gv, g))
    out = [o.clone() for o in out]
    if mutant == "c":
        for o, s in zip(out, reduce(*terms(_shift_left(x), _shift_left(y), gv, g))):
            o[:, :, -1] = s[:, :, -1]
    Ho = out[0].shape[1]
    strip = strip or Ho
    if mutant == "g":
        rows = [r for r in range(Ho) if r % strip >= 64]
        for o, s in zip(out, reduce(*terms(x, y, gv, g), lo=C - 64)):
            o[:, rows] = s[:, rows]
    if mutant == "i":
        for o in out:
            o[:, min(strip, Ho) - 1] = float("nan")
    return tuple(out)


# ---- the check ----------------------------------------------------------------------------------------------------
def rel_err(a, r64):
    """max|a - r64| / max|r64| of one map (all images); infinite if `a` holds a NaN (an element nobody wrote).  A map
    that is zero throughout (gamma of a 1 x 1 tap: no variance) has to come back as exact zeros."""
    a = a.detach().cpu().double()
    if torch.isnan(a).any() or a.shape != r64.shape:
        return float("inf")
    d, top = float((a - r64).abs().max()), float(r64.abs().max())
    if top == 0.0:
        return 0.0 if d == 0.0 else float("inf")
    return d / top


def bound(e32, family="A"):
    """The GPU test's bound on rel_err for a map whose float32 replay sits at e32.  Family B (scalars as the pipeline
    makes them) takes the yardstick-relative part alone."""
    return YARD * e32 if family == "B" else max(YARD * e32, FLOOR)


def check(outs, r64s, e32s, family="A"):
    """[(error, bound)] for (gamma, tw, sw) and whether all three pass."""
    figs = [(rel_err(o, r), bound(e, family)) for o, r, e in zip(outs, r64s, e32s)]
    return figs, all(err <= b for err, b in figs)


# ---- cases --------------------------------------------------------------------------------------------------------
# kind: which kernel the dispatch must reach.  prec: the entry point's mode.  strip: forced strip height (0 = launcher's).
# legacy: run under set_conv_variant(DEFAULT | 8).  grid: (nbx, nby, strip) the launcher must report, where asserted.
Case = namedtuple("Case", "kind prec B C H W strip legacy family grid")


def _c(kind, prec, B, C, H, W, strip=0, legacy=False, family="A", grid=None):
    return Case(kind, prec, B, C, H, W, strip, legacy, family, grid)


def case_id(c):
    return (f"{c.kind}-{c.prec}{'-first' if c.legacy else ''}-B{c.B}-C{c.C}-{c.H}x{c.W}"
            f"{'-s%d' % c.strip if c.strip else ''}-{c.family}")


def _cases():
    out = []
    # LDS kernel, float taps, the launcher's strips: Ho in {1, 2, 7, 21, 43, 64, 65}, Wo in {1, 2, 3, 4, 5, 10, 24}
    for C in (64, 128, 256, 512):
        out += [_c("lds", "f32", 1, C, 21, 21), _c("lds", "f32s", 1, C, 22, 25), _c("lds", "f32", 1, C, 27, 30)]
    out += [_c("lds", "f32", 1, 64, 41, 44), _c("lds", "f32", 1, 64, 63, 24), _c("lds", "f32", 1, 64, 84, 22),
            _c("lds", "f32", 1, 64, 85, 23)]
    # forced strips: groups of 64 + 6 rows over two channel blocks; exactly 64; 33 + 33 + 4; one row per block;
    # three groups (64, 64, 22) in one strip; 64 + 64 + 2 over four channel blocks
    out += [_c("lds", "f32", 1, 128, 90, 23, 70, grid=(1, 1, 70)), _c("lds", "f32", 1, 128, 90, 23, 64, grid=(1, 2, 64)),
            _c("lds", "f32", 2, 128, 90, 23, 33, grid=(1, 3, 33)), _c("lds", "f32", 1, 128, 90, 23, 1, grid=(1, 70, 1)),
            _c("lds", "f32", 1, 64, 170, 22, 150, grid=(1, 1, 150)), _c("lds", "f32", 1, 256, 150, 21, 130, grid=(1, 1, 130))]
    # grid sizes for the workgroup-id remap: 1, 6, 8, 9, 20 blocks
    out += [_c("lds", "f32", 1, 64, 21, 22, grid=(1, 1, 1)), _c("lds", "f32", 3, 64, 25, 25, grid=(2, 1, 5)),
            _c("lds", "f32", 2, 64, 22, 36, grid=(4, 1, 2)), _c("lds", "f32", 3, 64, 23, 29, grid=(3, 1, 3)),
            _c("lds", "f32", 2, 64, 90, 38, grid=(5, 2, 35))]
    # the first form: 16-bit taps, and float taps under the variant bit; Ho = 65 and 70 reach the second blockIdx.y
    for prec, legacy in (("f16", False), ("bf16", False), ("f32", True)):
        for C in (64, 256):
            out += [_c("lanes", prec, 1, C, 21, 21, legacy=legacy), _c("lanes", prec, 1, C, 22, 25, legacy=legacy),
                    _c("lanes", prec, 2, C, 85, 23, legacy=legacy), _c("lanes", prec, 1, C, 90, 24, legacy=legacy)]
    # planar kernel: Wo in {1, 63, 64, 65, 10, 257, 280}, Ho on both sides of 64
    for B, H, W in ((1, 21, 21), (1, 22, 83), (1, 22, 84), (2, 22, 85), (1, 84, 30), (1, 85, 30), (1, 22, 277), (1, 30, 300)):
        out.append(_c("planar", "f32", B, 3, H, W))
    # global branch
    for H, W in ((1, 1), (5, 7), (20, 50), (50, 20)):
        for C in (3, 64, 512):
            out.append(_c("global", "f32", 3, C, H, W))
    # families B (scalars as the pipeline makes them) and C (exact zeros) on one shape of every kernel
    for fam in ("B", "C"):
        out += [_c("lds", "f32", 1, 64, 41, 44, family=fam), _c("lds", "f32", 1, 512, 27, 30, family=fam),
                _c("lds", "f32", 2, 128, 90, 27, 70, family=fam), _c("lanes", "f16", 1, 64, 90, 26, family=fam),
                _c("lanes", "f32", 2, 256, 85, 25, legacy=True, family=fam), _c("planar", "f32", 2, 3, 85, 30, family=fam),
                _c("planar", "f32", 1, 3, 30, 300, family=fam), _c("global", "f32", 3, 64, 20, 50, family=fam)]
    assert len({case_id(c) for c in out}) == len(out)
    return out


CASES = _cases()
STORAGE = {"f32": torch.float32, "f32s": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def inputs(case):
    """(x, y, q, wgt) of a case from a fixed seed.  x, y: (B,C,H,W) in the tap's storage type, x = relu(4u - 2) + a smooth
    ramp, y = relu(x + 0.5 n); q (8,B,C) and wgt (B,C) float32, different for every image."""
    gen = torch.Generator().manual_seed(zlib.crc32(case_id(case).encode()))
    B, C, H, W = case.B, case.C, case.H, case.W
    ramp = 0.5 * (torch.arange(H, dtype=torch.float32)[:, None] / H + torch.arange(W, dtype=torch.float32)[None, :] / W)
    scale = 0.5 + torch.rand((B, C, 1, 1), generator=gen)  # channels of different size, as a tap's are
    x = scale * (torch.relu(4 * torch.rand((B, C, H, W), generator=gen) - 2) + ramp)
    y = torch.relu(x + 0.5 * scale * torch.randn((B, C, H, W), generator=gen))
    if case.family == "C":  # exact zeros only: a dead channel of x, one dead in both, a zero patch in a live channel
        x[:, 1] = 0
        x[:, 2] = 0
        y[:, 2] = 0
        x[:, 0, 1:26, 2:27] = 0
        y[:, 0, 1:26, 2:27] = 0
    x, y = x.to(STORAGE[case.prec]), y.to(STORAGE[case.prec])
    xd, yd = x.double(), y.double()
    mx, my = xd.mean((2, 3)), yd.mean((2, 3))
    q = torch.empty((8, B, C), dtype=torch.float64)
    if case.family == "B":
        q[0] = 1 / xd.pow(2).sum((2, 3)).sqrt().clamp_min(1e-12)
        q[1] = 1 / yd.pow(2).sum((2, 3)).sqrt().clamp_min(1e-12)
    else:
        q[0] = 0.5 + 1.5 * torch.rand((B, C), generator=gen, dtype=torch.float64)
        q[1] = 0.5 + 1.5 * torch.rand((B, C), generator=gen, dtype=torch.float64)
    q[2] = xd.sum((2, 3))
    q[3], q[4] = mx, my
    q[5] = xd.pow(2).mean((2, 3)) - mx * mx
    q[6] = yd.pow(2).mean((2, 3)) - my * my
    q[7] = (xd * yd).mean((2, 3)) - mx * my
    wgt = 0.1 + torch.rand((B, C), generator=gen, dtype=torch.float64)
    wgt = wgt / wgt.sum(1, keepdim=True)
    return x, y, q.float(), wgt.float()


def references(case):
    """(inputs, r64 maps, e32 per map) of a case."""
    x, y, q, wgt = inputs(case)
    r64 = stage(x, y, q, wgt, torch.float64)
    r32 = stage(x, y, q, wgt, torch.float32)
    return (x, y, q, wgt), r64, tuple(rel_err(a, r) for a, r in zip(r32, r64))
