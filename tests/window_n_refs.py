"""Plain-torch replay of ONE stage of the A-DISTS heavy pass for a general window size n (nqa_adists_window_stage_n and
its group form, include/nqa.h), the inputs and the case list of tests/test_gpu_adists_window_n.py, and deliberately
wrong replays.  The form is window_refs.stage's (which hard-wires the 21-tap window and stays as it is): window means of
the RAW maps by a column pass and a row pass of shifted slices, then gamma, T and S; at n = 21 the two are the same
operations in the same order, bit for bit.  The taps are rebuilt as the host builds them (gauss_n of nqa_adists.hip):
float32 of exp(-(i - n // 2)^2 / (2 (n / 3)^2)), a float32-rounded sum, float32 quotients -- centre n // 2, so an even
window is not symmetric.  float64 is the reference; float32 is the yardstick whose own distance from the reference
sets the GPU test's bound (window_refs.bound: max(8 x e32, 16 x 2^-24))."""
import math
import zlib
from collections import namedtuple

import torch

import window_refs as R21

WMIN, WMAX = 3, 63


def taps(n, dtype, sigma=None):
    """gaussian(n, n / 3) as the host builds it; `sigma` replaces n / 3 (a mutant)."""
    sigma = n / 3 if sigma is None else sigma
    v = torch.tensor([math.exp(-((i - n // 2) ** 2) / (2.0 * sigma * sigma)) for i in range(n)], dtype=torch.float64).float()
    s = v.double().sum().float()
    return (v / s).to(dtype)


def table_row(m, n, dtype):
    """The first n entries of the host table's row for a window of m (taps of m, zeros behind them): what a kernel
    handed the wrong row would use."""
    g = taps(m, dtype)
    return g[:n] if m >= n else torch.cat([g, torch.zeros(n - m, dtype=dtype)])


MUTANTS = {
    "n-1": "taps of n - 1",
    "n+1": "taps of n + 1",
    "sigma7": "sigma 7 instead of n / 3",
    "rot": "vertical taps rotated by one",
    "shift": "window shifted one column",
    "yx": "y read from x",
    "img0": "image 0's q / wgt used for image 1",
    "mirror": "an even window mirrored",
}


def mutant_applies(m, case):
    windowed = case.H >= case.n and case.W >= case.n
    if m == "img0":
        return case.B > 1
    if m == "yx":
        return True
    if m == "sigma7":
        return windowed and case.n != 21
    if m == "mirror":
        return windowed and case.n % 2 == 0
    if m == "n-1":
        return windowed and case.n - 1 >= WMIN
    if m == "n+1":
        return windowed and case.n + 1 <= WMAX
    return windowed


def stage(x, y, q, wgt, n, dtype, mutant=None):
    """(gamma, tw, sw), each (B, H-n+1, W-n+1) -- (B, 1, 1) from rows 3..7 of q when H or W is under n -- in `dtype`.
    x, y: (B,C,H,W) holding the values the kernel reads; q (8,B,C), wgt (B,C).  `mutant`: one of MUTANTS."""
    x, y, q, wgt = x.to(dtype), y.to(dtype), q.to(dtype), wgt.to(dtype)
    B, C, H, W = x.shape
    if mutant == "img0":
        q, wgt = q[:, :1].expand_as(q), wgt[:1].expand_as(wgt)
    if mutant == "yx":
        y = x
        q = torch.cat([q[:4], q[3:4], q[5:6], q[5:6], q[5:6]])  # (the global branch's y moments are x's too)
    ix, iy, w = q[0][:, :, None, None], q[1][:, :, None, None], wgt[:, :, None, None]
    windowed = H >= n and W >= n
    if windowed:
        if mutant == "n-1":
            g = table_row(n - 1, n, dtype)
        elif mutant == "n+1":
            g = table_row(n + 1, n, dtype)
        elif mutant == "sigma7":
            g = taps(n, dtype, sigma=7.0)
        elif mutant == "mirror":
            g = taps(n, dtype).flip(0)
        else:
            g = taps(n, dtype)
        gv = torch.roll(g, 1) if mutant == "rot" else g
        if mutant == "shift":
            x, y = R21._shift_left(x), R21._shift_left(y)
        m0, m1, m2, m3, m4 = (R21.window_mean(t, gv, g) for t in (x, y, x * x, y * y, x * y))
        gt = (m2 - m0 * m0) / (m0 + 1e-12)
        mx, my = ix * m0, iy * m1
        vx, vy, cov = ix * ix * m2 - mx * mx, iy * iy * m3 - my * my, ix * iy * m4 - mx * my
    else:
        rmx, rmy, rvx, rvy, rcov = (q[j][:, :, None, None] for j in range(3, 8))
        gt = rvx / (rmx + 1e-12)
        mx, my = ix * rmx, iy * rmy
        vx, vy, cov = ix * ix * rvx, iy * iy * rvy, ix * iy * rcov
    tt, ss = w * ((2 * mx * my + 1e-6) / (mx * mx + my * my + 1e-6)), w * ((2 * cov + 1e-6) / (vx + vy + 1e-6))
    return tuple(o.clone() for o in (gt.sum(1) / C, tt.sum(1), ss.sum(1)))


def moments(x, y, n, dtype):
    """The five window means of stage(), on their own (compared with the oracle's F.conv2d in test_window_n_refs.py)."""
    g = taps(n, dtype)
    x, y = x.to(dtype), y.to(dtype)
    return tuple(R21.window_mean(t, g, g) for t in (x, y, x * x, y * y, x * y))


# ---- cases --------------------------------------------------------------------------------------------------------
# kind: which kernel the dispatch must reach (lanes / planar: the generic kernels; global: the global branch).  B pairs;
# K > 0: the group form, B = R * K pairs of R = B / K references.  generic: run under set_conv_variant(DEFAULT | 2048)
# (a window of 21 on the generic kernels).  strip: forced strip height (0 = the launcher's).
Case = namedtuple("Case", "kind prec n B C H W strip K generic")


def _c(kind, prec, n, B, C, H, W, strip=0, K=0):
    return Case(kind, prec, n, B, C, H, W, strip, K, n == 21)


def case_id(c):
    return (f"{c.kind}-n{c.n}-{c.prec}-B{c.B}-C{c.C}-{c.H}x{c.W}{'-s%d' % c.strip if c.strip else ''}"
            f"{'-K%d' % c.K if c.K else ''}")


def _cases():
    out = []
    # NHWC, float taps.  A block of the lanes kernel covers ONE output column and a strip of (at these grid sizes) 64
    # rows: Ho = 65 is one row more, every Wo > 1 one column more.  n in {3, 4, 12, 21, 33, 63}, C in {64, 128}, B = 2
    out += [_c("lanes", "f32", 3, 2, 64, 67, 6), _c("lanes", "f32", 4, 2, 128, 20, 9), _c("lanes", "f32s", 12, 2, 64, 30, 17),
            _c("lanes", "f32", 21, 2, 128, 85, 23), _c("lanes", "f32", 33, 2, 64, 40, 35), _c("lanes", "f32", 63, 2, 64, 70, 66),
            _c("lanes", "f32", 63, 1, 128, 96, 112)]
    # H = n exactly (a one-row map), W = n exactly (a one-column map), both (one element)
    out += [_c("lanes", "f32", 12, 2, 64, 12, 20), _c("lanes", "f32", 12, 2, 64, 20, 12), _c("lanes", "f32", 63, 1, 64, 63, 63),
            _c("lanes", "f32", 4, 1, 128, 4, 4)]
    # forced strips: groups of 64 + 6 rows over two channel blocks and a second strip; exactly 64; one row per block
    out += [_c("lanes", "f32", 12, 1, 128, 90, 14, 70), _c("lanes", "f32", 12, 2, 128, 90, 14, 64),
            _c("lanes", "f32", 4, 1, 128, 20, 9, 1), _c("lanes", "f32", 33, 1, 64, 170, 34, 138)]
    # 16-bit taps
    out += [_c("lanes", "f16", 4, 2, 128, 24, 10), _c("lanes", "f16", 33, 2, 64, 40, 36), _c("lanes", "f16", 21, 2, 64, 85, 23),
            _c("lanes", "bf16", 3, 2, 64, 67, 5), _c("lanes", "bf16", 12, 2, 128, 30, 17), _c("lanes", "bf16", 63, 1, 64, 70, 65)]
    # planes: a block covers 64 columns and a strip of 64 rows; Wo in {1, 64, 65, 68}, Ho on both sides of 64
    out += [_c("planar", "f32", 3, 2, 3, 67, 67), _c("planar", "f32", 4, 2, 3, 24, 31), _c("planar", "f32", 12, 2, 3, 30, 75),
            _c("planar", "f32", 21, 2, 3, 85, 85), _c("planar", "f32", 33, 2, 3, 40, 100), _c("planar", "f32", 63, 2, 3, 72, 130),
            _c("planar", "f32", 12, 1, 3, 12, 40), _c("planar", "f32", 12, 1, 3, 40, 12), _c("planar", "f32", 4, 1, 3, 90, 9, 70)]
    # the group forms, K = 3 renders of R = 2 references
    out += [_c("lanes", "f32", 12, 6, 128, 30, 17, K=3), _c("lanes", "f16", 33, 6, 64, 40, 36, K=3),
            _c("lanes", "f32", 21, 6, 64, 85, 23, K=3), _c("lanes", "f32", 4, 6, 128, 90, 9, 70, K=3),
            _c("planar", "f32", 4, 6, 3, 24, 31, K=3), _c("planar", "f32", 21, 6, 3, 85, 85, K=3),
            _c("planar", "f32", 63, 6, 3, 72, 130, K=3)]
    # H = n - 1 or W = n - 1: the global branch, pair and group
    out += [_c("global", "f32", 12, 2, 64, 11, 30), _c("global", "f32", 63, 2, 3, 70, 62), _c("global", "f32", 4, 2, 128, 3, 9),
            _c("global", "f16", 33, 2, 64, 32, 40), _c("global", "f32", 33, 6, 64, 32, 40, K=3)]
    assert len({case_id(c) for c in out}) == len(out)
    assert all(c.H * c.W * c.C <= 96 * 112 * 128 for c in out)
    return out


CASES = _cases()
STORAGE = R21.STORAGE


def inputs(case):
    """(x, y, q, wgt) of a case from a fixed seed, by window_refs.inputs' recipe: x = relu(4u - 2) + a smooth ramp,
    y = relu(x + 0.5 n), channels of different size; q (8,B,C) and wgt float32, different for every image.  Group cases:
    x (R,C,H,W) and wgt (R,C) per reference, y and q per pair."""
    gen = torch.Generator().manual_seed(zlib.crc32(case_id(case).encode()))
    B, C, H, W = case.B, case.C, case.H, case.W
    X = B // case.K if case.K else B
    ramp = 0.5 * (torch.arange(H, dtype=torch.float32)[:, None] / H + torch.arange(W, dtype=torch.float32)[None, :] / W)
    scale = 0.5 + torch.rand((X, C, 1, 1), generator=gen)
    x = scale * (torch.relu(4 * torch.rand((X, C, H, W), generator=gen) - 2) + ramp)
    xp, sp = pair_rows(x, case), pair_rows(scale, case)
    y = torch.relu(xp + 0.5 * sp * torch.randn((B, C, H, W), generator=gen))
    x, y = x.to(STORAGE[case.prec]), y.to(STORAGE[case.prec])
    xd, yd = pair_rows(x, case).double(), y.double()
    mx, my = xd.mean((2, 3)), yd.mean((2, 3))
    q = torch.empty((8, B, C), dtype=torch.float64)
    q[0] = 0.5 + 1.5 * torch.rand((B, C), generator=gen, dtype=torch.float64)
    q[1] = 0.5 + 1.5 * torch.rand((B, C), generator=gen, dtype=torch.float64)
    q[2] = xd.sum((2, 3))
    q[3], q[4] = mx, my
    q[5] = xd.pow(2).mean((2, 3)) - mx * mx
    q[6] = yd.pow(2).mean((2, 3)) - my * my
    q[7] = (xd * yd).mean((2, 3)) - mx * my
    wgt = 0.1 + torch.rand((X, C), generator=gen, dtype=torch.float64)
    wgt = wgt / wgt.sum(1, keepdim=True)
    return x, y, q.float(), wgt.float()


def pair_rows(t, case):
    """A per-reference tensor with one row per pair (pair b reads reference b // K); itself for pairwise cases."""
    return t.repeat_interleave(case.K, dim=0) if case.K else t


def replay(case, ins, dtype, mutant=None):
    """stage() of a case's inputs; a group case's gamma comes back per reference, as the kernels write it."""
    x, y, q, wgt = ins
    g, t, s = stage(pair_rows(x, case), y, q, pair_rows(wgt, case), case.n, dtype, mutant)
    return (g[::case.K] if case.K else g), t, s


def references(case):
    """(inputs, r64 maps, e32 per map) of a case."""
    ins = inputs(case)
    r64 = replay(case, ins, torch.float64)
    r32 = replay(case, ins, torch.float32)
    return ins, r64, tuple(R21.rel_err(a, r) for a, r in zip(r32, r64))
