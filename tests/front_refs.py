"""Plain-torch replay of the FRONT part of the A-DISTS forward (nqa_adists_front, include/nqa.h): from the images and the
five tapped maps to the per-channel scalars q, the folded entropies hsum and the channel weights wgt; the inputs and the
case list of tests/test_gpu_adists_front.py, the check both test files share, and deliberately wrong replays.

`front` follows the reference's expressions: per (image, channel) of the RAW maps
    inv = 1 / max(||f||_2, 1e-12)                       (F.normalize's scalar, ADISTS.py:130,166-167)
    mean, population variance as mean((f - mean)^2), covariance as mean(f g) - mean_f mean_g      (:176-180)
    p = relu(f) inv;  p /= sum(p) + 1e-12;  hsum = -sum p log2(p + 1e-12)                        (:127-133)
    per stage hsum / (sum_c hsum + 1e-12) * C; all 1475: / sum, clamp to mean +- 0.5 population std, / sum  (:134-135,150-160)
float64 is the reference; float32 is the yardstick whose own distance from the reference sets the bound on hsum and wgt.
The planning functions below are ports of stats_units_per_block, stats_nchw_ppb and pool_stats_tiles (nqa_pool_stats.hip);
tests/test_cpu_adists_front_abi.py holds the library's grid query to them."""
import zlib
from collections import namedtuple

import torch

from window_refs import FLOOR, YARD, rel_err

CHNS = (3, 64, 128, 256, 512, 512)
COFF = (0, 3, 67, 195, 451, 963)
CTOT = 1475
STORAGE = {"f32": torch.float32, "f32s": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
C0 = 1e-12


# ---- the launch plan (ports of the host functions) ---------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def stats_units_per_block(units, C, prec, B):
    cpc = 4 if STORAGE[prec] == torch.float32 else 8
    PL = 256 // (C // cpc)
    target = 384 if C >= 512 else (768 if C >= 256 else 1024)
    per_thread = min(max(units * max(B, 1) // (PL * target), 4), 16)
    upb = per_thread * PL
    max_blocks = max(4096 // max(B, 1), 16)
    if cdiv(units, upb) > max_blocks:
        upb = cdiv(cdiv(units, max_blocks), PL) * PL
    return upb


def pool_stats_tiles(Ho, Wo, C, prec, B):
    """(blocks, TR, TC) of the fused pool + statistics pass on an Ho x Wo pooled map."""
    upb = stats_units_per_block(Ho * Wo, C, prec, B)
    cpc = 4 if STORAGE[prec] == torch.float32 else 8
    TC = 256 // (C // cpc)
    TR = min(max(upb // TC, 1), Ho)
    return cdiv(Wo, TC) * cdiv(Ho, TR), TR, TC


def ent_ppb(k, hw, prec, B):
    """Pixels per block of stage k's entropy pass (stage 0 runs on the padded 4-channel float image)."""
    return stats_units_per_block(hw, 4 if k == 0 else CHNS[k], "f32" if k == 0 else prec, B)


def plan(B, dims, prec):
    """[(statistics blocks, TR, TC, entropy blocks)] for k = 0..5: what nqa_adists_front_grid must report."""
    out = []
    for k, (h, w) in enumerate(dims):
        hw = h * w
        tr = tc = 0
        if k == 0:
            nblk = cdiv(hw, min(hw, 4096))
        elif k <= 4:
            nblk, tr, tc = pool_stats_tiles((h + 1) // 2, (w + 1) // 2, CHNS[k], prec, B)
        else:
            nblk = cdiv(hw, stats_units_per_block(hw, CHNS[k], prec, B))
        out.append((nblk, tr, tc, cdiv(hw, ent_ppb(k, hw, prec, B))))
    return out


# ---- the replay -------------------------------------------------------------------------------------------------------
# ONE_PIXEL: a 1 x 1 map has p = 1 in a live channel, and its entropy is -log2(1 + 1e-12): -1.4e-12 in exact arithmetic,
# 0 in float32, where 1 + 1e-12 is 1.  The stage's weights are those entropies over their sum: about 1 each from the
# float64 figures, 0 from the float32 ones, so the reference AS IT RUNS (float32) puts the whole stage on the clamp's lower
# bound and a float64 run does not.  The replay takes the float32 value, an exact 0, in both precisions: the operation
# under test is the reference's, and the kernels' p = 1 and log2f(1) = 0 give that 0 as well.  Everything downstream of
# it (the stage's weights, the common normalisation, the clamp) is then as well-conditioned as in any other case.
MUTANTS = {
    "row": "last input row dropped from an odd-height tap's sums (taps 1..4)",
    "col": "last input column dropped from an odd-width tap's sums (taps 1..4)",
    "twice": "the border pixel (0, 0) counted twice in the sums (taps 1..4)",
    "fold64": "entropy partial blocks from index 64 up skipped",
    "lastblk": "the last, partial entropy block skipped",
    "pad4": "stage 0 scaled by its padded channel count 4 instead of 3",
    "unbiased": "unbiased instead of population std in the clamp",
    "nm1": "variances and covariance divided by n - 1",
    "invsum": "inv taken from the sum instead of the sum of squares",
    "norenorm": "the clamp's second renormalisation left out",
}


def mutant_applies(m, case):
    pooled = case.dims[1:5]
    if m == "row":
        return any(h % 2 == 1 for h, _ in pooled)
    if m == "col":
        return any(w % 2 == 1 for _, w in pooled)
    if m == "fold64":
        return any(e > 64 for _, _, _, e in plan(case.B, case.dims, case.prec))
    if m == "lastblk":
        return any(h * w % ent_ppb(k, h * w, case.prec, case.B) for k, (h, w) in enumerate(case.dims))
    return True


def _stage(k, fx, fy, dtype, mutant, ppb):
    """Rows (inv_x, inv_y, hsum, mean_x, mean_y, var_x, var_y, cov), each (B, C), of one stage's raw maps (B,C,H,W)."""
    fx, fy = fx.to(dtype), fy.to(dtype)
    B, C, H, W = fx.shape
    n = H * W
    wmap = None  # how often the statistics sums count every pixel; None: once
    if 1 <= k <= 4 and ((mutant == "row" and H % 2) or (mutant == "col" and W % 2) or mutant == "twice"):
        wmap = torch.ones((H, W), dtype=dtype)
        if mutant == "row":
            wmap[-1, :] = 0
        elif mutant == "col":
            wmap[:, -1] = 0
        else:
            wmap[0, 0] = 2
    if wmap is None:
        mx, my = fx.mean((2, 3)), fy.mean((2, 3))
        dx, dy = fx - mx[:, :, None, None], fy - my[:, :, None, None]
        vx, vy = (dx * dx).mean((2, 3)), (dy * dy).mean((2, 3))
        cov = (fx * fy).mean((2, 3)) - mx * my
        sxx, syy, sx, sy = (fx * fx).sum((2, 3)), (fy * fy).sum((2, 3)), fx.sum((2, 3)), fy.sum((2, 3))
    else:  # the same moments from sums that count pixel p wmap[p] times and are still divided by n
        sx, sy = (wmap * fx).sum((2, 3)), (wmap * fy).sum((2, 3))
        sxx, syy, sxy = (wmap * fx * fx).sum((2, 3)), (wmap * fy * fy).sum((2, 3)), (wmap * fx * fy).sum((2, 3))
        mx, my = sx / n, sy / n
        vx, vy, cov = sxx / n - mx * mx, syy / n - my * my, sxy / n - mx * my
    if mutant == "nm1" and n > 1:
        vx, vy, cov = vx * n / (n - 1), vy * n / (n - 1), cov * n / (n - 1)
    if mutant == "invsum":
        sxx, syy = sx, sy
    ix, iy = 1 / sxx.sqrt().clamp_min(1e-12), 1 / syy.sqrt().clamp_min(1e-12)
    p = (torch.relu(fx) * ix[:, :, None, None]).reshape(B, C, n)
    den = p.sum(2, keepdim=True) if wmap is None else (wmap.reshape(1, 1, n) * p).sum(2, keepdim=True)
    p = p / (den + C0)
    terms = -p * torch.log2(p + C0)
    nblk = cdiv(n, ppb)
    if mutant == "fold64" and nblk > 64:
        terms = terms[:, :, :64 * ppb]
    if mutant == "lastblk" and n % ppb:
        terms = terms[:, :, :(nblk - 1) * ppb]
    hsum = terms.sum(2)
    if n == 1:  # see ONE_PIXEL
        hsum = torch.zeros_like(hsum)
    return ix, iy, hsum, mx, my, vx, vy, cov


def weights(hsum, mutant=None):
    """(wgt (B,1475), lo (B,)): the channel weights from the folded entropies, and what the clamp's lower bound becomes."""
    parts = []
    for k in range(6):
        h = hsum[:, COFF[k]:COFF[k] + CHNS[k]]
        parts.append(h / (h.sum(1, keepdim=True) + C0) * (4 if mutant == "pad4" and k == 0 else CHNS[k]))
    w = torch.cat(parts, 1)
    w = w / w.sum(1, keepdim=True)
    mu = w.mean(1, keepdim=True)
    sd = (((w - mu) ** 2).sum(1, keepdim=True) / (CTOT - 1 if mutant == "unbiased" else CTOT)).sqrt()
    lo, hi = mu - 0.5 * sd, mu + 0.5 * sd
    w = torch.minimum(torch.maximum(w, lo), hi)
    s1 = 1.0 if mutant == "norenorm" else w.sum(1, keepdim=True)
    return w / s1, (lo / s1)[:, 0]


def front(x, y, taps_x, taps_y, dtype, mutant=None, prec="f32"):
    """{"q": (8,B,1475) with row 2 = hsum, "wgt": (B,1475), "lo": (B,)} in `dtype`.  x, y (B,3,H,W); taps_x[k], taps_y[k]
    (B,C,H,W) holding the values the kernels read (16-bit taps as their rounded values).  `mutant`: one of MUTANTS;
    `prec` fixes the entropy passes' block size, which the block mutants refer to."""
    B = x.shape[0]
    rows = []
    for k, (fx, fy) in enumerate(zip([x] + list(taps_x), [y] + list(taps_y))):
        hw = fx.shape[2] * fx.shape[3]
        rows.append(_stage(k, fx, fy, dtype, mutant, ent_ppb(k, hw, prec, B)))
    q = torch.stack([torch.cat([r[j] for r in rows], 1) for j in range(8)])
    wgt, lo = weights(q[2], mutant)
    return {"q": q, "wgt": wgt, "lo": lo}


# ---- the check --------------------------------------------------------------------------------------------------------
ONE_E12 = float(torch.tensor(1e12, dtype=torch.float32))


def stage_slices():
    return [slice(COFF[k], COFF[k] + CHNS[k]) for k in range(6)]


def yardstick(r32, r64):
    """e32: rel_err per stage of hsum and of wgt, the float32 replay against the float64 one."""
    return {name: [rel_err(a[..., s], b[..., s]) for s in stage_slices()]
            for name, a, b in (("hsum", r32["q"][2], r64["q"][2]), ("wgt", r32["wgt"], r64["wgt"]))}


def dead_channels(x, y, taps_x, taps_y):
    """(dead_x, dead_y), each (B,1475) bool: channels whose raw map is zero throughout."""
    fx, fy = [x] + list(taps_x), [y] + list(taps_y)
    return (torch.cat([(f == 0).all(3).all(2) for f in fx], 1), torch.cat([(f == 0).all(3).all(2) for f in fy], 1))


def check(out, r64, e32, dead):
    """[(name, worst error / bound, worst error)] of every bound class, and whether all hold.  `out`: q (8,B,1475) and
    wgt (B,1475) of the code under test (any float type, any device); r64, e32: references(); dead: dead_channels()."""
    q, wgt = out["q"].detach().cpu(), out["wgt"].detach().cpu()
    qd, wd, rq, rw = q.double(), wgt.double(), r64["q"], r64["wgt"]
    figs = []

    def ratio(name, err, bound):
        bad = torch.isnan(err) | (err > bound)
        r = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
        r = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), r)
        figs.append((name, float(r.max()), float(torch.nan_to_num(err, nan=float("inf")).max())))
        return not bool(bad.any())

    ok = True
    for j in (3, 4):  # the means
        ok &= ratio("mean", (qd[j] - rq[j]).abs(), 1e-6 * (rq[j].abs() + 1e-3))
    scale = (rq[5] + rq[6]).clamp_min(1e-12)
    for j in (5, 6, 7):  # variances, covariance
        ok &= ratio("var", (qd[j] - rq[j]).abs(), 2e-5 * scale + 1e-12)
    for j in (0, 1):  # inv, elementwise
        ok &= ratio("inv", (qd[j] - rq[j]).abs(), 1e-6 * rq[j].abs())
    for name, a, r in (("hsum", qd[2], rq[2]), ("wgt", wd, rw)):
        for k, s in enumerate(stage_slices()):
            err, b = rel_err(a[..., s], r[..., s]), max(YARD * e32[name][k], FLOOR)
            figs.append((name, err / b, err))
            ok &= err <= b
    # a dead channel: inv exactly float32(1e12), mean, variance and covariance exactly 0; hsum exactly 0 (dead in x)
    dx, dy = dead
    exact = True
    for d, rows in ((dx, (0, 3, 5)), (dy, (1, 4, 6)), (dx | dy, (7,))):
        for j in rows:
            want = ONE_E12 if j < 2 else 0.0
            exact &= bool((q[j].float()[d] == want).all())
    exact &= bool((q[2][dx] == 0).all())
    figs.append(("dead exact", 0.0 if exact else float("inf"), 0.0))
    ok &= exact
    # a channel dead in x sits on the clamp's lower bound (0 if that bound is negative), to its stage's bound on wgt
    dw = 0.0
    for k, s in enumerate(stage_slices()):
        if bool(dx[:, s].any()):
            want = r64["lo"].clamp_min(0)[:, None].expand(-1, CHNS[k])
            err = float((wd[:, s] - want).abs()[dx[:, s]].max()) / float(rw[:, s].abs().max())
            dw = max(dw, err / max(YARD * e32["wgt"][k], FLOOR))
    figs.append(("dead wgt", dw, 0.0))
    ok &= dw <= 1
    # every image's weights sum to 1 within 1475 float32 roundings
    s = float((wd.sum(1) - 1).abs().max())
    figs.append(("sum wgt", s / (CTOT * 2.0 ** -24), s))
    ok &= s <= CTOT * 2.0 ** -24
    return figs, bool(ok)


def worst(figs):
    """{class: (largest error / bound, largest error)} of check()'s figures."""
    out = {}
    for name, r, e in figs:
        o = out.get(name, (0.0, 0.0))
        out[name] = (max(o[0], r), max(o[1], e))
    return out


def show(figs):
    return "  ".join("%s %.2e (%.2f)" % (n, e, r) for n, (r, e) in worst(figs).items())


# ---- cases ------------------------------------------------------------------------------------------------------------
# dims: (H, W) of the image and of taps 1..5.  family: A post-ReLU-like, B scale and cancellation edges, C exact zeros.
# expect: {k: (statistics blocks, TR, TC, entropy blocks)} the library's grid query must report (None: not asserted).
Case = namedtuple("Case", "name prec B dims family expect")
REST = (6, 10)  # taps not under test


def _c(name, prec="f32", B=1, family="A", expect=None, **taps):
    dims = [REST] * 6
    for key, hw in taps.items():
        dims[int(key[1:])] = hw
    return Case(name, prec, B, tuple(dims), family, expect or {})


def case_id(c):
    return "%s-%s-B%d-%s" % (c.name, c.prec, c.B, c.family)


MIXED = dict(k0=(7, 9), k1=(9, 33), k2=(13, 19), k3=(5, 7), k4=(9, 13), k5=(3, 3))


def _cases():
    out = []
    # pool_stats at C = 64 float (TC = 16, TR = 4): one tile; a ragged right tile of one pooled column; a ragged bottom tile
    # of one pooled row whose window's lower row is outside the image; both; fewer pooled rows than TR
    for (h, w), e in (((8, 32), (1, 4, 16, None)), ((8, 33), (2, 4, 16, None)), ((9, 32), (2, 4, 16, None)),
                      ((9, 33), (4, 4, 16, None)), ((3, 5), (1, 2, 16, None))):
        out.append(_c("pool64-%dx%d" % (h, w), k1=(h, w), expect={1: e}))
    # degenerate maps: every window is a border window
    for (h, w), e in (((1, 1), (1, 1, 16, 1)), ((1, 13), (1, 1, 16, 1)), ((13, 1), (2, 4, 16, 1)), ((2, 2), (1, 1, 16, 1))):
        out.append(_c("pool64-%dx%d" % (h, w), k1=(h, w), expect={1: e}))
    out.append(_c("pool-degenerate-all", k1=(1, 1), k2=(1, 13), k3=(13, 1), k4=(2, 2),
                  expect={1: (1, 1, 16, 1), 2: (1, 1, 8, None), 3: (2, 4, 4, None), 4: (1, 1, 2, 1)}))
    # C = 128, 256, 512 float (TC = 8, 4, 2) and 16-bit C = 64, 512 (TC = 32, 4): ragged odd x odd maps, several tiles each way
    out.append(_c("pool-wide-13x19", k1=(13, 19), k2=(13, 19), k3=(13, 19), k4=(13, 19),
                  expect={1: (2, 4, 16, None), 2: (4, 4, 8, None), 3: (6, 4, 4, None), 4: (10, 4, 2, None)}))
    for prec in ("f16", "bf16"):
        out.append(_c("pool-16bit", prec, k1=(13, 67), k4=(13, 19), expect={1: (4, 4, 32, None), 4: (6, 4, 4, None)}))
    # the workgroup-id remap over the XCDs: B = 3 with 12 blocks; B = 1 with exactly 8
    out.append(_c("pool-xcd12", B=3, k1=(9, 33), expect={1: (4, 4, 16, None)}))
    out.append(_c("pool-xcd8", k4=(9, 13), expect={4: (8, 4, 2, None)}))
    # stats_nhwc (tap 5) and the entropy at C = 512: 1 block; 2, the last of one pixel; 67, the last of one pixel
    for (h, w), n in (((2, 4), 1), ((3, 3), 2), ((23, 23), 67)):
        out.append(_c("tap5-%dx%d" % (h, w), k5=(h, w), expect={5: (n, 0, 0, n)}))
    # the entropy at C = 64: exactly one full block, and one pixel more
    out.append(_c("ent64-8x8", k1=(8, 8), expect={1: (None, None, None, 1)}))
    out.append(_c("ent64-5x13", k1=(5, 13), expect={1: (None, None, None, 2)}))
    # the images: one block; 4096 pixels exactly; 4160 (two statistics blocks, five entropy blocks, the last ragged)
    for (h, w), e in (((5, 7), (1, 0, 0, 1)), ((64, 64), (1, 0, 0, 4)), ((65, 64), (2, 0, 0, 5))):
        out.append(_c("image-%dx%d" % (h, w), k0=(h, w), expect={0: e}))
    # all four modes on one mixed case, B = 1 and B = 3
    for prec in ("f32", "f32s", "f16", "bf16"):
        for B in (1, 3):
            out.append(_c("mixed", prec, B, **MIXED))
    # families B and C on one shape per kernel, float and 16-bit taps
    for fam in ("B", "C"):
        for prec in ("f32", "f16"):
            out.append(_c("mixed", prec, 2, fam, **MIXED))
        out.append(_c("tap5-23x23", family=fam, k0=(65, 64), k5=(23, 23)))
    assert len({case_id(c) for c in out}) == len(out)
    return out


CASES = _cases()
DEAD_STAGE = 3  # family C: this whole stage is dead in x


def inputs(case):
    """(x, y, taps) of a case from a seed made of its id.  x, y: (B,3,H,W) float32 in [0,1]; taps[k]: (2B,H,W,C) NHWC in
    the mode's storage type, x images then y images."""
    gen = torch.Generator().manual_seed(zlib.crc32(case_id(case).encode()))
    B = case.B
    H, W = case.dims[0]
    x = torch.rand((B, 3, H, W), generator=gen)
    y = (x + 0.05 * torch.randn((B, 3, H, W), generator=gen)).clamp(0, 1)
    if case.family == "C":
        x[:, 1] = 0
        y[:, 2] = 0
        x[:, 0, 1:4, 2:6] = 0
    taps = []
    for k in range(1, 6):
        H, W = case.dims[k]
        C = CHNS[k]
        ramp = 0.5 * (torch.arange(H, dtype=torch.float32)[:, None] / H + torch.arange(W, dtype=torch.float32)[None, :] / W)
        scale = 0.5 + torch.rand((B, C, 1, 1), generator=gen)
        fx = scale * (torch.relu(4 * torch.rand((B, C, H, W), generator=gen) - 2) + ramp)
        fy = torch.relu(fx + 0.5 * scale * torch.randn((B, C, H, W), generator=gen))
        if case.family == "B":
            for f in (fx, fy):
                f[:, 5] = 2.0 + 1e-3 * torch.rand((B, H, W), generator=gen)    # nearly constant
                f[:, 6] = 1e-4 + 9e-4 * torch.rand((B, H, W), generator=gen)   # tiny
                f[:, 7] = 300 * torch.rand((B, H, W), generator=gen)           # large
        if case.family == "C":
            fx[:, 1] = 0  # dead in x only
            fx[:, 2] = 0  # dead in both
            fy[:, 2] = 0
            fx[:, 0, 1:4, 2:6] = 0  # a zero patch in a live channel
            fy[:, 0, 1:4, 2:6] = 0
            if k == DEAD_STAGE:
                fx[:] = 0
        taps.append(torch.cat([fx, fy]).permute(0, 2, 3, 1).contiguous().to(STORAGE[case.prec]))
    return x, y, taps


def nchw(taps, B):
    """(taps_x, taps_y) as (B,C,H,W) views of inputs()' taps."""
    return [t[:B].permute(0, 3, 1, 2) for t in taps], [t[B:].permute(0, 3, 1, 2) for t in taps]


def references(case):
    """(inputs, r64, e32, dead) of a case."""
    x, y, taps = inputs(case)
    tx, ty = nchw(taps, case.B)
    r64 = front(x, y, tx, ty, torch.float64, prec=case.prec)
    r32 = front(x, y, tx, ty, torch.float32, prec=case.prec)
    return (x, y, taps), r64, yardstick(r32, r64), dead_channels(x, y, tx, ty)
