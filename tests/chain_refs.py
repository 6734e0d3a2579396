"""Plain-torch replay of the BACK part of the A-DISTS forward (nqa_adists_chain, include/nqa.h): the texture-probability
chain from the coarsest stage to the finest (compute_prob, ADISTS.py:71-100; nerf_qa_amd/ADISTS/head.py
texture_probabilities is the model of the arithmetic), the stages' D sums and D_b (:185-191) and the as_map=True
resampler (:163, 188-189, 193), from the six stages' gamma / tw / sw maps.  Also the case list and seeded inputs of
tests/test_gpu_adists_chain.py, the bound both test files share, and deliberately wrong replays.

float64 is the reference; float32 is the yardstick whose own distance from the reference sets the GPU test's bound."""
import math
import warnings
import zlib
from collections import namedtuple

import torch
import torch.nn.functional as F

WIN = 21
C0 = 1e-12               # ADISTS.py:76
FLOOR = 16 * 2.0 ** -24  # 16 float32 roundings (tests/window_refs.py)
YARD = 8                 # a HIP chain may sit this many times as far from float64 as the float32 replay does (ibid.)

MUTANTS = {
    "biased_std": "population instead of unbiased standard deviation of gamma",
    "no_minmax1": "the sigmoid map is not min-max normalised",
    "no_minmax2": "the product with the upsampled coarser stage is not min-max normalised",
    "chain_half_pixel": "align_corners=False in the chain's upsample",
    "chain_nearest": "nearest-neighbour upsample in the chain",
    "map_corners": "align_corners=True in the map resampler",
    "d_wrong_count": "a stage's D sum divided by the next coarser stage's element count",
    "map_neighbour_ps": "the map's stages 0 and 1 (equal dims) built from each other's ps_prod",
}
# the output a mutant must show in: "ps" (any of the six ps_prod maps), "d" or "map"
MUTANT_OUTPUT = {"biased_std": "ps", "no_minmax1": "ps", "no_minmax2": "ps", "chain_half_pixel": "ps",
                 "chain_nearest": "ps", "map_corners": "map", "d_wrong_count": "d", "map_neighbour_ps": "map"}


def chain_dims(H, W):
    """([(mh, mw)] * 6, [windowed] * 6) of an H x W frame: the tap is H x W for stages 0 and 1 and halves, rounding up,
    from stage 2 on; a tap of at least 21 x 21 gives a map of valid windows, a smaller one the global branch's 1 x 1."""
    hs, ws = [H, H], [W, W]
    for _ in range(4):
        hs.append((hs[-1] + 1) // 2)
        ws.append((ws[-1] + 1) // 2)
    win = [h >= WIN and w >= WIN for h, w in zip(hs, ws)]
    return [(h - WIN + 1, w - WIN + 1) if ok else (1, 1) for h, w, ok in zip(hs, ws, win)], win


def _minmax(p):
    lo = p.flatten(2).amin(dim=-1, keepdim=True).unsqueeze(-1)
    hi = p.flatten(2).amax(dim=-1, keepdim=True).unsqueeze(-1)
    return (p - lo) / (hi - lo + C0)


def replay(gamma, tw, sw, H, W, dtype, mutant=None, probe=None):
    """(ps_prod: six (B, mh, mw) maps, D (B,), map (B, H, W)) in `dtype` from the six stages' (B, mh, mw) maps.
    `mutant`: one of MUTANTS, a one-line departure.  `probe`: a dict that receives, per windowed stage k, the ranges per
    image of the raw sigmoid map and of ps * upsampled coarser stage (the two quantities the min-max steps divide by)."""
    dims, windowed = chain_dims(H, W)
    gamma, tw, sw = ([t.to(dtype).unsqueeze(1) for t in ts] for ts in (gamma, tw, sw))
    prod = torch.ones_like(gamma[0][:, :, :1, :1])
    ps_prod = [None] * 6
    for k in range(5, -1, -1):
        g = gamma[k]
        assert tuple(g.shape[2:]) == dims[k], (k, tuple(g.shape), dims[k])
        if windowed[k]:
            with warnings.catch_warnings():  # one element: torch.std warns and gives NaN, which is the expected result
                warnings.simplefilter("ignore")
                sd = g.std(dim=(2, 3), keepdim=True, unbiased=mutant != "biased_std")
            raw = 1 / (1 + torch.exp(-(g - g.mean(dim=(2, 3), keepdim=True)) / (sd + C0)))
            ps = raw if mutant == "no_minmax1" else _minmax(raw)
            if mutant == "chain_nearest":
                up = F.interpolate(prod, size=dims[k], mode="nearest")
            else:
                up = F.interpolate(prod, size=dims[k], mode="bilinear", align_corners=mutant != "chain_half_pixel")
            pp = ps * up
            if probe is not None:
                rng = lambda t: t.flatten(1).amax(1) - t.flatten(1).amin(1)
                probe[k] = (rng(raw), rng(pp))
            prod = pp if mutant == "no_minmax2" else _minmax(pp)
        else:
            prod = 1 / (1 + torch.exp(-g)) * F.interpolate(prod, size=(1, 1), mode="bilinear", align_corners=True)
        ps_prod[k] = prod
    d = 0
    full = torch.zeros((gamma[0].shape[0], 1, H, W), dtype=dtype)
    for k in range(5, -1, -1):
        ps = ps_prod[k ^ 1] if (mutant == "map_neighbour_ps" and k < 2) else ps_prod[k]
        d_map = (1 - ps_prod[k]) * tw[k] + ps_prod[k] * sw[k]
        full = full + F.interpolate((1 - ps) * tw[k] + ps * sw[k], size=(H, W), mode="bilinear",
                                    align_corners=mutant == "map_corners")
        if mutant == "d_wrong_count":
            n = dims[min(k + 1, 5)]
            d = d + d_map.sum(dim=(2, 3)).sum(1) / (n[0] * n[1])
        else:
            d = d + d_map.mean(dim=(2, 3)).sum(1)
    return [p[:, 0] for p in ps_prod], d, (1 - full)[:, 0]


# ---- the check ----------------------------------------------------------------------------------------------------
def flat(outs):
    """(names, tensors) of a replay's or a call's outputs: ps_prod0..5, d, map."""
    ps, d, m = outs
    return ["ps_prod%d" % k for k in range(6)] + ["d", "map"], list(ps) + [d, m]


def abs_err(a, r64):
    """max|a - r64| over the elements where r64 is finite; infinite if the shapes differ or `a` is NaN anywhere r64 is not
    (an element nobody wrote) or is not NaN somewhere r64 is (NaN parity)."""
    a = a.detach().cpu().double()
    if a.shape != r64.shape or not torch.equal(torch.isnan(a), torch.isnan(r64)):
        return float("inf")
    ok = ~torch.isnan(r64)
    return float((a[ok] - r64[ok]).abs().max()) if bool(ok.any()) else 0.0


def bound(e32, r64):
    """The GPU test's bound on abs_err for an output whose float32 replay sits at e32 from r64."""
    ok = ~torch.isnan(r64)
    top = float(r64[ok].abs().max()) if bool(ok.any()) else 0.0
    return max(YARD * e32, FLOOR * max(1.0, top))


def check(outs, r64, e32):
    """[(name, error, bound)] of the eight outputs and whether all pass."""
    names, got = flat(outs)
    figs = [(n, abs_err(g, r), bound(e, r)) for n, g, r, e in zip(names, got, flat(r64)[1], e32)]
    return figs, all(err <= b for _, err, b in figs)


# ---- cases --------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "H W B family")
# each (H, W, B) is the smallest that reaches its edge
SHAPES = (
    (20, 20, 2),    # all six stages global
    (21, 21, 1),    # stages 0, 1: one-element windowed maps -- NaN parity with torch.std
    (21, 22, 2),    # 1 x 2 maps
    (24, 21, 2),    # 4 x 1 maps
    (22, 23, 3),    # 2 x 3 maps: unbiased variance of 6 elements
    (36, 36, 2),    # n = 256: exactly one full block
    (36, 37, 2),    # n = 272: a last block of 16 live threads
    (41, 43, 2),    # stage 2 windowed 1 x 2 (a 21 x 22 tap), upsampled to 21 x 23
    (45, 88, 2),    # 25 x 68 over 3 x 24: two blocks over a partial one, nothing square
    (97, 131, 3),   # four windowed stages over two global ones
    (181, 170, 2),  # five windowed stages
    (350, 340, 2),  # all six windowed, hundreds of blocks
    (533, 534, 1),  # 513 x 514 > 262 144 elements: the stride loop under the 1024-block cap
)
FAMILIES = ("lognormal", "smooth", "twolevel")
CASES = [Case(h, w, b, f) for h, w, b in SHAPES for f in FAMILIES]


def case_id(c):
    return f"{c.H}x{c.W}-B{c.B}-{c.family}"


def inputs(case):
    """(gamma, tw, sw): three lists of six (B, mh, mw) float32 maps from a fixed seed.  gamma: lognormal
    (0.05 exp(sigma N(0,1))), smooth (0.05 exp of a few low-frequency waves that span the map whatever its size) or
    two-level (0.03 / 0.12 patches, both levels present, 2 % jitter); tw in [0.6, 0.9], sw in [0.1, 0.6].  The images of a
    batch differ in scale (x 1, 4, 0.25) and, for the lognormal family, in sigma (1, 0.5, 1.5).  Maps of 2 to 8 elements
    are sorted: two 1 x 2 stages that disagree on which element is the textured one multiply to a map of exact zeros, whose
    min-max step is 0 / 1e-12 -- a knife edge of the reference itself, which test_chain_refs.py keeps out of the cases."""
    gen = torch.Generator().manual_seed(zlib.crc32(case_id(case).encode()))
    dims, _ = chain_dims(case.H, case.W)
    rand = lambda *s: torch.rand(s, generator=gen, dtype=torch.float64)
    randn = lambda *s: torch.randn(s, generator=gen, dtype=torch.float64)
    gamma, tw, sw = [], [], []
    for mh, mw in dims:
        gs = []
        for b in range(case.B):
            scale = (1.0, 4.0, 0.25)[b % 3]
            if case.family == "lognormal":
                g = torch.exp((1.0, 0.5, 1.5)[b % 3] * randn(mh, mw))
            elif case.family == "smooth":
                yy = torch.linspace(0, 1, mh, dtype=torch.float64)[:, None] if mh > 1 else torch.zeros(1, 1, dtype=torch.float64)
                xx = torch.linspace(0, 1, mw, dtype=torch.float64)[None, :] if mw > 1 else torch.zeros(1, 1, dtype=torch.float64)
                f = torch.zeros(mh, mw, dtype=torch.float64)
                for _ in range(4):
                    fy, fx, ph = 3 * rand(1), 3 * rand(1), 2 * math.pi * rand(1)
                    f = f + 0.6 * torch.sin(2 * math.pi * (fy * yy + fx * xx) + ph)
                g = torch.exp(f + 0.8 * (yy - xx))
            else:
                cell = 4
                coarse = (rand((mh + cell - 1) // cell, (mw + cell - 1) // cell) < 0.4).double()
                lv = coarse.repeat_interleave(cell, 0).repeat_interleave(cell, 1)[:mh, :mw].clone()
                lv.view(-1)[0], lv.view(-1)[-1] = 0.0, 1.0  # both levels are there (a one-element map keeps the high one)
                g = (0.6 + 1.8 * lv) * (1 + 0.02 * randn(mh, mw))
            if 1 < mh * mw <= 8:  # (see the docstring: tiny maps agree across stages on where the texture is)
                g = g.flatten().sort().values.view(mh, mw)
            gs.append(0.05 * scale * g)
        gamma.append(torch.stack(gs).float())
        tw.append((0.6 + 0.3 * rand(case.B, mh, mw)).float())
        sw.append((0.1 + 0.5 * rand(case.B, mh, mw)).float())
    return gamma, tw, sw


def references(case):
    """(inputs, r64 outputs, e32 per output (ps_prod0..5, d, map), probe of the float64 replay) of a case."""
    gamma, tw, sw = inputs(case)
    probe = {}
    r64 = replay(gamma, tw, sw, case.H, case.W, torch.float64, probe=probe)
    r32 = replay(gamma, tw, sw, case.H, case.W, torch.float32)
    e32 = tuple(abs_err(a, r) for a, r in zip(flat(r32)[1], flat(r64)[1]))
    return (gamma, tw, sw), r64, e32, probe
