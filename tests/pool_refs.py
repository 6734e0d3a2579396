"""Float64 references and inputs for the pair path's pool + statistics pass (pool_stats_kernel) and its last-tap
statistics pass (stats_nhwc_kernel); tests/test_pool_refs.py checks them on the CPU, tests/test_gpu_pool_stats.py holds the
kernels to them.  Everything here is torch and runs on whichever device its input lives on.

Maps are NHWC, (2B, H, W, C) or (2B, HW, C): the B x maps, then the B y maps.

The EXACT inputs (exact_maps) are multiples of 1/4 in [0, 4].  On them nothing the kernels compute for the sums rounds:
  - a thread's shifted float moments are sums of multiples of 1/16 (|f - p| <= 4, squares <= 16) over at most 64 samples
    of a pool_stats thread (16 pooled pixels of 4) or 16 of a stats_nhwc thread: below 2^14 in units of 1/16, far inside a
    float's 24 bits;
  - the raw fp64 sums, the block's partials and their fold are sums of multiples of 1/16 below 2^53.
So the five sums have ONE right answer in bits, and a pixel lost, counted twice or booked to the wrong pair or channel
moves at least one of them (test_pool_refs.py shows that on the reference alone).  The pooled window sum is exact too: the
weights are 1/16, 1/8, 1/4, so it is a multiple of 1/256 of at most 16 = 12 bits, and adding 1e-12f to a non-zero one (at
least 2^-8, half an ulp 2^-32) changes nothing.  What is left to round is sqrtf and the store.
"""
import math

import torch

HANN = (0.25, 0.5, 0.25)  # hanning(5)[1:-1] normalised, per axis (DISTS_pt.py:17-19): the 3 x 3 filter is its outer product
DEAD_BOTH, DEAD_X = 3, 5  # channels of exact_maps: dead in both images / in the x image only
FLAT = 5                  # channel of realistic_maps that is nearly constant: 2.0 + 1e-3 * rand
FLOOR = 2.0 ** -22        # floor of the S1 / S2 bound (tests/test_gpu_group_stats.py)
NEAR_TIE = 2.0 ** -22     # a 16-bit result this close (relative) to a rounding tie may take either neighbour
# (significand bits, frexp exponent below which the format is subnormal)
FORMATS = {"f16": (11, -13), "bf16": (8, -125)}


def exact_maps(n2, dims, c, seed, device="cpu"):
    """float32 (n2, *dims, c): multiples of 1/4 in [0, 4], about 40 % zeros as behind a ReLU, the two halves independent;
    channel DEAD_BOTH zero everywhere, channel DEAD_X zero in the first half (the x maps)."""
    g = torch.Generator(device=device).manual_seed(seed)
    shape = (n2,) + tuple(dims) + (c,)
    v = torch.randint(1, 17, shape, generator=g, device=device).float() * 0.25
    v = torch.where(torch.rand(shape, generator=g, device=device) < 0.4, torch.zeros_like(v), v)
    v[..., DEAD_BOTH] = 0
    v[: n2 // 2, ..., DEAD_X] = 0
    return v


def realistic_maps(n2, dims, c, seed, device="cpu"):
    """float32 (n2, *dims, c), the generator of tests/test_gpu_group_stats.py for pairs: non-negative maps with a
    channel-dependent mean and spread, every seventh channel exactly dead, every eleventh (from 3) dead in map 0 only; pair
    b's y map is its x map plus noise behind the x map's mask (b % 3 == 0), the x map blurred along the rows (1), or
    independent (2).  Channel FLAT is 2.0 + 1e-3 * rand in both (tests/test_gpu_conv_pool.py): a spread far under the mean."""
    g = torch.Generator(device=device).manual_seed(seed)
    b = n2 // 2
    shape = (b,) + tuple(dims) + (c,)
    scale = 0.05 + 2.0 * torch.rand(c, generator=g, device=device)
    shift = torch.rand(c, generator=g, device=device) - 0.3

    def maps():
        v = ((torch.randn(shape, generator=g, device=device) + shift) * scale).clamp_(min=0)
        v[..., ::7] = 0
        return v
    x, other = maps(), maps()
    x[0, ..., 3::11] = 0
    y = torch.empty_like(x)
    for i in range(b):
        kind = i % 3
        if kind == 0:
            y[i] = (x[i] + 0.1 * other[i]).clamp_(min=0) * (x[i] > 0)
        elif kind == 1:
            y[i] = 0.5 * (x[i] + x[i].roll(1, 0))
        else:
            y[i] = other[i]
    v = torch.cat([x, y])
    v[..., FLAT] = 2.0 + 1e-3 * torch.rand(v.shape[:-1], generator=g, device=device)
    return v


def sums_ref(feat, b):
    """float64 (b, C, 5) = sum x, sum y, sum x^2, sum y^2, sum xy over the pixels of the STORED values of feat (2b, ..., C)."""
    t = feat.double().reshape(2 * b, -1, feat.shape[-1])
    x, y = t[:b], t[b:]
    return torch.stack([x.sum(1), y.sum(1), (x * x).sum(1), (y * y).sum(1), (x * y).sum(1)], -1)


def pool_ref(feat):
    """float64 L2pooling.forward (DISTS_pt.py:22-25) of NHWC feat (n, H, W, C): sqrt(3 x 3 Hanning, stride 2, zero padding 1,
    of the squares, + 1e-12) -> (n, (H+1)//2, (W+1)//2, C).  Written as nine shifted slices, no convolution call."""
    n, h, w, c = feat.shape
    ho, wo = (h + 1) // 2, (w + 1) // 2
    sq = torch.zeros((n, 2 * ho + 1, 2 * wo + 1, c), dtype=torch.float64, device=feat.device)
    sq[:, 1:h + 1, 1:w + 1] = feat.double() ** 2
    acc = torch.zeros((n, ho, wo, c), dtype=torch.float64, device=feat.device)
    for dy in range(3):
        for dx in range(3):
            acc += (HANN[dy] * HANN[dx]) * sq[:, dy:dy + 2 * ho:2, dx:dx + 2 * wo:2]
    return (acc + 1e-12).sqrt()


def s_from_sums(sums, npx):
    """float64 (S1, S2), each (b, C), from five raw sums over npx pixels: DISTS_pt.py:131-141 with the population variance
    and covariance written through the raw moments, as the forwards' finalisation does in fp64."""
    s = sums.double()
    mx, my = s[..., 0] / npx, s[..., 1] / npx
    vx, vy = s[..., 2] / npx - mx * mx, s[..., 3] / npx - my * my
    cov = s[..., 4] / npx - mx * my
    return (2 * mx * my + 1e-6) / (mx * mx + my * my + 1e-6), (2 * cov + 1e-6) / (vx + vy + 1e-6)


def s_ref(feat, b, np_dtype):
    """(S1, S2), each numpy (b, C): DISTS_pt.py:131-141 on the stored values of feat (2b, ..., C) in numpy arithmetic of
    np_dtype -- two-pass variance, one-pass covariance (the yardstick of tests/test_gpu_group_stats.py)."""
    v = feat.float().cpu().numpy().reshape(2 * b, -1, feat.shape[-1])
    x, y = v[:b].astype(np_dtype), v[b:].astype(np_dtype)
    c1 = c2 = np_dtype(1e-6)
    two = np_dtype(2)
    xm, ym = x.mean(1, keepdims=True, dtype=np_dtype), y.mean(1, keepdims=True, dtype=np_dtype)
    s1 = (two * xm * ym + c1) / (xm ** 2 + ym ** 2 + c1)
    xv = ((x - xm) ** 2).mean(1, keepdims=True, dtype=np_dtype)
    yv = ((y - ym) ** 2).mean(1, keepdims=True, dtype=np_dtype)
    cov = (x * y).mean(1, keepdims=True, dtype=np_dtype) - xm * ym
    s2 = (two * cov + c2) / (xv + yv + c2)
    assert s1.dtype == np_dtype and s2.dtype == np_dtype
    return s1[:, 0], s2[:, 0]


def _pow2(e):
    """2.0 ** e as float64 for an integer tensor e in the normal range, built from the bits (no pow, no rounding)."""
    return ((e.to(torch.int64) + 1023) << 52).view(torch.float64)


def float_ulp(ref):
    """The spacing of float32 in the binade of each (positive, normal) float64 value."""
    _, e = torch.frexp(ref)
    return _pow2(e - 24)


def round_to(ref, fmt):
    """Positive float64 values against the 16-bit format fmt ("f16" / "bf16"): (nearest with ties to even, the neighbour
    below, the neighbour above, near_tie) -- the three as float64, near_tie where the value lies within NEAR_TIE * value of
    the midpoint of its two neighbours.  Subnormal halves included (sqrt(1e-12) is one)."""
    p, emin = FORMATS[fmt]
    _, e = torch.frexp(ref)
    step = _pow2(torch.clamp(e, min=emin) - p)
    q = ref / step  # exact: a power of two
    lo = torch.floor(q)
    near = ((q - lo) - 0.5).abs() * step <= NEAR_TIE * ref
    return torch.round(q) * step, lo * step, (lo + 1) * step, near


def stored_check(got, ref, fmt):
    """16-bit pooled output `got` against the float64 pooled map: (ok, near_tie) elementwise.  ok: the value is the float64
    one rounded to storage, or one of its two neighbours where it lies within NEAR_TIE of their midpoint (there a sqrtf good
    to one float ulp, 2^-23 of the value, may land on either side)."""
    nearest, lo, hi, near = round_to(ref, fmt)
    g = got.double()
    return (g == nearest) | (near & ((g == lo) | (g == hi))), near


def window_sum_near_ties(fmt):
    """The k in 1..4096 whose sqrt(k / 256) -- every value a non-zero window of the exact inputs can pool to -- is a near tie
    of fmt."""
    k = torch.arange(1, 4097, dtype=torch.float64)
    return k[round_to((k / 256).sqrt(), fmt)[3]].to(torch.int64).tolist()


def drop_last_row(feat):
    """feat (n, H, W, C) as a kernel that skipped the last input row would see it."""
    return feat[:, :-1]


def double_count_block(feat, b, y0, x0):
    """The sums of feat with the 2 x 2 input block at (y0, x0) of every map counted twice."""
    blk = feat[:, y0:y0 + 2, x0:x0 + 2]
    return sums_ref(feat, b) + sums_ref(blk, b)


def pl_of(c, prec):
    """Pixels a block takes side by side (= the pool pass' tile width TC): 256 threads over C / (channels per 16 bytes)."""
    return 256 // (c // (4 if prec in ("f32", "f32s") else 8))


assert math.isclose(sum(HANN), 1.0)
