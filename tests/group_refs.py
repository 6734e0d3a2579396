"""Float64 references and inputs for the group statistics kernels (nqa_group_stats.hip: group_stats_nhwc_kernel in float,
f16 and bf16, group_stats_nchw_kernel on float planes), built on tests/pool_refs.py; tests/test_group_refs.py checks them on
the CPU, tests/test_gpu_group_stats_exact.py holds the kernels to them.  Everything here is torch and runs on whichever
device its input lives on.

Maps are NHWC, (n, HW, C) with n = R + R * K: the R references, then render (r, k) at map R + r * K + k; pair p = r * K + k.

The EXACT inputs (group_exact_maps) are multiples of 1/4 in [0, 4], as pool_refs.exact_maps draws them.  On them nothing
the kernels compute for the five sums rounds:
  - a thread of group_stats_nhwc_kernel holds at most 16 samples of a channel (NQA_GROUP_ITEMS strip items) with
    |f - p| <= 4 around its pivot p, so every shifted float moment -- sum (f - p), sum (f - p)^2, sum (fx - px)(fy - py) --
    is a sum of at most 16 multiples of 1/16 of magnitude at most 16: below 2^12 in units of 1/16, far inside a float's
    24 bits, in whichever order and whether or not the compiler contracts a product and a sum into one fma;
  - the conversion to raw sums (ShiftedMoments::raw: products of two such numbers and a count up to 16), the block
    reduction over the pixel lanes and the fold of the per-block partials are sums of multiples of 1/16 below 2^53:
    exact in fp64;
  - the values themselves (0, 0.25 .. 4.0: at most 5 significant bits) are exact in f16 and bf16, so the 16-bit
    instances read the same numbers as the float one;
  - the plane kernel converts every sample to fp64 before it does anything and stays there.
So the five sums of every (pair, channel) have ONE right answer in bits, whatever the split of the map into blocks and
strips: a pixel lost, an item counted twice, a render booked to another row or read from another group, or a reference
strip that belongs to another block moves at least one of them (tests/test_group_refs.py shows each on the reference
alone).  What is left to round is the finalisation: S1 / S2 are formed in fp64 and stored as floats.

S CRITERION (s_close): |got - ref| <= 2^-23 |ref| + 2^-40 against pool_refs.s_from_sums of the exact sums in float64 --
one float rounding of an fp64 result (relative 2^-24) with a factor two for the fp64 operations that finalize_kernel
orders differently (a multiplication by 1 / HW where the reference divides), and nothing else.
"""
import torch

import pool_refs as P

DEAD_BOTH, DEAD_X = P.DEAD_BOTH, P.DEAD_X
DEAD_REN0 = 6  # live in the references, zero in render 0 of each group
S_REL, S_ABS = 2.0 ** -23, 2.0 ** -40


def special_channels(c):
    """(dead in every map, dead in the references only, dead in render 0 of a group only) and the groups they apply to
    (None = all).  Maps of fewer than 8 channels (the planes of tap 0, C = 3) take channels 0, 1, 2 in group 0 ONLY, so
    that every later group keeps all its channels live."""
    if c >= 8:
        return (DEAD_BOTH, DEAD_X, DEAD_REN0), None
    assert c >= 3
    return (0, 1, 2), 1


def group_exact_maps(R, K, hw, c, seed, device="cpu"):
    """float32 (R + R K, hw, c), the references first: multiples of 1/4 in [0, 4], about 40 % zeros as behind a ReLU, all
    maps independent, then
      - channel DEAD_BOTH zero everywhere, channel DEAD_X zero in the references only,
      - channel DEAD_REN0 zero in render 0 of each group only (a live reference against a dead render),
      - render K - 1 of each group identical to its reference, when K >= 2
    (for c < 8 see special_channels)."""
    g = torch.Generator(device=device).manual_seed(seed)
    n = R + R * K
    shape = (n, hw, c)
    v = torch.randint(1, 17, shape, generator=g, device=device).float() * 0.25
    v = torch.where(torch.rand(shape, generator=g, device=device) < 0.4, torch.zeros_like(v), v)
    (both, dead_x, ren0), groups = special_channels(c)
    for r in range(R if groups is None else groups):
        v[r, :, both] = 0
        v[R + r * K:R + (r + 1) * K, :, both] = 0
        v[r, :, dead_x] = 0
        v[R + r * K, :, ren0] = 0
    if K >= 2:
        for r in range(R):
            v[R + r * K + K - 1] = v[r]
    return v


def _sums(x, y):
    """float64 (R, K, C, 5) from x (R, n_px, C) and y (R, K, n_px, C), both float64."""
    r, k = y.shape[:2]
    sx = x.sum(1)[:, None].expand(r, k, -1)
    sxx = (x * x).sum(1)[:, None].expand(r, k, -1)
    sxy = torch.stack([(x * y[:, j]).sum(1) for j in range(k)], 1)  # (one render at a time: no (R, K, HW, C) product)
    return torch.stack([sx, y.sum(2), sxx, (y * y).sum(2), sxy], -1)


def group_sums_ref(feat, R, K):
    """float64 (R K, C, 5) = sum x, sum y, sum x^2, sum y^2, sum xy over the pixels of the STORED values of feat
    (R + R K, HW, C): x the reference of the pair's group (repeated per render), y the render."""
    t = feat.double()
    n, hw, c = t.shape
    assert n == R + R * K
    return _sums(t[:R], t[R:].view(R, K, hw, c)).reshape(R * K, c, 5)


def s_finalize(sums, hw):
    """float32 (S1, S2) from float64 sums (..., 5) in finalize_kernel's own order (plane_moments, nqa_common.h): inv =
    1.0 / HW, mx = s0 * inv, vx = s2 * inv - mx * mx, ... in fp64, the quotients rounded to float."""
    s = sums.double()
    inv = 1.0 / float(hw)
    mx, my = s[..., 0] * inv, s[..., 1] * inv
    vx, vy = s[..., 2] * inv - mx * mx, s[..., 3] * inv - my * my
    cov = s[..., 4] * inv - mx * my
    c1 = c2 = 1e-6
    return ((2.0 * mx * my + c1) / (mx * mx + my * my + c1)).float(), ((2.0 * cov + c2) / (vx + vy + c2)).float()


def s_bound(ref):
    return S_REL * ref.abs() + S_ABS


def s_excess(got, ref):
    """max over the entries of |got - ref| / (2^-23 |ref| + 2^-40), both taken to float64: the criterion holds at <= 1."""
    ref = ref.double()
    return ((got.double() - ref).abs() / s_bound(ref)).max().item()


# ---- what a kernel with a given defect would return, computed on the reference alone (tests/test_group_refs.py) ----
def drop_last_pixel(feat, R, K):
    """The last pixel of every map never read."""
    return group_sums_ref(feat[:, :-1], R, K)


def double_item(feat, R, K, pixel):
    """One strip item -- pixel `pixel` of the reference and of each of its renders -- counted twice."""
    return group_sums_ref(feat, R, K) + group_sums_ref(feat[:, pixel:pixel + 1], R, K)


def neighbour_group(feat, R, K):
    """Group r's renders read from group (r + 1) % R."""
    ren = feat[R:].view(R, K, *feat.shape[1:]).roll(-1, 0)
    return group_sums_ref(torch.cat([feat[:R], ren.flatten(0, 1)]), R, K)


def rows_exchanged(feat, R, K, k0, k1):
    """The sums of renders k0 and k1 of every group written to each other's rows."""
    s = group_sums_ref(feat, R, K).view(R, K, -1, 5).clone()
    s[:, [k0, k1]] = s[:, [k1, k0]]
    return s.view(R * K, -1, 5)


def stale_strip(feat, R, K, ppb):
    """Every block after the first walks its renders against the reference strip of the block before it (ppb pixels per
    block; the last block takes as many pixels of that strip as it has itself)."""
    hw = feat.shape[1]
    assert hw > ppb
    x = feat[:R].clone()
    x[:, ppb:] = feat[:R, :hw - ppb]
    return group_sums_ref(torch.cat([x, feat[R:]]), R, K)
