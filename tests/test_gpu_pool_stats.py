"""The pair path's pool + statistics pass (pool_stats_kernel: PrecF32, PrecF32S, PrecF16, PrecBF16 and the mixed modes'
PrecF16X) and its last-tap statistics pass (stats_nhwc_kernel: PrecF32, PrecF16, PrecBF16) on their own, through
ops.pool_stats / ops.stats_nhwc (include/nqa.h: nqa_pool_stats, nqa_pool_stats_f16_to_split16, nqa_stats_nhwc), against the
float64 references of tests/pool_refs.py.  Every launch writes into 0xFF-filled pooled / sums tensors, and those are
searched for NaN first: a tile the XCD permutation of the block ids never reaches leaves its NaNs behind.

(a) EXACT SUMS.  On pool_refs.exact_maps (multiples of 1/4 in [0, 4], 40 % zeros, one channel dead in both images and one
    in x only) every shifted float moment, every fp64 partial and the fold are exact (the argument is in pool_refs.py), so
    the five sums must be BIT-EQUAL to the float64 sums: torch.equal, no tolerance.  Sanity of that check, shown on the
    reference alone in tests/test_pool_refs.py::test_a_dropped_row_or_a_doubled_block_is_not_bit_equal: a reference with
    its last border row dropped moves sum x and sum y of every live channel, one 2 x 2 block counted twice moves over 90 %
    of the live channels (a block that is all zero in a channel cannot move it), and two pairs' x maps swapped move sum xy
    of every live channel -- none of them is bit-equal, so a kernel doing any of it fails here.
(b) POOLED MAP on the same inputs.  The window sum is exact in float and 1e-12f is absorbed by a non-zero one, so sqrtf
    (taken at 1 ulp, HIP's documented bound where it is not built correctly rounded) and the store are the only
    roundings.  Float output: within one float ulp (of the value's own binade) of the float64 value -- all-zero windows
    included, where sqrt(float(1e-12)) itself sits 0.02 ulp from 1e-6.  f16 / bf16 output: the float64 value rounded to
    storage, or either neighbour where that value lies within 2^-22 (relative) of their midpoint; such near ties must be at
    most 1 % of a case (test_pool_refs.py: 3 of the 4096 possible window sums in f16, none in bf16, under 0.1 % of any case).
    split16 output (f32s; f16 -> split16), decoded with ops.split16_decode: within 2^-21 |ref| + 2^-24 (test_split16_roundtrip's
    figure, plus one subnormal half step for the 1e-6 of an all-zero window).  The f32s bits must be ops.split16_encode of
    the f32 instance's map.
(c) REALISTIC VALUES (pool_refs.realistic_maps: the generator of test_gpu_group_stats.py plus a nearly constant channel
    2.0 + 1e-3 * rand): S1 / S2 in float64 from the returned sums against float64 S1 / S2 of the stored values; bound =
    the error of the same formula in float32 numpy, floored at 2^-22 -- test_gpu_group_stats.py's yardstick, taken over
    the ordinary channels and over the nearly constant one SEPARATELY (float32's one-pass covariance loses that channel
    altogether, and one bound over all channels would let every other channel be as wrong).  The nearly constant channel
    is held to 2^-16 besides: a thread's shifted float sums run over at most 64 samples, so they carry at most 64 * 2^-24
    of the VARIANCE, and S2, a quotient of such sums that is at most 1, moves by a few times that.  All figures are
    printed.  Measured on an MI355X: ordinary channels |dS1| <= 2.8e-8, |dS2| <= 2.0e-7 against bounds of 3.3e-6 .. 5.0e-5
    (pool_stats) and |dS2| <= 9.6e-8 against 2.4e-7 .. 2.1e-4 (stats_nhwc), at most 0.09 of the bound; the nearly constant
    channel |dS2| <= 3.6e-8 where the float32 replay errs by up to 9.2e+2.
(d) stats_nhwc: (a) and (c) at test_gpu_group_stats.py's (B, HW, C); the regimes are asserted from the grid query.
(e) EXACT PROPERTIES of both operators on realistic values: y == x gives equal x / y columns and equal sum x^2, sum y^2,
    sum xy (and identical pooled halves); swapping x and y swaps the columns bit for bit; two launches are bit-equal; a
    pair's row does not depend on its batch neighbours while the grid query reports the same tile shape.

Shapes of pool_stats, each regime asserted from nqa_pool_stats_grid (printed as TR / TC / tiles / grid):
  - all-border maps (1,1,1) (2,2,2) (1,1,9) (1,9,1) (1,3,3) (1,5,7) (8,4,6), at C = 64 (Wo < TC: a one-block grid, grids
    under 8, a grid that is a multiple of 8) and at C = 512 (TC = 2 or 4: several tile columns);
  - every storage type and C at (3, 37, 4 TC + 3): three tile columns, the last two pixels wide; five tile rows, the last
    ragged; H and W odd; grid 45, no multiple of 8 -- and at its even counterpart (2, 36, 4 TC);
  - TR >= 5 at C = 512: float (2, 96, 80), 16-bit (2, 128, 120); TR = 16: f32 (2, 163, 153), f16 (2, 222, 221) (201 / 197 MB
    of tap; the float64 reference is taken with torch on the device).
NOT covered: the planner's cap on the blocks of a batch (more than max(4096 / B, 16) tiles per pair, e.g. B >= 128 on maps
of over 500 MB), which only lengthens the tiles.
"""
import numpy as np
import pytest
import torch

import pool_refs as P

pytestmark = pytest.mark.gpu

# storage: (prec of the call, dtype of the tap, to_split16, 16-bit format of the pooled map or None)
STORAGE = {"f32": ("f32", torch.float32, False, None), "f32s": ("f32s", torch.float32, False, "split16"),
           "f16": ("f16", torch.float16, False, "f16"), "bf16": ("bf16", torch.bfloat16, False, "bf16"),
           "f16x": ("f16", torch.float16, True, "split16")}
CHANNELS = (64, 128, 256, 512)
BORDER = [(1, 1, 1), (2, 2, 2), (1, 1, 9), (1, 9, 1), (1, 3, 3), (1, 5, 7), (8, 4, 6)]


def _ragged(storage, c, even):
    tc = P.pl_of(c, STORAGE[storage][0])
    return (2, 36, 4 * tc) if even else (3, 37, 4 * tc + 3)


CASES = [(s, c, shape) for s in STORAGE for c in (64, 512) for shape in BORDER]
CASES += [(s, c, _ragged(s, c, even)) for s in STORAGE for c in CHANNELS for even in (False, True)]
TALL = [("f32", 512, (2, 96, 80)), ("f32s", 512, (2, 96, 80)), ("f16", 512, (2, 128, 120)), ("bf16", 512, (2, 128, 120)),
        ("f16x", 512, (2, 128, 120))]
TR16 = [("f32", 512, (2, 163, 153)), ("f16", 512, (2, 222, 221))]
CASES += TALL + TR16
# (the float32 replay is numpy on the host: the tall case is run for the float instance only, to stay inside a few seconds)
REALISTIC = [(s, c, _ragged(s, c, False)) for s in STORAGE for c in CHANNELS] + [("f32", 512, (2, 96, 80))]
NHWC_SHAPES = [(1, 1, 64), (2, 35, 64), (1, 299, 128), (3, 1551, 256), (2, 77, 512), (1, 6007, 512), (1, 24589, 512)]
NHWC_STORAGE = ("f32", "f16", "bf16")


def _id(case):
    return "%s_c%d_%dx%dx%d" % (case[0], case[1], *case[2])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _ff(shape, dtype, dev):
    """A tensor whose every byte is 0xFF: NaN as half, bfloat16, float, float64 and as the halves of a split16 record."""
    t = torch.empty(shape, dtype=dtype, device=dev)
    t.view(torch.uint8).fill_(0xFF)
    return t


def _has_nan(t, split16=False):
    return bool(torch.isnan(t.view(torch.float16) if split16 else t).any())


def _pool_stats(feat, b, storage, dev):
    """ops.pool_stats into 0xFF-filled outputs, searched for NaN, shapes and dtypes asserted."""
    from nerf_qa_amd import ops
    prec, dtype, to_split, fmt = STORAGE[storage]
    n, h, w, c = feat.shape
    assert feat.dtype == dtype and n == 2 * b
    pooled = _ff((n, (h + 1) // 2, (w + 1) // 2, c), torch.float32 if fmt == "split16" else dtype, dev)
    sums = _ff((b, c, 5), torch.float64, dev)
    assert _has_nan(pooled, fmt == "split16") and _has_nan(sums)
    p, s = ops.pool_stats(feat, b, prec, pooled=pooled, sums=sums, to_split16=to_split)
    assert p.data_ptr() == pooled.data_ptr() and s.data_ptr() == sums.data_ptr()
    assert not _has_nan(sums), "a partial sum was never written"
    assert not _has_nan(pooled, fmt == "split16"), "a pooled pixel was never written"
    assert p.shape == (n, (h + 1) // 2, (w + 1) // 2, c) and s.shape == (b, c, 5) and s.dtype == torch.float64
    return p, s


def _stats_nhwc(feat, b, prec, dev):
    from nerf_qa_amd import ops
    sums = _ff((b, feat.shape[-1], 5), torch.float64, dev)
    s = ops.stats_nhwc(feat, b, prec, sums=sums)
    assert s.data_ptr() == sums.data_ptr() and not _has_nan(s), "a partial sum was never written"
    return s


def _grid(storage, c, shape):
    from nerf_qa_amd import ops
    return ops.pool_stats_grid(shape[0], shape[1], shape[2], c, STORAGE[storage][0])


def test_the_shapes_reach_the_regimes_they_are_chosen_for():
    """From nqa_pool_stats_grid, for the cases of this file (no launch)."""
    grids = {_id(k): _grid(*k) for k in CASES}
    print("\nTR / TC / tiles across / tiles per pair / grid of every pool_stats case:")
    for k, g in grids.items():
        print(f"  {k}: {g}")
    for s in STORAGE:
        small = [_grid(s, 64, shape) for shape in BORDER]
        tc = P.pl_of(64, STORAGE[s][0])
        assert all(g[1] == tc and g[2] == 1 and (shape[2] + 1) // 2 < tc for g, shape in zip(small, BORDER))  # Wo < TC
        sizes = [g[4] for g in small]
        assert 1 in sizes and any(1 < n < 8 for n in sizes) and any(n % 8 == 0 for n in sizes), sizes
        assert any(g[2] > 1 for g in (_grid(s, 512, shape) for shape in BORDER))
        for c in CHANNELS:
            tr, tc, tiles_x, nblk, grid = _grid(s, c, _ragged(s, c, False))
            assert (tr, tc, tiles_x, nblk, grid) == (4, P.pl_of(c, STORAGE[s][0]), 3, 15, 45) and grid % 8
            wo = (4 * tc + 3 + 1) // 2
            assert wo - 2 * tc == 2 and 19 - 4 * tr == 3  # the last tile column is two pooled pixels wide, the last row three high
            tr, tc, tiles_x, nblk, grid = _grid(s, c, _ragged(s, c, True))
            assert (tr, tiles_x, nblk, grid) == (4, 2, 10, 20)
    for k in TALL:
        assert 5 <= _grid(*k)[0] < 16, (k, _grid(*k))
    for k in TR16:
        assert _grid(*k)[0] == 16, (k, _grid(*k))
        assert 4 * k[2][1] * k[2][2] * k[1] * (4 if k[0] == "f32" else 2) <= 256 << 20  # the tap stays under 256 MB


def _check_pooled(storage, feat, pooled, b, dev):
    """Check (b) of the module docstring; returns the figures it prints."""
    from nerf_qa_amd import ops
    fmt = STORAGE[storage][3]
    ref = P.pool_ref(feat)
    if fmt is None:  # float
        err = ((pooled.double() - ref).abs() / P.float_ulp(ref)).max().item()
        assert err <= 1.0, f"float pooled map {err:.3f} ulp from the float64 value"
        return f"max {err:.3f} float ulp"
    if fmt == "split16":
        dec = ops.split16_decode(pooled).double()
        over = ((dec - ref).abs() / (2.0 ** -21 * ref + 2.0 ** -24)).max().item()
        assert over <= 1.0, f"split16 pooled map at {over:.3f} of its bound"
        if storage == "f32s":
            plain, _ = _pool_stats(feat, b, "f32", dev)
            assert torch.equal(pooled.view(torch.int32), ops.split16_encode(plain).view(torch.int32))
        return f"split16 at {over:.3f} of 2^-21 |ref| + 2^-24"
    ok, near = P.stored_check(pooled, ref, fmt)
    share = near.double().mean().item()
    assert share <= 0.01, f"{share:.2e} of the case are near ties"
    bad = int((~ok).sum())
    assert bad == 0, f"{bad} pooled values are not the float64 value rounded to {fmt}"
    return f"near ties {share:.1e}, off-nearest among them {int((pooled.double() != P.round_to(ref, fmt)[0]).sum())}"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_exact_sums_and_pooled_map(case, dev):
    """(a) and (b)."""
    storage, c, (b, h, w) = case
    feat = P.exact_maps(2 * b, (h, w), c, 31 * h + w + c, device=dev).to(STORAGE[storage][1])
    pooled, sums = _pool_stats(feat, b, storage, dev)
    want = P.sums_ref(feat, b)
    mism = int((sums != want).sum())
    print(f"\npool_stats exact {_id(case)}: TR/TC/tiles_x/tiles/grid {_grid(storage, c, (b, h, w))}; sums differing {mism}")
    assert torch.equal(sums, want), f"{mism} of {sums.numel()} sums are not bit-equal to the float64 sums"
    assert not sums[:, P.DEAD_BOTH].any() and not sums[:, P.DEAD_X, [0, 2, 4]].any()
    print("   pooled: " + _check_pooled(storage, feat, pooled, b, dev))


def _yardstick(feat, sums, b, npx, label):
    """Check (c): S1 / S2 from the kernel's sums against the float64 formula on the stored values, bounded by the float32
    numpy replay of the same formula (floored at 2^-22), over the ordinary channels and the nearly constant one apart."""
    w1, w2 = P.s_ref(feat, b, np.float64)
    f1, f2 = P.s_ref(feat, b, np.float32)
    g1, g2 = (t.cpu().numpy() for t in P.s_from_sums(sums, npx))
    assert np.isfinite(g1).all() and np.isfinite(g2).all()
    c = feat.shape[-1]
    groups = {"ordinary": [k for k in range(c) if k != P.FLAT], "flat": [P.FLAT]}
    for name, ch in groups.items():
        e1, e2 = np.abs(g1 - w1)[:, ch].max(), np.abs(g2 - w2)[:, ch].max()
        replay = max(np.abs(f1 - w1)[:, ch].max(), np.abs(f2 - w2)[:, ch].max())
        bound = max(float(replay), P.FLOOR)
        if name == "flat":  # where float32 loses the channel, the kernels' own arithmetic still bounds them (docstring, (c))
            bound = min(bound, 2.0 ** -16)
        print(f"\n{label} [{name} channels] |dS1|={e1:.2e} |dS2|={e2:.2e} float32 replay={replay:.2e} bound={bound:.2e}")
        assert max(e1, e2) <= bound, (name, e1, e2, bound)
    dead = list(range(0, c, 7))
    assert (g1[:, dead] == 1.0).all() and (g2[:, dead] == 1.0).all()  # dead in both: (0 + c) / (0 + c)


@pytest.mark.parametrize("case", REALISTIC, ids=_id)
def test_realistic_values_against_float64(case, dev):
    storage, c, (b, h, w) = case
    feat = P.realistic_maps(2 * b, (h, w), c, 7 * h + w + c).to(STORAGE[storage][1])
    on_dev = feat.to(dev)
    pooled, sums = _pool_stats(on_dev, b, storage, dev)
    _yardstick(feat, sums, b, h * w, f"pool_stats {_id(case)} grid {_grid(storage, c, (b, h, w))}")
    # the pooled map is nqa_l2pool's, bit for bit (as the forwards' tests hold it), whatever the values
    from nerf_qa_amd import ops
    if not STORAGE[storage][2]:
        assert torch.equal(pooled.view(torch.int16 if pooled.element_size() == 2 else torch.int32),
                           ops.l2pool(on_dev, STORAGE[storage][0]).view(torch.int16 if pooled.element_size() == 2 else torch.int32))
    else:
        assert torch.equal(pooled.view(torch.int32), ops.l2pool_f16_to_split16(on_dev).view(torch.int32))


def test_stats_nhwc_shapes_reach_their_regimes():
    """From nqa_stats_nhwc_grid: a strip shorter than one pass of the block, a ragged last block, and threads of one block
    holding different item counts; 4 items per thread at the small maps and more at the large ones."""
    from nerf_qa_amd import ops
    short = ragged = uneven = long_ = False
    print("\npixels per block / blocks per pair / pixels side by side of every stats_nhwc case:")
    for prec in NHWC_STORAGE:
        for b, hw, c in NHWC_SHAPES:
            upb, nblk, pl = ops.stats_nhwc_grid(b, hw, c, prec)
            print(f"  {prec} {(b, hw, c)}: {(upb, nblk, pl)}")
            assert pl == P.pl_of(c, prec) and nblk == -(-hw // upb) and upb // pl <= 16
            last = hw - (nblk - 1) * upb
            short |= hw < pl
            ragged |= nblk > 1 and last < upb
            uneven |= last % pl != 0 and last > pl
            long_ |= upb // pl > 4
    assert short and ragged and uneven and long_


@pytest.mark.parametrize("prec", NHWC_STORAGE)
@pytest.mark.parametrize("shape", NHWC_SHAPES, ids=lambda s: "B%d_hw%d_c%d" % s)
def test_stats_nhwc_exact_sums(shape, prec, dev):
    b, hw, c = shape
    feat = P.exact_maps(2 * b, (hw,), c, hw + c, device=dev).to(STORAGE[prec][1])
    sums = _stats_nhwc(feat, b, prec, dev)
    want = P.sums_ref(feat, b)
    mism = int((sums != want).sum())
    assert torch.equal(sums, want), f"{mism} of {sums.numel()} sums are not bit-equal to the float64 sums"
    if prec == "f32":  # the same kernel under "f32s" (float taps)
        assert torch.equal(_stats_nhwc(feat, b, "f32s", dev), sums)


@pytest.mark.parametrize("prec", NHWC_STORAGE)
@pytest.mark.parametrize("shape", NHWC_SHAPES, ids=lambda s: "B%d_hw%d_c%d" % s)
def test_stats_nhwc_realistic_values_against_float64(shape, prec, dev):
    from nerf_qa_amd import ops
    b, hw, c = shape
    feat = P.realistic_maps(2 * b, (hw,), c, 3 * hw + c).to(STORAGE[prec][1])
    sums = _stats_nhwc(feat.to(dev), b, prec, dev)
    _yardstick(feat, sums, b, hw, f"stats_nhwc {prec} {shape} grid {ops.stats_nhwc_grid(b, hw, c, prec)}")


PROPERTY_POOL = [("f32", 64, (3, 37, 67)), ("f32s", 512, (3, 37, 11)), ("f16", 128, (3, 37, 67)), ("bf16", 256, (3, 37, 35)),
                 ("f16x", 64, (3, 37, 131)), ("f16", 512, (2, 128, 120))]
PROPERTY_NHWC = [("f32", (3, 1551, 256)), ("f16", (2, 77, 512)), ("bf16", (2, 35, 64)), ("f32", (2, 6007, 512))]
SWAP = [1, 0, 3, 2, 4]


def _properties(run, feat, b, same_plan):
    """(e) for one operator: run(feat, b) -> (pooled or None, sums).  same_plan: the grid query reports the same split into
    blocks for this pair alone as for the batch."""
    x, y = feat[:b], feat[b:]
    p, s = run(feat, b)
    q, t = run(feat, b)
    assert torch.equal(t, s) and (p is None or torch.equal(q.view(torch.uint8), p.view(torch.uint8)))  # two launches
    p2, s2 = run(torch.cat([y, x]), b)
    assert torch.equal(s2, s[..., SWAP]), "swapping x and y does not swap the columns bit for bit"
    if p is not None:
        assert torch.equal(p2[:b].view(torch.uint8), p[b:].view(torch.uint8)) and torch.equal(p2[b:].view(torch.uint8), p[:b].view(torch.uint8))
    p3, s3 = run(torch.cat([x, x]), b)
    assert torch.equal(s3[..., 0], s3[..., 1]) and torch.equal(s3[..., 2], s3[..., 3]) and torch.equal(s3[..., 2], s3[..., 4])
    assert torch.equal(s3[..., [0, 2]], s[..., [0, 2]])
    if p is not None:
        assert torch.equal(p3[:b].view(torch.uint8), p3[b:].view(torch.uint8)) and torch.equal(p3[:b].view(torch.uint8), p[:b].view(torch.uint8))
    assert not torch.equal(s[..., 0], s[..., 1])
    i = b - 1
    p4, s4 = run(torch.cat([x[i:i + 1], y[i:i + 1]]), 1)
    if p is not None:  # (the pooled map has no summation order to depend on)
        assert torch.equal(p4[0].view(torch.uint8), p[i].view(torch.uint8)) and torch.equal(p4[1].view(torch.uint8), p[b + i].view(torch.uint8))
    if same_plan:
        assert torch.equal(s4[0], s[i]), "a pair's sums depend on its batch neighbours"


@pytest.mark.parametrize("case", PROPERTY_POOL, ids=_id)
def test_pool_stats_exact_properties(case, dev):
    storage, c, (b, h, w) = case
    feat = P.realistic_maps(2 * b, (h, w), c, 5 + h + c, device=dev).to(STORAGE[storage][1])
    same = _grid(storage, c, (b, h, w))[:4] == _grid(storage, c, (1, h, w))[:4]
    assert same or (b, h, w) == (2, 128, 120)  # (only the tall case changes its tile height with the batch)
    _properties(lambda f, n: _pool_stats(f.contiguous(), n, storage, dev), feat, b, same)


@pytest.mark.parametrize("case", PROPERTY_NHWC, ids=lambda k: "%s_B%d_hw%d_c%d" % (k[0], *k[1]))
def test_stats_nhwc_exact_properties(case, dev):
    from nerf_qa_amd import ops
    prec, (b, hw, c) = case
    feat = P.realistic_maps(2 * b, (hw,), c, 9 + hw + c, device=dev).to(STORAGE[prec][1])
    same = ops.stats_nhwc_grid(b, hw, c, prec) == ops.stats_nhwc_grid(1, hw, c, prec)
    assert same or hw == 6007  # (only the long strips change their length with the batch)
    _properties(lambda f, n: (None, _stats_nhwc(f.contiguous(), n, prec, dev)), feat, b, same)
