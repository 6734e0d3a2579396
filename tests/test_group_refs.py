"""tests/group_refs.py on the CPU, on the reference alone: what tests/test_gpu_group_stats_exact.py relies on.

  - the inputs are what their docstring says (quarter steps in [0, 4], the dead channels, the identical render), exact
    in f16 and bf16, and the float64 sums agree with an independent per-pair evaluation by pool_refs.sums_ref;
  - each MODEL ERROR a group kernel could make fails bit equality in at least one of the five sums of every pair it
    touches: the last pixel dropped, one strip item counted twice, a render taken from the neighbouring group, the rows
    of two renders of a group exchanged, the reference strip of block blk used for block blk + 1;
  - the S criterion |got - ref| <= 2^-23 |ref| + 2^-40 holds for a float64 replay of finalize_kernel's own order rounded
    to float32 (group_refs.s_finalize) against pool_refs.s_from_sums: at most 0.50 of the bound over the shapes of
    tests/test_gpu_group_stats.py, which is the float rounding itself;
  - a dropped last pixel is far outside that criterion: of the (pair, channel) entries it can move at all, over 90 %
    (measured: every one, at all seven shapes) move by more than twice the bound.  It cannot move every entry of the table: a pair whose
    render is its reference keeps S1 = S2 = 1.0 whatever pixels are summed (which is why the GPU test also holds those
    rows' sum x^2, sum y^2 and sum xy equal bit for bit), and where the last pixel is zero in both maps (0.4 * 0.4 = 16 %
    of the entries) no sum changes.  Over ALL entries of the other renders the share is 83 to 85 %, which the test
    asserts as well (>= 80 %); the sums themselves differ in EVERY pair (the bit-equality check above).
"""
import functools

import pytest
import torch

import group_refs as G
import pool_refs as P

SHAPES = [(1, 1, 1, 64), (2, 3, 35, 64), (1, 5, 299, 128), (3, 2, 1551, 256), (2, 4, 77, 512), (1, 2, 6007, 512),
          (1, 2, 24589, 512)]  # tests/test_gpu_group_stats.py's NHWC_SHAPES
IDS = ["R%dK%d_hw%d_c%d" % s for s in SHAPES]


@functools.lru_cache(maxsize=None)
def _case(shape):
    R, K, hw, c = shape
    feat = G.group_exact_maps(R, K, hw, c, 1000 + hw + c)
    return feat, G.group_sums_ref(feat, R, K)


def _pairs_differ(a, b):
    """Per pair: whether any of its (channel, sum) entries differs in bits."""
    return (a != b).flatten(1).any(1)


@pytest.mark.parametrize("shape", SHAPES + [(2, 3, 35, 3), (2, 1, 9, 64)], ids=IDS + ["planes", "K1"])
def test_inputs_are_what_the_docstring_says(shape):
    R, K, hw, c = shape
    feat = G.group_exact_maps(R, K, hw, c, 5)
    assert feat.shape == (R + R * K, hw, c) and feat.dtype == torch.float32
    assert torch.equal(feat * 4, (feat * 4).round()) and feat.min() == 0 and feat.max() <= 4
    assert torch.equal(feat.half().float(), feat) and torch.equal(feat.bfloat16().float(), feat)
    if hw * c >= 2000:
        assert 0.35 < (feat[:, :, -1] == 0).float().mean() < 0.45
    (both, dead_x, ren0), groups = G.special_channels(c)
    ref, ren = feat[:R], feat[R:].view(R, K, hw, c)
    for r in range(R):
        special = groups is None or r < groups
        live = hw * c < 200 or (ref[r].amax(0) > 0).all()
        if special:
            assert not ref[r, :, both].any() and not ren[r, :, :, both].any()
            assert not ref[r, :, dead_x].any() and not ren[r, 0, :, ren0].any()
            if hw >= 9:
                assert ren[r, 0, :, dead_x].any()
                assert ref[r, :, ren0].any()
                if K >= 3:
                    assert ren[r, 1, :, ren0].any()
        elif hw >= 9:
            assert live and (ren[r].amax(1) > 0).all()
        if K >= 2:
            assert torch.equal(ren[r, K - 1], ref[r])
            if hw >= 9:
                assert not torch.equal(ren[r, 0], ref[r])
    if R >= 2 and hw >= 9:
        assert not torch.equal(ref[0], ref[1])
    assert torch.equal(G.group_exact_maps(R, K, hw, c, 5), feat) and not torch.equal(G.group_exact_maps(R, K, hw, c, 6), feat)


@pytest.mark.parametrize("shape", SHAPES[:5], ids=IDS[:5])
def test_sums_agree_with_the_pairwise_reference(shape):
    R, K, hw, c = shape
    feat, sums = _case(shape)
    assert sums.shape == (R * K, c, 5) and sums.dtype == torch.float64
    pairs = torch.cat([feat[:R].repeat_interleave(K, 0), feat[R:]])
    assert torch.equal(sums, P.sums_ref(pairs, R * K))
    assert torch.equal(sums * 16, (sums * 16).round()) and sums.max() < 2.0 ** 40  # multiples of 1/16, far below 2^53
    assert not sums[:, G.DEAD_BOTH].any() and not sums[:, G.DEAD_X, [0, 2, 4]].any()
    rows0 = torch.arange(R) * K
    assert not sums[rows0][:, G.DEAD_REN0, [1, 3, 4]].any() and (hw < 9 or sums[rows0][:, G.DEAD_REN0, 0].all())
    if K >= 2:
        same = sums[rows0 + K - 1]
        assert torch.equal(same[..., 0], same[..., 1]) and torch.equal(same[..., 2], same[..., 3]) and torch.equal(same[..., 2], same[..., 4])


def test_every_model_error_fails_bit_equality():
    seen = {"drop": 0, "double": 0, "neighbour": 0, "rows": 0, "strip": 0}
    for shape in SHAPES:
        R, K, hw, c = shape
        feat, sums = _case(shape)
        if hw > 1:
            assert _pairs_differ(G.drop_last_pixel(feat, R, K), sums).all(), shape
            seen["drop"] += 1
        for pixel in {0, hw // 2, hw - 1}:
            assert _pairs_differ(G.double_item(feat, R, K, pixel), sums).all(), (shape, pixel)
            seen["double"] += 1
        if R >= 2:
            assert _pairs_differ(G.neighbour_group(feat, R, K), sums).all(), shape
            seen["neighbour"] += 1
        if K >= 2:
            d = _pairs_differ(G.rows_exchanged(feat, R, K, 0, K - 1), sums).view(R, K)
            assert d[:, 0].all() and d[:, K - 1].all() and int(d.sum()) == 2 * R, shape
            seen["rows"] += 1
            if K >= 3:
                d = _pairs_differ(G.rows_exchanged(feat, R, K, 0, 1), sums).view(R, K)
                assert d[:, 0].all() and d[:, 1].all() and int(d.sum()) == 2 * R, shape
        for prec in ("f32", "f16"):
            for items in (4, 16):
                ppb = items * P.pl_of(c, prec)
                if hw > ppb:
                    assert _pairs_differ(G.stale_strip(feat, R, K, ppb), sums).all(), (shape, prec, items)
                    seen["strip"] += 1
    assert min(seen.values()) >= 3, seen


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_the_finalisation_replay_meets_the_s_criterion_and_a_dropped_pixel_does_not(shape):
    R, K, hw, c = shape
    feat, sums = _case(shape)
    r1, r2 = P.s_from_sums(sums, hw)
    g1, g2 = G.s_finalize(sums, hw)
    assert g1.dtype == torch.float32 and g2.dtype == torch.float32
    e1, e2 = G.s_excess(g1, r1), G.s_excess(g2, r2)
    print(f"\nfinalize replay {shape}: S1 at {e1:.3f}, S2 at {e2:.3f} of 2^-23 |ref| + 2^-40")
    assert max(e1, e2) <= 1.0
    if K >= 2:  # the identical render: exactly 1.0 in the replay and in the reference
        rows = torch.arange(R) * K + K - 1
        assert (g1[rows] == 1.0).all() and (g2[rows] == 1.0).all() and (r1[rows] == 1.0).all() and (r2[rows] == 1.0).all()
    assert (g1[:, G.DEAD_BOTH] == 1.0).all() and (g2[:, G.DEAD_BOTH] == 1.0).all()
    if hw == 1:
        return
    dropped = G.drop_last_pixel(feat, R, K)
    d1, d2 = G.s_finalize(dropped, hw)  # (the kernel still divides by HW)
    moved = ((d1.double() - r1).abs() > 2 * G.s_bound(r1)) | ((d2.double() - r2).abs() > 2 * G.s_bound(r2))
    can_move = (dropped != sums).any(-1)
    other = torch.ones(R, K, dtype=torch.bool)
    if K >= 2:
        other[:, K - 1] = False  # (S of a render that IS its reference is 1.0 whatever is summed)
        assert not moved.view(R, K, c)[:, K - 1].any()
    other = other.view(R * K, 1).expand(R * K, c)
    assert not (moved & ~can_move).any()
    of_movable = moved[can_move & other].double().mean().item()
    of_all = moved[other].double().mean().item()
    print(f"   last pixel dropped: {of_movable:.3f} of the entries whose sums change, {of_all:.3f} of all entries of the other renders, "
          f"move S by more than twice the bound")
    assert of_movable > 0.9 and of_all >= 0.8
