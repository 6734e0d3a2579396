"""tests/pool_refs.py without a GPU: the float64 pooled map against oracle.dists_oracle.l2pool, the float64 sums against
oracle.dists_oracle.dists_stats through the S1 / S2 formula, the 16-bit rounding helper against the conversions of numpy
and torch, the preconditions of the exact inputs, and the two facts tests/test_gpu_pool_stats.py leans on:

  - the pooled values of the exact inputs are near a 16-bit rounding tie (where the GPU test accepts either neighbour) in
    far under 1 % of a case;
  - SANITY OF THE BIT-EQUAL CHECK: a reference that drops one border row, or counts one 2 x 2 block twice, is not bit-equal
    to the reference -- in every live channel -- so a kernel doing either cannot pass check (a) of the GPU test.
"""
import numpy as np
import pytest
import torch

import pool_refs as P


@pytest.mark.parametrize("h,w", [(1, 1), (2, 2), (1, 9), (9, 1), (3, 3), (5, 7), (4, 6), (37, 67), (36, 64)])
def test_pooled_reference_is_the_oracles_l2pool(h, w):
    feat = P.realistic_maps(4, (h, w), 16, 100 + h * w)
    want = dists_l2pool(feat)
    got = P.pool_ref(feat)
    assert got.shape == (4, (h + 1) // 2, (w + 1) // 2, 16) and got.dtype == torch.float64
    err = ((got - want).abs() / want).max().item()
    print(f"\npool_ref vs oracle l2pool {h}x{w}: max relative difference {err:.2e}")
    assert err <= 2.0 ** -50  # two float64 summation orders of nine non-negative terms, then a square root


def dists_l2pool(feat):
    from oracle import dists_oracle
    return dists_oracle.l2pool(feat.double().permute(0, 3, 1, 2)).permute(0, 2, 3, 1)


@pytest.mark.parametrize("kind", ["exact", "realistic"])
def test_sums_reference_gives_the_oracles_similarities(kind):
    from oracle import dists_oracle
    b, h, w, c = 3, 9, 13, 24
    feat = (P.exact_maps if kind == "exact" else P.realistic_maps)(2 * b, (h, w), c, 7)
    sums = P.sums_ref(feat, b)
    assert sums.shape == (b, c, 5) and sums.dtype == torch.float64
    s1, s2 = P.s_from_sums(sums, h * w)
    x, y = feat[:b].double().permute(0, 3, 1, 2), feat[b:].double().permute(0, 3, 1, 2)
    w1, w2 = dists_oracle.dists_stats([x], [y])
    e1, e2 = (s1 - w1).abs().max().item(), (s2 - w2).abs().max().item()
    print(f"\nS1 / S2 from the raw float64 sums vs dists_stats [{kind}]: {e1:.2e} {e2:.2e}")
    # float64 throughout; the raw-moment variance of the nearly constant channel (mean 2, variance 1e-7) cancels ~26 bits
    assert e1 <= 1e-14 and e2 <= 1e-8
    live = [k for k in range(c) if k != P.FLAT]
    assert (s2 - w2)[:, live].abs().max().item() <= 1e-12
    n1, n2 = P.s_ref(feat, b, np.float64)
    assert np.abs(n1 - w1.numpy()).max() <= 1e-14 and np.abs(n2 - w2.numpy()).max() <= 1e-12
    # the layout a (2b, HW, C) map has is the same sums
    assert torch.equal(P.sums_ref(feat.reshape(2 * b, h * w, c), b), sums)


def test_exact_inputs_are_what_the_argument_needs():
    v = P.exact_maps(6, (11, 13), 64, 3)
    assert v.dtype == torch.float32 and torch.equal(v * 4, (v * 4).round()) and v.min() == 0 and v.max() == 4
    zeros = (v == 0).float().mean().item()
    assert 0.35 < zeros < 0.5
    assert not v[..., P.DEAD_BOTH].any() and not v[:3, ..., P.DEAD_X].any() and v[3:, ..., P.DEAD_X].any()
    assert not torch.equal(v[:3], v[3:])
    for dt in (torch.float16, torch.bfloat16):  # stored without rounding in every storage type
        assert torch.equal(v.to(dt).float(), v)
    # every window sum is a multiple of 1/256 of at most 16, and float64 == float32 arithmetic on it
    acc = P.pool_ref(v) ** 2 - 1e-12
    k = (acc * 256).round()
    assert (acc * 256 - k).abs().max().item() < 1e-6 and k.max().item() <= 4096
    # sums of squares stay far inside a float: 64 samples of at most 16, in units of 1/16
    assert 64 * 16 * 16 < 2 ** 24


def test_rounding_helper_is_the_conversion_of_numpy_and_torch():
    g = torch.Generator().manual_seed(1)
    ref = torch.cat([torch.rand(20000, generator=g, dtype=torch.float64) * 4.5,
                     torch.rand(2000, generator=g, dtype=torch.float64) * 1e-4,
                     torch.tensor([1e-6, 2.0 ** -14, 2.0 ** -24, 1.0, 4.0, 0.0625, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11,
                                   1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8], dtype=torch.float64)])
    ref = ref[ref > 0]
    near16 = P.round_to(ref, "f16")
    assert torch.equal(near16[0], torch.from_numpy(ref.numpy().astype(np.float16).astype(np.float64)))
    assert (near16[1] <= ref).all() and (ref < near16[2]).all()
    f32 = ref.float()  # torch rounds float -> bfloat16 to nearest even: compare on float-representable values
    nearb = P.round_to(f32.double(), "bf16")
    assert torch.equal(nearb[0], f32.bfloat16().double())
    # exact ties are flagged and resolved to even; values a quarter step off are not flagged
    tie = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -12], dtype=torch.float64)
    n, lo, hi, near = P.round_to(tie, "f16")
    assert near.tolist() == [True, True, False] and n.tolist() == [1.0, 1.0 + 2.0 ** -9, 1.0]
    assert P.float_ulp(torch.tensor([1.0, 1.5, 0.99, 1e-6], dtype=torch.float64)).tolist() == \
        [2.0 ** -23, 2.0 ** -23, 2.0 ** -24, 2.0 ** -43]
    ok, _ = P.stored_check(torch.tensor([1.0, 1.0 + 2.0 ** -10, 1.0 + 2.0 ** -9]).half(),
                           torch.full((3,), 1.0 + 2.0 ** -11 * (1 + 2.0 ** -13), dtype=torch.float64), "f16")
    assert ok.tolist() == [True, True, False]


# (storage, C, B, H, W): the all-border maps and the ragged case of tests/test_gpu_pool_stats.py where they are cheap here
NEAR_TIE_CASES = [("f16", 64, 1, 1, 1), ("f16", 64, 1, 5, 7), ("f16", 64, 8, 4, 6), ("bf16", 64, 1, 1, 9), ("f16", 64, 3, 37, 131),
                  ("bf16", 64, 3, 37, 131), ("f16", 512, 3, 37, 19), ("bf16", 512, 2, 36, 16), ("f16", 128, 2, 36, 64)]


@pytest.mark.parametrize("fmt,c,b,h,w", NEAR_TIE_CASES, ids=lambda v: str(v))
def test_near_ties_of_the_exact_inputs_stay_under_one_percent(fmt, c, b, h, w):
    ref = P.pool_ref(P.exact_maps(2 * b, (h, w), c, 1000 + h * w + c))
    share = P.round_to(ref, fmt)[3].double().mean().item()
    print(f"\nnear-tie share of the pooled exact inputs {fmt} C={c} {b}x{h}x{w}: {share:.2e}")
    assert share <= 0.01


def test_near_ties_over_every_window_sum():
    """A non-zero window of the exact inputs sums to k / 256, k = 1..4096, and pools to sqrt(k) / 16: the k that are near
    ties are a handful (a perfect square pools to a representable value, anything else to an irrational one that is near
    a midpoint by chance only), and sqrt(1e-12) of an all-zero window is none."""
    for fmt in P.FORMATS:
        ks = P.window_sum_near_ties(fmt)
        print(f"\n{fmt}: near-tie window sums k/256 for k in {ks}")
        assert len(ks) <= 41  # 1 % of the 4096 values
        assert not P.round_to(torch.tensor([1e-6], dtype=torch.float64), fmt)[3].item()


@pytest.mark.parametrize("h,w", [(37, 67), (5, 7), (36, 64)])
def test_a_dropped_row_or_a_doubled_block_is_not_bit_equal(h, w):
    b, c = 3, 64
    feat = P.exact_maps(2 * b, (h, w), c, 11)
    want = P.sums_ref(feat, b)
    live = [k for k in range(c) if k not in (P.DEAD_BOTH, P.DEAD_X)]
    dropped = P.sums_ref(P.drop_last_row(feat), b)
    assert not torch.equal(dropped, want)
    assert (dropped[:, live, :2] != want[:, live, :2]).all()  # every live channel's sum x and sum y move
    assert torch.equal(dropped[:, P.DEAD_BOTH], want[:, P.DEAD_BOTH])  # (a dead channel cannot show it: the rest do)
    # one pooled pixel's own 2 x 2 block counted twice, at a corner, on the bottom edge and inside
    for y0, x0 in ((0, 0), (h - 1 - (h - 1) % 2, 2), (2, 2 * ((w - 1) // 2))):
        doubled = P.double_count_block(feat, b, y0, x0)
        moved = (doubled != want).any(-1)  # (b, C): some sum of the channel differs
        assert not torch.equal(doubled, want)
        # a block that is zero in a channel cannot move it; with 40 % zeros that is 0.4^4 of the 2 x 2 blocks
        assert moved[:, live].float().mean().item() > 0.9, (y0, x0)
    # and a pixel booked to the wrong pair: swapping two pairs' x maps moves sum xy and leaves sum x of the batch alone
    swapped = feat.clone()
    swapped[[0, 1]] = feat[[1, 0]]
    got = P.sums_ref(swapped, b)
    assert (got[:2, live, 4] != want[:2, live, 4]).all() and torch.equal(got[2], want[2])
