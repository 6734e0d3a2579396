"""The reference figures behind tests/test_gpu_mixed_layers.py, recomputed without a GPU, and the proof that its checks
have teeth: a float32 replay of a two-term layer that loses its `lo` term -- everywhere, or in one tap of nine -- falls
outside the envelope and over the share cap that the correct replay meets with room to spare."""
import pytest
import torch

import mixed_refs as R

# What the GPU module's docstring quotes, recomputed below.  The float32 replays go through torch's CPU convolution, whose
# summation order (and use of FMA) depends on the CPU: the largest rounding error over a map moves by ten per cent and
# more with it, so the figures are pinned to a band of 1.5 either way -- enough to show a change of the stand-in weights,
# the inputs or the replay's arithmetic, which moves them by far more.  The GPU tests take their bars from the replay
# as they run, not from these constants.
REPLAY_C = (2.22, 5.34)           # float32 two-term replay, |acc - pre| / (2^-24 mag): smallest and largest case maximum
REPLAY_C_BIG = 6.11               # ... on BIG_CASE, which carries its own c
REPLAY_SHARE_MAX = 3.93e-3        # ... share of outputs differing from f16(relu(pre))
CONV1_1_C = (2.50, 4.27)
FUSED_OWN = (2.63e-4, 2.20e-4, 4.30e-4, 4.01e-4)  # float32 replay of the fused stage 1, of the maximum, per FUSED_SHAPES
FUSED_SHARE = (5.98e-3, 3.00e-3, 6.46e-3, 5.55e-3)  # ... share of its halves differing from the float64 replay's
POOL_OWN = (1.24e-7, 6.2e-8, 8.4e-8, 1.05e-7)     # float32 L2-pool oracle, of the maximum, per POOL_SHAPES
SHARE_CAP = 1e-2
CASES = R.CONV_CASES + [(4, 2, 9, 33), R.BIG_CASE]


def _near(got, want, band=1.5):
    return want / band <= got <= want * band


@pytest.fixture(scope="module")
def replays():
    out = {}
    for case in CASES:
        a = R.relu_like_input(*case)
        out[case] = (a, *R.conv_layer_ref(a, *R.convs()[case[0]]))
    return out


def test_two_term_replay_figures(replays):
    cs = {case: R.replay_constant(pre, mag, acc) for case, (_, pre, mag, acc) in replays.items()}
    shares = {case: R.share_differing(R.to_half(acc.clamp_min(0)), pre) for case, (_, pre, mag, acc) in replays.items()}
    print("\n" + "\n".join(f"{case}: {cs[case]:.2f} x 2^-24 mag, share {shares[case]:.2e}" for case in CASES))
    big = cs.pop(R.BIG_CASE)
    assert _near(min(cs.values()), REPLAY_C[0]) and _near(max(cs.values()), REPLAY_C[1]), (min(cs.values()), max(cs.values()))
    assert _near(big, REPLAY_C_BIG), big
    assert _near(max(shares.values()), REPLAY_SHARE_MAX), max(shares.values())
    assert max(shares.values()) < SHARE_CAP / 2 and 3 * max(big, *cs.values()) < 230 / 5  # far below a lost lo tap (230 ...)


@pytest.mark.parametrize("case", [c for c in R.CONV_CASES if c != (12, 1, 1, 1)], ids=lambda c: "x".join(map(str, c)))
def test_a_lost_lo_term_fails_both_checks(case, replays):
    a, pre, mag, acc = replays[case]
    c = 3 * REPLAY_C[1]  # (the constant of these cases; BIG_CASE's is larger)
    lo, hi = R.half_envelope(pre, mag, c)
    good = R.to_half(acc.clamp_min(0))
    assert ((good >= lo) & (good <= hi)).all()
    for drop in ("all", (0, 0), (1, 1), (2, 1)):
        _, _, bad = R.conv_layer_ref(a, *R.convs()[case[0]], drop_lo=drop)
        assert R.replay_constant(pre, mag, bad) > 10 * c, drop  # hundreds of 2^-24 mag against c = 16
        badh = R.to_half(bad.clamp_min(0))
        outside = float(((badh < lo) | (badh > hi)).double().mean())
        share = R.share_differing(badh, pre)
        print(f"\n{case} lo lost {drop}: {outside:.2e} outside the envelope, {share:.2e} differ from f16(relu(pre))")
        assert outside > 0 and share >= 7 * SHARE_CAP, (drop, outside, share)


def test_one_pixel_map_sees_only_the_centre_tap(replays):
    """(12, 1, 1, 1): all eight outer taps meet padding, so only a fault in the centre tap can show there."""
    a, pre, mag, acc = replays[(12, 1, 1, 1)]
    _, _, bad = R.conv_layer_ref(a, *R.convs()[12], drop_lo=(1, 1))
    lo, hi = R.half_envelope(pre, mag, 3 * REPLAY_C[1])
    badh = R.to_half(bad.clamp_min(0))
    assert ((badh < lo) | (badh > hi)).any()


def test_conv1_1_replay_figures():
    cs = [R.replay_constant(*R.conv1_1_ref(R.image(s))) for s in R.STAGE1_SHAPES]
    print("\nconv1_1 float32 replay:", ", ".join(f"{c:.2f}" for c in cs))
    assert _near(min(cs), CONV1_1_C[0]) and _near(max(cs), CONV1_1_C[1]), cs


@pytest.mark.parametrize("i", range(len(R.FUSED_SHAPES)), ids=["x".join(map(str, s)) for s in R.FUSED_SHAPES])
def test_fused_stage1_replay_figures_and_a_lost_lo_term(i):
    """The relative-to-maximum bar of the fused stage 1 cannot see a lost lo term; the share cap beside it does."""
    x = R.image(R.FUSED_SHAPES[i], 21)
    r64 = R.fused_stage1_ref(x, torch.float64)
    r32 = R.to_half(R.fused_stage1_ref(x, torch.float32))
    own, share = R.rel_to_max(r32, r64), R.share_of_halves_differing(r32, r64)
    print(f"\nfused stage 1 {R.FUSED_SHAPES[i]}: float32 replay {own:.2e} of the maximum, {share:.2e} of its halves differ")
    assert _near(own, FUSED_OWN[i]) and _near(share, FUSED_SHARE[i]), (own, share)
    for drop in ((0,), (1,), (0, 1)):
        bad = R.to_half(R.fused_stage1_ref(x, torch.float32, drop_lo=drop))
        e, sh = R.rel_to_max(bad, r64), R.share_of_halves_differing(bad, r64)
        print(f"   lo lost in convolution(s) {drop}: {e:.2e} of the maximum, {sh:.2e} differ (cap {4 * share:.2e})")
        assert e <= 4 * own  # (why the first bar is not enough)
        assert sh > 5 * 4 * share, (drop, sh, share)


def test_boundary_pool_reference_figures():
    for shape, want in zip(R.POOL_SHAPES, POOL_OWN):
        a = R.pool_input(*shape)
        p64, p32 = R.pool_refs(a)
        own = R.rel_to_max(p32, p64)
        # what a correct kernel stores: the float32 value as split16 (hi = half(v), lo = half(v - hi))
        hi = p32.half().float()
        dec = (hi + (p32 - hi).half().float()).double()
        emu = R.rel_to_max(dec, p64)
        print(f"\npool {shape}: float32 oracle {own:.2e}, as split16 {emu:.2e}, bar {4 * own:.2e}")
        assert _near(own, want) and emu <= 0.75 * 4 * own, (own, emu)  # a correct store meets the bar with room
        for ch in (3, 5):  # below 2^-14: a subnormal half hi, lo = 0 -> absolute 2^-25
            assert float(p64[:, ch].max()) < 2.0 ** -14
            assert float((dec[:, ch] - p64[:, ch]).abs().max()) <= 2.0 ** -25 and (dec[:, ch] > 0).all()
