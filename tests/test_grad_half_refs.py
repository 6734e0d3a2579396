"""The half gradient chain's yardstick (tests/grad_half_refs.py) proved on the CPU.

With its roundings switched off the emulation IS grad_replay.replay: every step differs from the replay's by an exact
power of two per image, so the two agree to float64 rounding (1e-12 of the largest gradient and of the rms).  With the
roundings on it stays within e_max <= 2e-3 and e_rms <= 2e-3 of the exact replay on DISTS' own tap gradients -- a guard
on the yardstick (twice the worst figure seen when the emulation was written, 1.0e-3), not a bound on any kernel.

Measured here (float64 oracle forward, published alpha / beta; run with -s):
    case                        gain    e_max     e_rms     1 - cosine
    33x47 nerf_white+nerf_float 1.0     3.9e-4    6.5e-4    2.1e-7
    33x47 nerf_white+nerf_float 1.3     5.5e-4    7.2e-4    2.6e-7
    40x56 noise10+blur          1.0     5.5e-4    5.8e-4    1.7e-7
    40x56 noise10+blur          1.3     7.8e-4    6.8e-4    2.3e-7
    window [8, 16) against [128, 256) on the first case: 1.6e-9 / 5.0e-10 of each other
"""
import pytest
import torch

import grad_half_refs as ghr
import grad_replay

CASES = [  # (h, w, kinds, seeds)
    (33, 47, ("nerf_white", "nerf_float"), (11, 12)),
    (40, 56, ("noise10", "blur"), (11, 12)),
]
IDS = ["33x47-nerf", "40x56-texture"]


@pytest.mark.parametrize("h,w,kinds,seeds", CASES, ids=IDS)
def test_without_rounding_the_emulation_is_the_replay(h, w, kinds, seeds):
    acts, taps, g_taps, convs = ghr.oracle_case(h, w, kinds, seeds)
    exact = grad_replay.replay(acts, taps, g_taps, convs, torch.float64)
    for top in (ghr.WINDOW_TOP, 8):  # the window does not matter either
        got = ghr.replay_half(acts, taps, g_taps, convs, rounding=False, top=top)
        assert got.dtype == torch.float64 and got.shape == exact.shape and torch.isfinite(got).all()
        e_max, e_rms = grad_replay.errors(got, exact)
        print(f"\n[half refs] {h}x{w} {'+'.join(kinds)} no rounding, window top 2^{top}: e_max {e_max:.2e} e_rms {e_rms:.2e}")
        assert e_max <= 1e-12 and e_rms <= 1e-12, (e_max, e_rms)
    # and on dense random tap gradients, which reach every mask
    gen = torch.Generator().manual_seed(5)
    g_rand = [torch.randn(t.shape, generator=gen, dtype=torch.float64) for t in taps]
    e_max, e_rms = grad_replay.errors(ghr.replay_half(acts, taps, g_rand, convs, rounding=False),
                                      grad_replay.replay(acts, taps, g_rand, convs, torch.float64))
    assert e_max <= 1e-12 and e_rms <= 1e-12, (e_max, e_rms)


@pytest.mark.parametrize("gain", [1.0, 1.3])
@pytest.mark.parametrize("h,w,kinds,seeds", CASES, ids=IDS)
def test_with_rounding_the_emulation_stays_near_the_replay(h, w, kinds, seeds, gain):
    e_max, e_rms, cgap = ghr.emulation_figures(h, w, kinds, seeds, gain)
    print(f"\n[half refs] {h}x{w} {'+'.join(kinds)} gain {gain}: emulation e_max {e_max:.2e} e_rms {e_rms:.2e} "
          f"1-cos {cgap:.2e}")
    assert 0 < e_max <= 2e-3 and 0 < e_rms <= 2e-3, (e_max, e_rms)
    assert cgap <= 5e-6, cgap


def test_the_window_does_not_change_the_figures():
    """[8, 16) against the split16 chain's [128, 256): halves scale exactly, so unless something leaves the half range
    (nothing does on these weights) the emulation is the same to the bit after the final rescaling."""
    h, w, kinds, seeds = CASES[0]
    acts, taps, g_taps, convs = ghr.oracle_case(h, w, kinds, seeds)
    lo = ghr.replay_half(acts, taps, g_taps, convs, top=4)
    hi = ghr.replay_half(acts, taps, g_taps, convs, top=8)
    assert torch.isfinite(lo).all() and torch.isfinite(hi).all()
    e_max, e_rms = grad_replay.errors(lo, hi)
    print(f"\n[half refs] window [8,16) against [128,256): e_max {e_max:.2e} e_rms {e_rms:.2e}")
    assert e_max <= 1e-4 and e_rms <= 1e-4  # (subnormal halves differ between the windows; everything else is bit-equal)


def test_exponents():
    g = torch.tensor([[8.0, -1.0], [0.0, 0.0], [float("inf"), 1.0], [-15.99, 3.0], [16.0, 1.0], [3e-9, 0.0]], dtype=torch.float64)
    k = ghr.exponents(g.view(6, 2, 1, 1)).flatten().tolist()
    assert k[:5] == [0.0, 0.0, 0.0, 0.0, -1.0]
    assert 8.0 <= 3e-9 * 2.0 ** k[5] < 16.0
