"""tests/stage1_split_refs.py without a GPU: the pixel table replays the kernel's normalisation to exact (hi, lo) levels, the
weights encode to the intended halves, at every shape of tests/test_gpu_stage1_split_exact.py every product of either
layer is a multiple of its quantum with sum |terms| + |bias| below quantum x 2^24 and relu1_1 re-splits to (A, eps) -- so
the float64 reference IS the kernel's float32 arithmetic in any order -- and the reference has power: the share of the
outputs each mutant of stage1_split_refs.MUTANTS changes is printed and must be positive.  Measured on the "split" set
(1x1 | 5x7 | 4x32 | 9x33 | 37x70 | 3x200 | 150x130):
  conv1_1: Wl*Ah dropped                           0.25 | 0.46 | 0.46 | 0.46 | 0.46 | 0.46 | 0.46
  conv1_1: Wh*Al dropped                           0.21 | 0.46 | 0.45 | 0.46 | 0.46 | 0.45 | 0.46
  relu1_1: lo = 0                                  0.30 | 0.46 | 0.46 | 0.46 | 0.46 | 0.46 | 0.46
  relu1_1: lo truncated toward zero                0    | 0    | 0    | 0    | 0    | 0    | 0       (see below)
  conv1_2: Wl*Ah dropped                           0.43 | 0.47 | 0.47 | 0.47 | 0.47 | 0.47 | 0.47
  conv1_2: Wh*Al dropped                           0.30 | 0.46 | 0.46 | 0.46 | 0.46 | 0.46 | 0.46
  conv1_2: cross terms' activation halves swapped  0.45 | 0.48 | 0.47 | 0.47 | 0.48 | 0.48 | 0.48
  halo outside the image left at relu(bias)        0.65 | 0.33 | 0.30 | 0.15 | 0.05 | 0.37 | 0.02
  raw patch's pad channel not finite               0.68 | 0.69 | 0.69 | 0.69 | 0.68 | 0.69 | 0.68
  tile reads the previous tile's halo slot         0.46 | 0.67 | 0.59 | 0.68 | 0.60 | 0.56 | 0.58
(about 0.47 of the outputs are positive: a mutant cannot show under the final ReLU's zero.)

The truncation mutant changes NOTHING, on this set or on any set that is exact: relu1_1's lo half is eps, a multiple of
2^-13 below 2^-10, which is a half as it stands -- a conversion that has nothing to round gives the same half toward zero
as to nearest.  Making lo need a rounding takes a residual of twelve significant bits, i.e. relu1_1 >= 1024 next to
2^-13 (conv1_1's bias x scale then leaves its accumulator's exact range) or levels between the integers (the lone-tap
channels then re-split to something other than (A, eps)).  Its share is asserted to be 0, so that a set on which it could
show does not go unnoticed; test_truncation_differs_where_there_is_something_to_round shows the mutant's conversion itself
is not vacuous.  A finite value in the raw patch's pad channel cannot show either (the blob's weights there are zero);
the mutant is a non-finite one."""
import numpy as np
import pytest
import torch

import persistent_refs as P
import stage1_split_refs as T

_ID = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)  # noqa: E731
ALL_SHAPES = T.SHAPES + (T.RING_SHAPE,)
SILENT = "relu1_1: lo truncated toward zero"


def test_pixel_table_replays_to_exact_levels():
    for c in range(3):
        tab = T.pixel_table()[c]
        raw, hi, lo = T.table_arrays(c)
        levels = {h: [b for b in T.TABLE_B if (h, b) in tab] for h in sorted({k[0] for k in tab})}
        print(f"\n channel {c}: {len(tab)} pixels; hi -> b of lo = b 2^-13: {levels}")
        assert raw.dtype == np.float32 and 0.0 <= raw.min() and raw.max() <= 1.0
        v = T.normalise(raw, c)
        assert v.dtype == np.float32 and np.array_equal(v.astype(np.float64), hi + lo)   # the replay gives hi + lo exactly
        ehi, elo = T.encode32(v)
        assert np.array_equal(ehi, hi) and np.array_equal(elo, lo)                        # and the encode gives them back
        assert np.array_equal(np.round(2 * hi), 2 * hi) and set(np.round(lo / T.Q).tolist()) <= set(T.TABLE_B)
        # the condition: 0, a negative and a positive hi level, lo of both signs
        assert (0.0, 0) in tab and raw[(hi == 0)][0] == P.S1_MEAN[c] and (hi < 0).any() and (hi > 0).any()
        assert (lo < 0).any() and (lo > 0).any() and not lo[hi == 0].any()
        # the levels the frames draw from
        assert {b for b in (-1, 0, 1) if (-1.0, b) in tab} == {-1, 0, 1} and (2.0, 1) in tab
        fl = T.frame_levels(c)
        assert all(len(bs) >= 1 for bs in fl.values()) and any(b < 0 for b in fl[-1.0]) and any(b > 0 for b in fl[2.0])
    assert [len(t) for t in T.pixel_table()] == [24, 26, 29]  # (a deterministic search: recorded)


def test_frames_use_every_level_and_normalise_to_their_halves():
    for h, w in ALL_SHAPES:
        raw, vh, vl = T.frames(h, w)
        mh, ml = T.normalised_halves(h, w)  # asserts the replay's encode == (Vh, Vl)
        assert torch.equal(mh, vh) and torch.equal(ml, vl) and raw.dtype == torch.float32
        assert not torch.equal(raw[0], raw[1]) and not torch.equal(raw[1], raw[2]) and not torch.equal(raw[0], raw[2])
        if h * w >= 35:
            assert set(vh.unique().tolist()) == {-1.0, 0.0, 2.0} and set((vl / T.Q).unique().tolist()) == {-1.0, 0.0, 1.0}
    x2 = T.frames(9, 33, 1)[0]
    assert not torch.equal(x2, T.frames(9, 33)[0])  # a second base triple


def test_weights_use_every_position_and_encode_to_their_halves():
    for key in ("split", "wl0"):
        m = T.halves(key)  # asserts the scale and the encode model's (s Wh, s Wl)
        w, wh, wl, b = T.conv1_1_weights(key == "wl0")
        taps = (wh != 0).reshape(64, 27)
        print(f"\n conv1_1 [{key}]: scale {m['s1']:.0f}, taps per channel {sorted(set(taps.sum(1).tolist()))}, bias {sorted(set(b.tolist()))}, "
              f"positions used {int(taps.any(0).sum())} of 27, channels with a lo weight {int((wl != 0).reshape(64, -1).any(1).sum())}")
        assert set(taps.sum(1).tolist()) == {1, 2} and bool(taps.any(0).all())
        assert set(wh.unique().tolist()) == {-1.0, 0.0, 1.0} and bool((b == b.round()).all())
        assert set((wl / T.Q).unique().tolist()) == ({0.0} if key == "wl0" else {-1.0, 0.0, 1.0})
        assert bool(((wl != 0) <= (wh != 0)).all())
        if key == "split":
            assert bool(((wh * wl) < 0).any()) and bool(((wh * wl) > 0).any())  # a sign of its own
        for o in range(64):
            signs, bias = T.C11_TYPES[o % len(T.C11_TYPES)]
            assert sorted(wh[o][wh[o] != 0].tolist()) == sorted(signs) and float(b[o]) == bias
    w, wh, wl, b = T.conv1_2_weights()
    nz = (wh != 0).reshape(64, 576)
    assert int(nz.sum(1).max()) == T.C12_TERMS <= 400 and bool(nz.any(0).all()) and T.C12_TERMS * 9 * (1 + 8 * T.Q) + 3 < 2048
    assert set((wl / T.Q).unique().tolist()) == {-1.0, 0.0, 1.0} and set(b.tolist()) <= set(range(-3, 4)) and len(set(b.tolist())) > 3
    assert float(np.abs(w).max()) == 1.0 + T.Q
    for name, cs in (("split", T.convs("split")), ("wl0", T.convs("wl0")), ("copy", T.copy_convs())):
        assert len(cs) == 13 and cs[0][0].shape == (64, 3, 3, 3) and cs[1][0].shape == (64, 64, 3, 3), name


def test_every_tap_pattern_of_conv1_1_gives_zero_or_an_integer_from_2():
    """C11_TYPES over every combination of tap values in {-1, 0, 2}: the integer part is <= -1, 0 from a lone tap on a zero
    pixel (no lo term), or >= 2 -- and 2 only from one tap, whose lo terms stay below 4 q."""
    for signs, bias in T.C11_TYPES:
        for vals in np.ndindex(*(3,) * len(signs)):
            v = [(-1.0, 0.0, 2.0)[i] for i in vals]
            a = bias + sum(s * t for s, t in zip(signs, v))
            eps_max = sum((1.0 if t else 0.0) + abs(t) for t in v)  # |Wh vl| <= q, |Wl vh| <= |vh| q per tap
            assert a <= -1 or (a == 0 and eps_max == 0) or (a == 2 and eps_max < 4) or (a >= 3 and eps_max < 8), (signs, bias, v)


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=_ID)
def test_the_reference_is_exact_and_has_power(shape):
    h, w = shape
    a = T.analysis("split", h, w)  # asserts the quanta, the bounds and relu1_1's (A, eps)
    print(f"\n split {h}x{w}: conv1_1 sum |terms| + |bias| <= {a['bound1']:.4f}, conv1_2 <= {a['bound2']:.2f} < 2048; relu1_1 <= "
          f"{a['largest1']:.4f}, {a['live1']:.2f} of it live, {a['lo1']:.2f} with a lo half; largest |pre-activation| {a['largest']:.3f}, "
          f"{a['positive']:.2f} of them positive; {a['lolo1']:.2f} of conv1_1's outputs have a (dropped) lo*lo product")
    for mutant, share in a["mutants"].items():
        print(f"   {mutant}: {share:.4f} of the outputs differ")
        assert (share == 0.0) if mutant == SILENT else (share > 0.0), (mutant, share)
    assert 0.3 < a["positive"] < 0.7 and a["live1"] > 0.5 and (a["lo1"] > 0.3 or h * w == 1)
    assert T.tiled_replay_matches("split", h, w)
    ref = T.reference("split", h, w)
    assert ref.shape == (3, h, w, 64) and ref.dtype == torch.float32 and not bool(torch.signbit(ref).any())
    assert not torch.equal(ref[0], ref[1]) and not torch.equal(ref[1], ref[2])


@pytest.mark.parametrize("shape", T.SHAPES, ids=_ID)
def test_the_wl0_set_is_exact_and_has_no_lo_lo_product(shape):
    """What the two-kernel form (conv1_1 in float, then the implicit GEMM) is held to: with Wl = 0 a float product
    Wh (vh + vl) is the kernel's two terms, so the same reference binds both."""
    h, w = shape
    a = T.analysis("wl0", h, w)
    print(f"\n wl0 {h}x{w}: conv1_1 <= {a['bound1']:.4f}, conv1_2 <= {a['bound2']:.2f}; {a['lo1']:.2f} of relu1_1 with a lo half")
    assert a["lolo1"] == 0.0 and a["mutants"]["conv1_1: Wl*Ah dropped"] == 0.0
    for mutant in ("conv1_1: Wh*Al dropped", "relu1_1: lo = 0", "conv1_2: Wl*Ah dropped", "conv1_2: Wh*Al dropped"):
        assert a["mutants"][mutant] > 0.0, mutant
    rh, rl = T.relu1_1_reference("wl0", h, w)
    assert rh.shape == (3, h, w, 64) and rh.dtype == torch.float16 and bool((rl != 0).any())


def test_truncation_differs_where_there_is_something_to_round():
    v = torch.tensor([1.0 - T.Q, -(1.0 - T.Q), 1.0 + T.Q, 5 * T.Q, 0.0], dtype=torch.float64)
    assert T.truncated_half(v).tolist() == [1.0 - 4 * T.Q, -(1.0 - 4 * T.Q), 1.0, 5 * T.Q, 0.0]
    assert v.half().double().tolist() == [1.0, -1.0, 1.0, 5 * T.Q, 0.0]


@pytest.mark.parametrize("cus", P.CU_COUNTS)
def test_the_shapes_reach_their_regimes(cus):
    h, w = T.RING_SHAPE
    n = P.batch_for("conv1_regw_split", h, w, cus)
    r = P.regime("conv1_regw_split", n, h, w, cus)
    assert P.in_regime(r) and r["most"] >= 4 and r["least"] < r["most"] and r["dummy_halo"] and n % 3 == 0, r
    for sh, sw in T.SHAPES:
        r = P.regime("conv1_regw_split", 3, sh, sw, cus)
        # a block per tile wherever the tiles find as many CUs; the XCD-aware split deals an XCD's share of the tiles to
        # its share of the blocks, so a block may still own two (and another none)
        assert r["most"] <= (1 if r["total"] == 3 else 2) or cus < r["total"], r
