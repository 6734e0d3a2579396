"""The layers of the mixed modes (f16w / f32m4 / f32m / f32m2) ONE AT A TIME, through the single-operator entry points:
f16 activations x two-term (hi, lo) f16 weights against a float64 convolution with the unrounded float32 weights.

Through a whole pyramid a layer that drops its `lo` term is off by 2-4e-4 of a map's maximum and passes every bar of the
pyramid and score tests; a chain of layers cannot be pinned tighter either, because f16 rounding flips cascade.  One
layer has no cascade, so it is held to an exact envelope here.  All references are computed once on the CPU
(tests/mixed_refs.py) and every reference figure below is recomputed without a GPU by tests/test_mixed_refs.py.  The
float32 replays run through torch's CPU convolution, whose summation order depends on the CPU, so the figures hold to
some ten per cent; the fixtures take the bars from what the replay measures when the tests run.

(a) two-term layers.  pre = conv2d(a, w, b) and mag = conv2d(|a|, |w|) + |b| in float64, tau = c 2^-24 mag; every output
    must lie in [f16(relu(pre - tau)), f16(relu(pre + tau))] (rounding to half is monotone: exact, no ulp arithmetic, no
    special case for tiny outputs of cancelling sums).
      reference figure: a float32 replay conv2d(a, hi) + conv2d(a, lo) + b, hi = f16(w), lo = f16(w - hi), is within
        2.22 ... 5.34 x 2^-24 mag of pre over CONV_CASES and EXTRA_CASES, and 6.11 on BIG_CASE (conv3_2, 48 x 13 x 33)
      bar: c = 3 x the largest = 16.0 for CONV_CASES and EXTRA_CASES; BIG_CASE, added for the tile variants, gets its own
        c = 3 x 6.11 = 18.3 and widens no other case (the margin is the MFMA's other summation order over K = 9 Cin); the
        fixture recomputes both.  A replay without lo is at 570 ... 1840, one that loses lo in one tap of nine at 230 ... 980.
    and the share of outputs that differ at all from f16(relu(pre)) is capped:
      reference figure: the float32 replay differs in <= 3.9e-3 of the elements (1.8e-3 with the scaled terms)
      bar: 1e-2.  One lo tap lost of nine: >= 7.5e-2; no lo: >= 2.0e-1.
    Kernels by nqa_set_conv_variant in a mixed mode (nqa_conv.hip, launch_conv<.., NTERM = 2>):
      1 (default) conv1_2, conv2_1: conv3x3_regw_kernel<.., 2>; conv2_2, conv3_1: conv3x3_regw128_kernel<.., 2> (W >= 16);
                  everything else the implicit GEMM <.., NTERM = 2> in its 64-channel, 4-wave or 8-wave tile, 16 or 32 wide
      0           the 4-wave tile where 1 takes the 8-wave one: >= 256 output channels, W > 16 and >= 192 blocks of it
                  (BIG_CASE; on every smaller map 0 and 1 launch the same kernel)
      +16         the implicit GEMM for layers 1..4 (and stage 1 unfused)
      +32         the implicit GEMM for conv2_2 / conv3_1
    without effect on a two-term layer: 2 (the 128 x 512 tile is chosen behind the two-term dispatch: same as 1), +4 (tile
    form of the ONE-term fused stage 1), +8 (A-DISTS window pass), +64 / +128 (fusions of the DISTS path, not of an operator).
(b) float stages of a mixed blob (layers 4 | 7 | 10 behind the boundary of f32m2 | f32m | f32m4, and layer 12):
    nqa_pack_vgg_weights writes their rows by the same code as for f32s and conv3x3 launches the same
    launch_conv<PrecF32S, 1> instance with the same tile choice, so the result is BIT-EQUAL to the f32s blob's.
(c) the boundary pool f16 -> split16 against dists_oracle.l2pool in float64 of the same half values, float-class:
      reference figure: the float32 oracle is 1.24e-7 | 6.2e-8 | 8.4e-8 | 1.05e-7 of the map's maximum from the float64 one
      bar: 4 x that, per shape (a split16 emulation of the float32 oracle sits at 1.1 ... 2.0e-7).
    Channels at 0 and at 2^-15 pool to 1e-6 and ~3e-5, below 2^-14: split16 does not lose them, it keeps them as a
    subnormal half hi with lo = 0, i.e. to an ABSOLUTE 2^-25 (measured 1.3e-8 and 2.2e-8), which is what is asserted.
(d) stage 1.  The mixed conv1_1 is an exact float conv with a half store: the envelope of (a) with
      reference figure: float32 replay (normalisation and conv in float32) within 2.50 ... 4.27 x 2^-24 mag; bar c = 3 x 4.27 = 12.8
    then conv1_2 on that output under (a).  The fused stage 1 (conv1_regw_kernel<PrecF16, 2>) rounds the NORMALISED
    pixels to half, starts conv1_1 at bias x scale, descales, applies the ReLU and rounds relu1_1 to half; relu1_1 is not
    observable and its flips cascade, so it is compared relative to the map's maximum against a float64 replay with
    those rounding points:
      reference figure: the float32 replay with the same rounding points is 2.63e-4 | 2.20e-4 | 4.30e-4 | 4.01e-4 of the
        maximum from the float64 one on the four shapes (the half store of the outputs near the maximum)
      bar: 4 x that, per shape.  This bar alone cannot see a lost lo term (3.0 ... 5.6e-4 of the maximum: inside it), so
    the share of outputs that differ at all from f16(relu1_2 of the float64 replay) is capped beside it:
      reference figure: the float32 replay differs in 5.98e-3 | 3.00e-3 | 6.46e-3 | 5.55e-3 of the elements
      bar: 4 x that, per shape (the factor of the bar above).  A replay that loses lo in conv1_1, in conv1_2 or in both
        differs in 2.1e-1 ... 2.8e-1.
(e) nqa_vgg_pyramid's five taps rebuilt op by op through these entry points are BIT-EQUAL in all four mixed modes (the
    operators see the same batch, so every kernel gets the same grid)."""
import pytest
import torch

import mixed_refs as R

pytestmark = pytest.mark.gpu

MIXED = ("f16w", "f32m4", "f32m", "f32m2")
LAST_16BIT_LAYER = {"f32m4": 9, "f32m": 6, "f32m2": 3}
SHARE_CAP = 1e-2
EXTRA_CASES = [(4, 2, 9, 33)]  # conv3_1 on the register-weights kernel (the issue's only conv3_1 map is below 16 wide)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def blobs(np_convs, dev):
    from nerf_qa_amd import ops
    return {p: ops.pack_vgg_weights(np_convs, p).to(dev) for p in MIXED + ("f32s",)}


@pytest.fixture(scope="module")
def conv_refs():
    """({case: (input, pre, mag, c)}, c): the envelope constant c = 3 x the float32 replay's largest distance over
    CONV_CASES and EXTRA_CASES; BIG_CASE carries 3 x its own figure.  Computed once."""
    refs, own, share = {}, {}, 0.0
    for case in R.CONV_CASES + EXTRA_CASES + [R.BIG_CASE]:
        a = R.relu_like_input(*case)
        pre, mag, acc = R.conv_layer_ref(a, *R.convs()[case[0]])
        own[case] = R.replay_constant(pre, mag, acc)
        share = max(share, R.share_differing(R.to_half(acc.clamp_min(0)), pre))
        refs[case] = (a, pre, mag)
    worst = max(v for case, v in own.items() if case != R.BIG_CASE)
    print(f"\nfloat32 replay of the two-term layers: max |acc - pre| = {worst:.2f} x 2^-24 mag -> c = {3 * worst:.1f} "
          f"({own[R.BIG_CASE]:.2f} -> {3 * own[R.BIG_CASE]:.1f} on {R.BIG_CASE}); share differing from f16(relu(pre)) <= "
          f"{share:.1e} (cap {SHARE_CAP:.0e})")
    assert share < SHARE_CAP  # (the reference itself meets the cap)
    refs = {case: (*v, 3.0 * (own[case] if case == R.BIG_CASE else worst)) for case, v in refs.items()}
    return refs, 3.0 * worst


def _check_two_term(got_nhwc, pre, mag, c, what):
    got = got_nhwc.permute(0, 3, 1, 2).double().cpu()
    lo, hi = R.half_envelope(pre, mag, c)
    out = (got < lo) | (got > hi)
    share = R.share_differing(got, pre)
    worst = float(((got - pre.clamp_min(0)).abs() / (R.EPS24 * mag)).max())  # (includes the store's own rounding)
    print(f"\n{what}: outside the envelope {int(out.sum())} of {out.numel()}; share differing from f16(relu(pre)) {share:.2e}; "
          f"max |got - relu(pre)| = {worst:.0f} x 2^-24 mag")
    if out.any():
        n, ch, y, x = (t.tolist()[:8] for t in out.nonzero(as_tuple=True))
        raise AssertionError(f"{what}: {int(out.sum())} outputs outside [f16(relu(pre - tau)), f16(relu(pre + tau))], c = {c:.1f}; "
                             f"first at image {n} channel {ch} row {y} column {x}; channels hit: "
                             f"{sorted(set(out.nonzero()[:, 1].tolist()))[:32]}")
    assert share <= SHARE_CAP, f"{what}: {share:.2e} of the outputs differ from f16(relu(pre))"


def _two_term_params():
    ps = []
    for case in R.CONV_CASES + EXTRA_CASES:
        layer, _, _, w = case
        modes = ["f16w"] + [m for m, last in LAST_16BIT_LAYER.items() if last == layer]
        for m in modes:
            ps.append((m, 1, case))
        if layer <= 4 and w >= 16:  # the register-weights kernels' layers: +16 moves them to the implicit GEMM
            ps.append(("f16w", 1 + 16, case))
        if layer in (3, 4) and w >= 16:
            ps.append(("f16w", 1 + 32, case))
    ps += [("f16w", 0, R.BIG_CASE), ("f16w", 1, R.BIG_CASE)]
    return ps


@pytest.mark.parametrize("prec,variant,case", _two_term_params(),
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_two_term_layer_in_its_float64_envelope(prec, variant, case, conv_refs, blobs, dev):
    from nerf_qa_amd import ops
    a, pre, mag, c = conv_refs[0][case]
    ops.set_conv_variant(variant)
    try:
        out = ops.conv3x3_relu(a.to(dev), case[0], blobs[prec], prec)
    finally:
        ops.set_conv_variant(ops.DEFAULT_CONV_VARIANT)
    assert out.dtype == torch.float16 and out.shape == (*a.shape[:3], ops.CONV_COUT[case[0]])
    _check_two_term(out, pre, mag, c, f"conv layer {case[0]} [{prec}, variant {variant}] {case[1:]}")


# ---- (b) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,layer,n,h,w", [("f32m2", 4, 1, 7, 7), ("f32m2", 4, 2, 9, 33), ("f32m", 7, 1, 6, 18),
                                              ("f32m4", 10, 1, 5, 6), ("f32m2", 12, 3, 4, 16), ("f32m", 12, 3, 4, 16),
                                              ("f32m4", 12, 1, 1, 1)])
def test_float_stage_of_a_mixed_blob_is_bit_equal_to_f32s(prec, layer, n, h, w, blobs, dev):
    from nerf_qa_amd import ops
    a = R.uniform((n, h, w, ops.CONV_CIN[layer]), 100 + layer, -2.0, 2.0).clamp_min(0)
    inp = ops.split16_encode(a.to(dev))
    want = ops.conv3x3_relu(inp, layer, blobs["f32s"], "f32s")
    got = ops.conv3x3_relu(inp, layer, blobs[prec], prec)
    assert got.dtype == torch.float32 and torch.isfinite(ops.split16_decode(got) if layer not in ops.TAP_LAYERS else got).all()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


# ---- (c) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w,c", R.POOL_SHAPES, ids=lambda v: str(v))
def test_boundary_pool_is_float_class(n, h, w, c, dev):
    from nerf_qa_amd import ops
    a = R.pool_input(n, h, w, c)
    p64, p32 = R.pool_refs(a)
    own = R.rel_to_max(p32, p64)
    out = ops.l2pool_f16_to_split16(a.to(dev))
    assert out.dtype == torch.float32 and out.shape == (n, (h + 1) // 2, (w + 1) // 2, c)
    got = ops.split16_decode(out).permute(0, 3, 1, 2).double().cpu()
    err = R.rel_to_max(got, p64)
    print(f"\nboundary pool {(n, h, w, c)}: {err:.2e} of the maximum from float64 (float32 oracle: {own:.2e}, bar {4 * own:.2e})")
    assert err <= 4 * own
    # below 2^-14: kept as a subnormal half `hi` (quantum 2^-24) with lo = 0 -- to an absolute 2^-25, not flushed to zero
    for ch in (3, 5):
        assert float(p64[:, ch].max()) < 2.0 ** -14
        d = float((got[:, ch] - p64[:, ch]).abs().max())
        print(f"   channel {ch}: pooled {float(p64[:, ch].max()):.3e}, |error| {d:.2e} (2^-25 = {2.0 ** -25:.2e})")
        assert d <= 2.0 ** -25 * (1 + 1e-3) and (got[:, ch] > 0).all()


# ---- (d) ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def conv1_1_c():
    worst = max(R.replay_constant(*R.conv1_1_ref(R.image(s))) for s in R.STAGE1_SHAPES)
    print(f"\nfloat32 replay of conv1_1: max |acc - pre| = {worst:.2f} x 2^-24 mag -> c = {3 * worst:.1f}")
    return 3.0 * worst


@pytest.mark.parametrize("shape", R.STAGE1_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("prec", MIXED)
def test_mixed_conv1_1_and_conv1_2_on_its_output(prec, shape, conv1_1_c, conv_refs, blobs, dev):
    from nerf_qa_amd import ops
    x = R.image(shape)
    pre, mag, _ = R.conv1_1_ref(x)
    r11 = ops.conv1_1(x.to(dev), blobs[prec], prec)
    assert r11.dtype == torch.float16 and r11.shape == (shape[0], shape[2], shape[3], 64)
    got = r11.permute(0, 3, 1, 2).double().cpu()
    lo, hi = R.half_envelope(pre, mag, conv1_1_c)
    out = (got < lo) | (got > hi)
    print(f"\nconv1_1 [{prec}] {shape}: outside the envelope {int(out.sum())}; share differing {R.share_differing(got, pre):.2e}")
    assert not out.any(), (int(out.sum()), out.nonzero()[:8].tolist())
    assert R.share_differing(got, pre) <= SHARE_CAP
    # conv1_2 on exactly these half values, as a two-term layer of its own
    a = r11.cpu()
    pre2, mag2, _ = R.conv_layer_ref(a, *R.convs()[1])
    r12 = ops.conv3x3_relu(r11, 1, blobs[prec], prec)
    _check_two_term(r12, pre2, mag2, conv_refs[1], f"conv1_2 on conv1_1's output [{prec}] {shape}")


@pytest.fixture(scope="module")
def fused_refs():
    """{shape: (image, float64 replay, the float32 replay's distance from it, the float32 replay's share of differing
    halves)}, once for all modes."""
    refs = {}
    for shape in R.FUSED_SHAPES:
        x = R.image(shape, 21)
        r64, r32 = R.fused_stage1_ref(x, torch.float64), R.to_half(R.fused_stage1_ref(x, torch.float32))
        refs[shape] = (x, r64, R.rel_to_max(r32, r64), R.share_of_halves_differing(r32, r64))
    return refs


@pytest.mark.parametrize("shape", R.FUSED_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("prec", MIXED)
def test_mixed_fused_stage1_against_its_float64_replay(prec, shape, fused_refs, blobs, dev):
    from nerf_qa_amd import ops
    x, r64, own, own_share = fused_refs[shape]
    out = ops.conv1_fused(x.to(dev), blobs[prec], prec)
    assert out.dtype == torch.float16 and out.shape == (shape[0], shape[2], shape[3], 64)
    got = out.permute(0, 3, 1, 2).cpu()
    err, share = R.rel_to_max(got, r64), R.share_of_halves_differing(got, r64)
    print(f"\nfused stage 1 [{prec}] {shape}: {err:.2e} of the maximum from the float64 replay (float32 replay: {own:.2e}, "
          f"bar {4 * own:.2e}); {share:.2e} of the outputs differ from its halves (float32 replay: {own_share:.2e}, "
          f"cap {4 * own_share:.2e})")
    assert err <= 4 * own
    assert share <= 4 * own_share  # (a lost lo term in either convolution: >= 2.1e-1)


@pytest.mark.parametrize("prec", MIXED)
def test_mixed_fused_stage1_refuses_what_the_pyramid_does_not_fuse(prec, blobs, dev):
    from nerf_qa_amd import NqaError, ops
    with pytest.raises(NqaError, match=r"error -2: .*W >= 16"):  # NQA_E_SHAPE
        ops.conv1_fused(torch.zeros(1, 3, 16, 15, device=dev), blobs[prec], prec)
    ops.set_conv_variant(ops.DEFAULT_CONV_VARIANT + 16)
    try:
        with pytest.raises(NqaError, match="error -2"):  # the first-forms bit: the pyramid runs stage 1 as two kernels
            ops.conv1_fused(torch.zeros(1, 3, 16, 16, device=dev), blobs[prec], prec)
    finally:
        ops.set_conv_variant(ops.DEFAULT_CONV_VARIANT)


# ---- (e) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(45, 70), (9, 13)], ids=["45x70_fused_stage1", "9x13_two_kernel_stage1"])
@pytest.mark.parametrize("prec", MIXED)
def test_pyramid_taps_are_these_operators(prec, h, w, blobs, dev):
    """The mixed-mode twin of test_gpu_ops.py::test_pool_stats_matches_separate_kernels."""
    from nerf_qa_amd import _lib, ops, synth
    x, _ = synth.frame_batch([3], h, w)
    x = torch.from_numpy(x).to(dev)
    p = _lib.prec_id(prec)
    taps = ops.vgg_pyramid(x, blobs[prec], prec)
    if w >= 16:
        t = ops.conv1_fused(x, blobs[prec], prec)
    else:
        t = ops.conv3x3_relu(ops.conv1_1(x, blobs[prec], prec), 1, blobs[prec], prec)
    layer = 2
    for k in range(5):
        assert t.dtype == taps[k].dtype and torch.equal(t.view(torch.int16 if t.dtype == torch.float16 else torch.int32),
                                                        taps[k].view(torch.int16 if t.dtype == torch.float16 else torch.int32)), \
            f"tap {k + 1} differs"
        if k == 4:
            break
        here, behind = _lib.stage_prec(p, k), _lib.stage_prec(p, k + 1)
        if here == _lib.PREC_F16 and behind == _lib.PREC_F32S:
            t = ops.l2pool_f16_to_split16(t)
        elif here == _lib.PREC_F16:
            t = ops.l2pool(t, prec)
        else:
            t = ops.l2pool(t, "f32s")  # float tap in, split16 out: the f32s pool, as run_stages calls it
        for _ in range((2, 2, 3, 3, 3)[k + 1]):
            t = ops.conv3x3_relu(t, layer, blobs[prec], prec)
            layer += 1
