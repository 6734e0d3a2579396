"""conv2_2 + ReLU + L2-pool + statistics in one kernel (nqa_conv_pool.hip) against the unfused operators it replaces:
the same MFMA sequence produces the same tap values, so the pooled map may differ from l2pool(conv(.)) only by the
float summation order inside a 3x3 window (then at most one unit in the last place of the f16 result), and the five
sums from float64 sums of the unfused tap only by float32 accumulation error relative to the VARIANCE."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def blobs(dev):
    from nerf_qa_amd import ops, synth
    convs = synth.vgg16_weights(1234)
    return {p: ops.pack_vgg_weights(convs, p).to(dev) for p in ("f16", "f32m", "f16w")}


def _input(n, h, w, dev, seed, flat=False):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.rand(n, h, w, 128, device=dev, generator=g) * 1.5
    # sparse like a post-ReLU map, some channels nearly constant (their variance is what the shifted sums are for)
    x = torch.where(torch.rand(n, h, w, 128, device=dev, generator=g) < 0.4, torch.zeros_like(x), x)
    x[..., 5] = 2.0 + 1e-3 * torch.rand(n, h, w, device=dev, generator=g)
    x[..., 77] = 0.0
    if flat:
        x = x * 0 + 0.5
    return x.half().contiguous()


# (B, H, W): full tiles, ragged in either direction, one strip, tiny, many blocks per strip (warm-up starts), many pairs
SHAPES = [(1, 4, 16), (1, 8, 32), (2, 16, 48), (1, 5, 16), (1, 4, 17), (3, 13, 37), (1, 128, 128), (2, 64, 80),
          (5, 24, 32), (1, 540, 960), (1, 269, 477), (16, 32, 32)]


@pytest.mark.parametrize("b,h,w", SHAPES, ids=[f"{b}x{h}x{w}" for b, h, w in SHAPES])
@pytest.mark.parametrize("prec", ["f16", "f32m", "f16w"])
def test_fused_conv_pool_stats_against_the_unfused_operators(b, h, w, prec, dev, blobs):
    from nerf_qa_amd import ops
    inp = _input(2 * b, h, w, dev, seed=h * 1000 + w + b)
    kprec = "f16"
    pooled, sums = ops.conv_pool_stats(inp, 3, blobs[prec], prec)
    # the unfused pair: conv2_2 (same kernels' MFMA order; the mixed blobs' two-term layer through the same entry point)
    # then the L2-pool
    tap = ops.conv3x3_relu(inp, 3, blobs[prec], prec)
    ref_pool = ops.l2pool(tap, kprec)
    d = (pooled.float() - ref_pool.float()).abs()
    ulp = torch.maximum(ref_pool.float().abs(), torch.tensor(6.1e-5, device=dev)) * 2.0 ** -10
    assert (d <= ulp).all(), (b, h, w, float((d / ulp).max()))
    frac = float((d > 0).float().mean())
    assert frac < 2e-2, frac  # a different summation order flips the last bit of a few results, no more
    t = tap.double()
    tx, ty = t[:b], t[b:]
    want = torch.stack([tx.sum((1, 2)), ty.sum((1, 2)), (tx * tx).sum((1, 2)), (ty * ty).sum((1, 2)), (tx * ty).sum((1, 2))], -1)
    npx = h * w
    mx, my = want[..., 0] / npx, want[..., 1] / npx
    var_x, var_y = want[..., 2] / npx - mx * mx, want[..., 3] / npx - my * my
    got = sums
    gmx, gmy = got[..., 0] / npx, got[..., 1] / npx
    gvx, gvy = got[..., 2] / npx - gmx * gmx, got[..., 3] / npx - gmy * gmy
    gcov, cov = got[..., 4] / npx - gmx * gmy, want[..., 4] / npx - mx * my
    scale = torch.maximum(var_x + var_y, torch.tensor(1e-12, device=dev, dtype=torch.float64))
    assert ((gmx - mx).abs() <= 1e-6 * (mx.abs() + 1e-3)).all() and ((gmy - my).abs() <= 1e-6 * (my.abs() + 1e-3)).all()
    # variances / covariance to 1e-5 of the variance itself (the nearly constant channel 5 included)
    assert ((gvx - var_x).abs() <= 2e-5 * scale + 1e-12).all(), float(((gvx - var_x).abs() / scale).max())
    assert ((gvy - var_y).abs() <= 2e-5 * scale + 1e-12).all()
    assert ((gcov - cov).abs() <= 2e-5 * scale + 1e-12).all()
    assert torch.isfinite(pooled.float()).all() and torch.isfinite(sums).all()
    assert pooled.shape == (2 * b, (h + 1) // 2, (w + 1) // 2, 128)


@pytest.mark.parametrize("h,w,b", [(64, 96, 2), (97, 131, 2), (256, 256, 4), (270, 480, 2)])
@pytest.mark.parametrize("prec", ["f16", "f16w", "f32m"])
def test_dists_forward_fused_tap_equals_unfused(h, w, b, prec, dev):
    """The whole DISTS forward with the fused tap 2 against the same forward with nqa_set_conv_variant(+64) (the unfused
    tap): S1 / S2 of every channel and the scores agree to the float rounding of a different summation order."""
    from nerf_qa_amd import ops
    from nerf_qa_amd.DISTS_pytorch import DISTS
    m = DISTS(precision=prec, vgg16_path="synth:1234").to(dev).eval()
    g = torch.Generator(device=dev).manual_seed(h + w)
    x = torch.rand(b, 3, h, w, device=dev, generator=g)
    y = (x + 0.1 * torch.randn(x.shape, device=dev, generator=g)).clamp_(0, 1)
    try:
        with torch.no_grad():
            s1f, s2f = m._similarities(x, y)
            sf = m(x, y)
            ops.set_conv_variant(ops.DEFAULT_CONV_VARIANT + 64)
            s1u, s2u = m._similarities(x, y)
            su = m(x, y)
    finally:
        ops.set_conv_variant(ops.DEFAULT_CONV_VARIANT)
    e1, e2, es = (s1f - s1u).abs().max().item(), (s2f - s2u).abs().max().item(), (sf - su).abs().max().item()
    print(f"\n{h}x{w} B={b} {prec}: fused vs unfused max|dS1|={e1:.2e} max|dS2|={e2:.2e} max|dscore|={es:.2e}")
    # the score is the bar; single channels of the DEEPER taps may move more (a pooled value whose last f16 bit flipped
    # feeds three more stages, and a nearly dead channel's S2 is a quotient of two tiny moments: tests/test_gpu_fullsize_golden.py)
    # (f16 / f16w: a flipped last bit of a pooled half is the mode's own rounding noise, ~1e-5 on the score)
    assert es <= (2e-6 if prec == "f32m" else 2e-5), (es, e1, e2)
    # tap 2's own channels (67..194): the same rounded values summed in another order; taps 0 and 1 are untouched
    t1, t2 = (s1f[:, 67:195] - s1u[:, 67:195]).abs().max().item(), (s2f[:, 67:195] - s2u[:, 67:195]).abs().max().item()
    print(f"   tap 2 alone: max|dS1|={t1:.2e} max|dS2|={t2:.2e}")
    assert t1 <= 1e-5 and t2 <= 1e-3, (t1, t2)
    assert torch.equal(s1f[:, :67], s1u[:, :67]) and torch.equal(s2f[:, :67], s2u[:, :67])


# stage 1 from the raw frames (nqa_conv1_pool.hip).  (B, H, W): full units, ragged in either direction (a unit is 4 x 32),
# a second half-strip wholly outside the image (W = 48), one strip pair, many blocks per strip, many pairs
S1_SHAPES = [(1, 4, 32), (1, 8, 64), (2, 16, 48), (1, 5, 32), (1, 4, 33), (3, 13, 37), (1, 128, 128), (2, 64, 80),
             (5, 24, 32), (1, 1080, 1920), (1, 269, 477), (16, 32, 32), (1, 16, 16), (2, 20, 17)]


@pytest.mark.parametrize("b,h,w", S1_SHAPES, ids=[f"{b}x{h}x{w}" for b, h, w in S1_SHAPES])
def test_fused_stage1_pool_stats_against_the_unfused_operators(b, h, w, dev, blobs):
    """The fused kernel's tail waves take relu1_2 rounded to f16 -- the unfused kernels' values -- so the pooled map and
    the sums agree as tightly as tap 2's, but for the few pre-activations that sit within rounding of zero (below)."""
    rounded = True
    from nerf_qa_amd import ops
    g = torch.Generator(device=dev).manual_seed(h * 977 + w + b)
    x = torch.rand(b, 3, h, w, device=dev, generator=g)
    y = (0.5 * x + 0.5 * torch.rand(b, 3, h, w, device=dev, generator=g)).clamp_(0, 1)
    x[:, :, : h // 2, : w // 3] = 1.0  # a constant region: exactly dead / constant channels
    pooled, sums = ops.conv1_pool_stats(x, y, blobs["f16"], "f16")
    tap = ops.conv1_fused(torch.cat([x, y]), blobs["f16"], "f16")  # conv1_regw_kernel: relu1_2 as f16 NHWC
    ref_pool = ops.l2pool(tap, "f16")
    assert pooled.shape == ref_pool.shape == (2 * b, (h + 1) // 2, (w + 1) // 2, 64)
    d = (pooled.float() - ref_pool.float()).abs()
    ulp = torch.maximum(ref_pool.float().abs(), torch.tensor(6.1e-5, device=dev)) * 2.0 ** -10
    # The fused kernel starts its accumulators at the bias (the unfused one adds it behind the sum) and normalises the
    # pixels with a corrected reciprocal: a pre-activation within rounding of zero may land on the other side of the
    # ReLU, so a few pooled values in 10^4 differ by more than the last place -- everything else to one (two) units.
    over = d > (1.0 if rounded else 2.0) * ulp
    assert float(over.float().mean()) < 1e-3, (b, h, w, float(over.float().mean()))
    assert (d <= 0.1 * ref_pool.float().abs() + 2e-3).all(), (b, h, w, float(d.max()))
    if rounded:
        assert float((d > 0).float().mean()) < 2e-2
    t = tap.double()
    tx, ty = t[:b], t[b:]
    want = torch.stack([tx.sum((1, 2)), ty.sum((1, 2)), (tx * tx).sum((1, 2)), (ty * ty).sum((1, 2)), (tx * ty).sum((1, 2))], -1)
    npx = h * w
    m2 = torch.maximum((want[..., 2] + want[..., 3]) / npx, torch.tensor(1e-12, device=dev, dtype=torch.float64))

    def moments(s):
        mx, my = s[..., 0] / npx, s[..., 1] / npx
        return mx, my, s[..., 2] / npx - mx * mx, s[..., 3] / npx - my * my, s[..., 4] / npx - mx * my
    wm, gm = moments(want), moments(sums)
    scale = torch.maximum(wm[2] + wm[3], torch.tensor(1e-12, device=dev, dtype=torch.float64))
    for k in range(5):
        err = (gm[k] - wm[k]).abs()
        if rounded:
            # (a lane's float32 sums run over up to ~2 000 samples of a 1080p run before they are folded in float64:
            # eps * sqrt(n) of drift on the shifted first moment, i.e. a few 1e-6 of the mean, far inside what S1 / S2 see)
            tol = 3e-5 * wm[k].abs() + 1e-6 if k < 2 else 1e-4 * scale + 1e-9  # (floors: a ReLU flip in a nearly dead channel)
        else:  # the tap's f16 rounding: 2^-11 per value, averaging down with the pixel count; bounded loosely
            tol = 1e-3 * (wm[k].abs() + 1e-3) if k < 2 else 2e-3 * m2 + 1e-12
        assert (err <= tol).all(), (k, float((err / tol).max()))
    assert torch.isfinite(sums).all()


@pytest.mark.parametrize("h,w,b", [(64, 96, 2), (97, 131, 2), (256, 256, 4), (270, 480, 2), (540, 960, 1)])
def test_dists_forward_fused_stage1_equals_unfused(h, w, b, dev):
    """DISTS f16 forward with stage 1 fused (shipped) against the forward with both fused taps off: scores to the f16
    mode's own rounding noise; with the rounded-tap form of the fused stage 1 as tightly as tap 2's test."""
    from nerf_qa_amd import ops
    from nerf_qa_amd.DISTS_pytorch import DISTS
    m = DISTS(precision="f16", vgg16_path="synth:1234").to(dev).eval()
    g = torch.Generator(device=dev).manual_seed(h + w)
    x = torch.rand(b, 3, h, w, device=dev, generator=g)
    y = (x + 0.1 * torch.randn(x.shape, device=dev, generator=g)).clamp_(0, 1)
    out = {}
    try:
        with torch.no_grad():
            for name, v in (("fused", 0), ("unfused", 64 + 128)):
                ops.set_conv_variant(ops.DEFAULT_CONV_VARIANT + v)
                out[name] = (m(x, y), *m._similarities(x, y))
    finally:
        ops.set_conv_variant(ops.DEFAULT_CONV_VARIANT)
    for name in ("fused",):
        es = (out[name][0] - out["unfused"][0]).abs().max().item()
        t1 = (out[name][1][:, 3:67] - out["unfused"][1][:, 3:67]).abs().max().item()
        t2 = (out[name][2][:, 3:67] - out["unfused"][2][:, 3:67]).abs().max().item()
        print(f"\n{h}x{w} B={b} {name} vs unfused: max|dscore|={es:.2e}; tap 1 alone max|dS1|={t1:.2e} max|dS2|={t2:.2e}")
        assert es <= 2e-5, (name, es)
        assert t1 <= 1e-5 and t2 <= 1e-3, (name, t1, t2)
    assert torch.equal(out["fused"][1][:, :3], out["unfused"][1][:, :3])  # tap 0 (the raw image) is untouched


def _nan_filled_like(t):
    """A tensor of t's shape and type whose every byte is 0xFF (NaN in half, float, split16 records and float64): passed as
    out= / pooled= / sums=, a store the kernel skipped shows instead of hiding behind an allocator block that still holds
    the previous, correct result."""
    out = torch.empty_like(t)
    out.view(torch.uint8).fill_(0xFF)
    return out


@pytest.mark.parametrize("n,h,w", [(2, 97, 131), (4, 49, 66), (3, 42, 33)], ids=["2x97x131", "4x49x66", "3x42x33"])
def test_repeated_launches_are_bit_equal_on_ragged_maps(n, h, w, dev, blobs):
    """The persistent LDS-DMA kernels of round 4 (conv2_1 in f32s with register weights, the two fused conv + pool +
    statistics kernels) launched ten times on ragged maps whose blocks own one or two tiles each: bit-equal outputs.  (How a
    DMA lane that addressed LDS behind its slot showed itself: single wrong pixels in about every second launch.)  Every
    repeated launch writes into NaN-filled outputs of the caller's."""
    from nerf_qa_amd import ops, synth
    g = torch.Generator(device=dev).manual_seed(n * 1000 + h)
    # conv2_1, f32s: split16 in, split16 out
    packed32 = ops.pack_vgg_weights(synth.vgg16_weights(1234), "f32s").to(dev)
    a = ops.split16_encode((torch.rand(n, h, w, 64, device=dev, generator=g) * 4 - 1).clamp_min(0))
    first = ops.conv3x3_relu(a, 2, packed32, "f32s").clone()
    assert not torch.isnan(first.view(torch.float16)).any()
    for _ in range(10):
        again = ops.conv3x3_relu(a, 2, packed32, "f32s", out=_nan_filled_like(first))
        assert torch.equal(first.view(torch.int32), again.view(torch.int32))
    # the fused stage 1 and the fused conv2_2 (f16)
    x = torch.rand(n, 3, 2 * h, 2 * w, device=dev, generator=g)
    y = (0.5 * x + 0.5 * torch.rand(x.shape, device=dev, generator=g)).clamp_(0, 1)
    p1, s1 = ops.conv1_pool_stats(x, y, blobs["f16"], "f16")
    t = (torch.rand(2 * n, h, w, 128, device=dev, generator=g) * 2 - 0.5).clamp_min(0).half()
    p2, s2 = ops.conv_pool_stats(t, 3, blobs["f16"], "f16")
    p1, s1, p2, s2 = p1.clone(), s1.clone(), p2.clone(), s2.clone()
    assert not any(bool(torch.isnan(v).any()) for v in (p1, s1, p2, s2))
    for _ in range(10):
        q1, r1 = ops.conv1_pool_stats(x, y, blobs["f16"], "f16", pooled=_nan_filled_like(p1), sums=_nan_filled_like(s1))
        q2, r2 = ops.conv_pool_stats(t, 3, blobs["f16"], "f16", pooled=_nan_filled_like(p2), sums=_nan_filled_like(s2))
        assert torch.equal(p1, q1) and torch.equal(s1, r1) and torch.equal(p2, q2) and torch.equal(s2, r2)


# ---- y = x: a map scored against itself ---------------------------------------------------------------------------------------
def _assert_y_equals_x(pooled, sums, b, what):
    """pooled (2b, ho, wo, C) halves, sums (b, C, 5) float64 of a launch whose y images ARE its x images: no tolerance."""
    assert not bool(torch.isnan(pooled).any()) and not bool(torch.isnan(sums).any()), f"{what}: the NaN fill is still there"
    for lhs, rhs, name in ((0, 1, "sum x != sum y"), (2, 3, "sum x^2 != sum y^2"), (2, 4, "sum x^2 != sum xy")):
        unlike = (sums[..., lhs] != sums[..., rhs]).nonzero().cpu()
        print(f"   {name}: {unlike.shape[0]} of {sums.shape[0] * sums.shape[1]} (pair, channel)")
        if unlike.shape[0]:
            p, c = unlike[0].tolist()
            raise AssertionError(f"{what}: {name} in {unlike.shape[0]} (pair, channel), first {unlike[:6].tolist()}: "
                                 f"{sums[p, c, lhs].item()!r} against {sums[p, c, rhs].item()!r}; channels hit "
                                 f"{sorted(set(unlike[:, 1].tolist()))[:16]}")
    assert torch.equal(sums[..., 0], sums[..., 1]) and torch.equal(sums[..., 2], sums[..., 3])
    assert torch.equal(sums[..., 2], sums[..., 4])
    assert torch.equal(pooled[:b].view(torch.int16), pooled[b:].view(torch.int16)), f"{what}: the y half of the pooled map differs"
    assert float(sums[..., 2].min()) >= 0.0 and float(sums[..., 2].max()) > 0.0


@pytest.mark.parametrize("h,w", [(36, 64), (37, 70)], ids=["36x64", "37x70"])
@pytest.mark.parametrize("prec", ["f16", "f16w", "f32m"])
def test_fused_conv_pool_stats_of_a_map_with_itself(h, w, prec, dev, blobs):
    """y = x through conv3x3_regw128_pool_kernel on realistic values (the nearly constant channel 5 included), both
    instances, a batch in which lane sums are flushed inside the loop and at the drain: sum x = sum y, sum x^2 = sum y^2 =
    sum xy and the two halves of the pooled map, bit for bit.  With y == x a lane's moments of x and y are the same
    numbers; flush_stats must then round sum xy as it rounds sum x^2 (the two cross terms summed first, as
    ShiftedMoments::raw does; added one after the other they gave sum x^2 != sum xy in 1 of 2 816 (pair, channel) at 36 x 64
    in f16).  There is NO x <-> y swap property here: the fused kernels pivot both images on the x
    image's first activation, so a swap changes the pivot and the float moments -- bit-equality under a swap is
    pool_stats_kernel's contract (separate pivots), not theirs."""
    import persistent_refs as P
    from nerf_qa_amd import ops
    cus, nct = torch.cuda.get_device_properties(dev).multi_processor_count, 1 if prec == "f16" else 2
    b = P.pool_strong_batch_for(h, w, cus, nct) or P.pool_batch_for(h, w, cus, nct)
    r = P.pool_regime(b, h, w, cus, nct)
    print(f"\n conv2_2 + pool + statistics [{prec}] y = x, RAGGED = {P.pool_is_ragged(h, w)}: {b} pairs of {h}x{w}, {r['units']} units "
          f"on {r['grid']} blocks, {r['least']}..{r['most']} steps per block, {r['cross']} runs cross an image pair")
    assert P.pool_in_regime(r) and r["cross"] >= 1, r
    t = _input(b, h, w, dev, seed=h * 1000 + w + b)
    pooled = _nan_filled_like(torch.empty(2 * b, (h + 1) // 2, (w + 1) // 2, 128, dtype=torch.float16, device=dev))
    sums = _nan_filled_like(torch.empty(b, 128, 5, dtype=torch.float64, device=dev))
    res = ops.conv_pool_stats(torch.cat([t, t]), 3, blobs[prec], prec, pooled=pooled, sums=sums)
    assert res[0] is pooled and res[1] is sums
    _assert_y_equals_x(pooled, sums, b, f"conv2_2 + pool + statistics [{prec}] {b} pairs of {h}x{w}, y = x")


@pytest.mark.parametrize("h,w", [(64, 96), (37, 70)], ids=["64x96", "37x70"])
def test_fused_stage1_pool_stats_of_a_frame_with_itself(h, w, dev, blobs):
    """The same property of conv1_pool_kernel (both instances) on random frames with a constant region; no swap property
    either, for the same reason."""
    import persistent_refs as P
    from nerf_qa_amd import ops
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    b = P.s1_batch_for(h, w, cus)
    r = P.s1_regime(b, h, w, cus)
    print(f"\n fused stage 1 y = x: {b} pairs of {h}x{w}, {r['units']} units on {r['grid']} blocks, {r['least']}..{r['most']} steps "
          f"per block, {r['cross']} runs cross an image pair")
    assert P.s1_in_regime(r) and r["cross"] >= 1, r
    g = torch.Generator(device=dev).manual_seed(h * 977 + w + b)
    x = torch.rand(b, 3, h, w, device=dev, generator=g)
    x[:, :, : h // 2, : w // 3] = 1.0  # a constant region: exactly dead / constant channels
    pooled = _nan_filled_like(torch.empty(2 * b, (h + 1) // 2, (w + 1) // 2, 64, dtype=torch.float16, device=dev))
    sums = _nan_filled_like(torch.empty(b, 64, 5, dtype=torch.float64, device=dev))
    res = ops.conv1_pool_stats(x, x.clone(), blobs["f16"], "f16", pooled=pooled, sums=sums)
    assert res[0] is pooled and res[1] is sums
    _assert_y_equals_x(pooled, sums, b, f"fused stage 1, {b} pairs of {h}x{w}, y = x")
