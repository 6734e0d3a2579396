"""DISTS.forward(x, y, require_grad=True): image gradients through the HIP pyramid (nerf_qa_amd/autograd.py,
csrc/nqa_backward.hip) against torch autograd over the CPU oracle -- which is what the reference does
(DISTS_pt.py:105-108 runs forward_once with autograd).  Each backward kernel is also checked on its own."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _oracle_score(x, y, convs, alpha, beta):
    from oracle import dists_oracle as do
    f0, f1 = do.vgg_pyramid(x, convs), do.vgg_pyramid(y, convs)
    s1, s2 = do.dists_stats(f0, f1)
    return do.dists_score(s1, s2, alpha, beta)


@pytest.mark.parametrize("cin,cout,h,w", [(64, 64, 9, 21), (128, 64, 12, 33), (256, 128, 7, 16), (512, 512, 5, 9)])
def test_conv3x3_split_generic_is_a_float_conv(cin, cout, h, w, dev):
    from nerf_qa_amd import ops
    g = torch.Generator().manual_seed(cin + cout)
    wgt = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
    a = torch.randn(2, h, w, cin, generator=g)  # signed input, no ReLU anywhere
    want = F.conv2d(a.permute(0, 3, 1, 2).double(), wgt.double(), padding=1).permute(0, 2, 3, 1).float()
    blob = ops.pack_conv_split(wgt).to(dev)
    got = ops.conv3x3_split(ops.split16_encode(a.to(dev)), blob, cout, relu=False).cpu()
    err = (got - want).abs().max().item() / want.abs().max().item()
    assert got.min().item() < 0 and err < 2e-6, err
    got_r = ops.conv3x3_split(ops.split16_encode(a.to(dev)), blob, cout, relu=True).cpu()
    assert torch.equal(got_r, got.clamp_min(0))


def test_relu_mask_l2pool_and_conv1_1_backward_kernels(dev):
    from nerf_qa_amd import ops
    from oracle import dists_oracle as do
    g = torch.Generator().manual_seed(7)
    # relu mask: float and split16 activations
    act = torch.randn(2, 5, 9, 64, generator=g).clamp_min(0)
    gr = torch.randn(2, 5, 9, 64, generator=g)
    want = gr * (act > 0)
    for split in (False, True):
        a_dev = ops.split16_encode(act.to(dev)) if split else act.to(dev)
        got = ops.split16_decode(ops.relu_mask_split16(gr.to(dev), a_dev, split)).cpu()
        assert (got - want).abs().max().item() <= 2e-6 * gr.abs().max().item()
    # L2-pool gradient vs autograd of the oracle's pool, odd sizes (ragged last row / column)
    for (n, h, w, c) in ((2, 9, 13, 64), (1, 8, 6, 128), (1, 1, 1, 64), (1, 2, 3, 64)):
        x = (torch.rand(n, c, h, w, generator=g) + 0.05).requires_grad_()
        yp = do.l2pool(x)
        gy = torch.randn(yp.shape, generator=g)
        (yp * gy).sum().backward()
        tap = x.detach().permute(0, 2, 3, 1).contiguous().to(dev)
        pooled = ops.l2pool(tap, "f32s")  # split16, as the forward leaves it
        gt = torch.zeros_like(tap)
        ops.l2pool_backward(tap, pooled, gy.permute(0, 2, 3, 1).contiguous().to(dev), gt)
        err = (gt.cpu().permute(0, 3, 1, 2) - x.grad).abs().max().item() / x.grad.abs().max().item()
        assert err < 1e-5, ((n, h, w, c), err)
    # conv1_1 gradient (normalisation included) vs autograd
    w0 = torch.randn(64, 3, 3, 3, generator=g) * 0.2
    img = torch.rand(2, 3, 7, 10, generator=g).requires_grad_()
    mean = torch.tensor(do.IMAGENET_MEAN).view(1, 3, 1, 1)
    std = torch.tensor(do.IMAGENET_STD).view(1, 3, 1, 1)
    out = F.conv2d((img - mean) / std, w0, padding=1)
    gm = torch.randn(out.shape, generator=g)
    (out * gm).sum().backward()
    got = ops.conv1_1_backward(gm.permute(0, 2, 3, 1).contiguous().to(dev), w0.to(dev)).cpu()
    assert (got - img.grad).abs().max().item() / img.grad.abs().max().item() < 1e-5


BACKWARD_SHAPES = [(64, 64), (128, 64), (128, 128), (256, 128), (256, 256), (512, 256), (512, 512)]  # (cin, cout) of the data-gradient layers


def _split_conv_case(cin, cout, n, h, w, dev):
    """Signed inputs whose magnitudes span 1e-4 .. 256 (what normalise() hands the convolution, and everything below
    it), against a float64 convolution: the existing 2e-6 of the largest output."""
    from nerf_qa_amd import ops
    g = torch.Generator().manual_seed(cin * 7 + cout + h * 1000 + w)
    wgt = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
    mag = 10.0 ** (torch.rand(n, h, w, cin, generator=g) * (np.log10(256.0) + 4.0) - 4.0)
    a = mag * (torch.randint(0, 2, mag.shape, generator=g) * 2 - 1)
    assert a.abs().min().item() < 1e-3 and a.abs().max().item() > 100 and a.min().item() < 0 < a.max().item()
    want = F.conv2d(a.permute(0, 3, 1, 2).double(), wgt.double(), padding=1).permute(0, 2, 3, 1)
    got = ops.conv3x3_split(ops.split16_encode(a.to(dev)), ops.pack_conv_split(wgt).to(dev), cout, relu=False).cpu()
    err = (got.double() - want).abs().max().item() / want.abs().max().item()
    print(f"\nconv3x3_split {cin} -> {cout} n={n} {h}x{w}: max err / max {err:.2e}")
    assert torch.isfinite(got).all() and got.min().item() < 0 and err < 2e-6, ((cin, cout, n, h, w), err)


@pytest.mark.parametrize("cin,cout", BACKWARD_SHAPES)
@pytest.mark.parametrize("h,w", [(1, 1), (2, 2), (3, 200)])
def test_conv3x3_split_generic_every_backward_shape_at_the_smallest_maps(cin, cout, h, w, dev):
    """Measured on an MI355X: 1e-7 .. 1.1e-6 (512 -> 256 at 3x200 the largest).  With the three split products of a k-step
    in ONE float accumulator that case stood at 2.02e-6 and missed the bound (torch's own float32 convolution: 2.82e-6 on
    the same inputs): the data-gradient convolutions now keep the two cross terms in an accumulator of their own."""
    _split_conv_case(cin, cout, 2, h, w, dev)


@pytest.mark.parametrize("cin,cout,n,h,w", [(128, 128, 2, 11, 19), (256, 256, 1, 9, 14), (512, 256, 2, 6, 21), (128, 64, 2, 128, 128)])
def test_conv3x3_split_generic_remaining_shapes_and_many_tiles(cin, cout, n, h, w, dev):
    _split_conv_case(cin, cout, n, h, w, dev)


@pytest.mark.parametrize("c", [64, 128, 256, 512])
def test_relu_mask_split16_on_subnormal_halves_and_zeros(c, dev):
    """The mask is (decoded split16 activation > 0), exactly: activations below the smallest normal half (2^-14 down to
    2^-24, where hi is a subnormal half and lo is gone), values that encode to zero altogether, and exact zeros."""
    from nerf_qa_amd import ops
    g = torch.Generator().manual_seed(c)
    shape = (2, 5, 9, c)
    act = torch.randn(shape, generator=g).clamp_min(0)
    pick = torch.randint(0, 16, shape, generator=g)
    for k in range(14, 28):  # 2^-14 .. 2^-24 are halves (subnormal below 2^-14); 2^-26 and below encode to zero
        act = torch.where(pick == k - 14, torch.full(shape, 2.0 ** -k) * (1 + torch.rand(shape, generator=g)), act)
    act = torch.where(pick == 14, torch.zeros(shape), act)
    gr = (1 + torch.rand(shape, generator=g)) * (torch.randint(0, 2, shape, generator=g) * 2 - 1)  # 1 <= |g| < 2: never zero
    a_dev = ops.split16_encode(act.to(dev))
    dec = ops.split16_decode(a_dev).cpu()
    assert (dec == 0).any() and ((dec > 0) & (dec < 2.0 ** -14)).any() and ((act > 0) & (dec == 0)).any()
    got = ops.split16_decode(ops.relu_mask_split16(gr.to(dev), a_dev, True)).cpu()
    assert torch.equal(got != 0, dec > 0)
    assert (got - gr * (dec > 0)).abs().max().item() <= 2e-6 * gr.abs().max().item()
    # a float (tapped) activation: the mask is act > 0 on the float itself, however small
    got_f = ops.split16_decode(ops.relu_mask_split16(gr.to(dev), act.to(dev), False)).cpu()
    assert torch.equal(got_f != 0, act > 0)


def _l2pool_backward_case(x, gy, dev):
    """x (n,c,h,w) float32, gy as the pooled map: (device gradient, float64 autograd of the oracle's pool), both NCHW."""
    from nerf_qa_amd import ops
    from oracle import dists_oracle as do
    xd = x.double().requires_grad_()
    (do.l2pool(xd) * gy.double()).sum().backward()
    tap = x.permute(0, 2, 3, 1).contiguous().to(dev)
    pooled = ops.l2pool(tap, "f32s")  # split16, as the forward leaves it
    gt = torch.zeros_like(tap)
    ops.l2pool_backward(tap, pooled, gy.permute(0, 2, 3, 1).contiguous().to(dev), gt)
    return gt.cpu().permute(0, 3, 1, 2), xd.grad


L2POOL_EDGES = ["zero_regions", "tiny_values", "one_pixel_per_window", "1xN", "Nx1", "C256", "C512"]


@pytest.mark.parametrize("edge", L2POOL_EDGES)
def test_l2pool_backward_edges(edge, dev):
    """Against float64 autograd of dists_oracle.l2pool, the existing 1e-5 of the largest gradient; g_pooled reaches 256,
    the largest value pyramid_backward's normalise() hands the kernel."""
    g = torch.Generator().manual_seed(L2POOL_EDGES.index(edge))
    n, c, h, w = {"1xN": (2, 64, 1, 13), "Nx1": (2, 64, 13, 1), "C256": (1, 256, 6, 7), "C512": (2, 512, 5, 4)}.get(edge, (2, 64, 13, 18))
    x = torch.rand(n, c, h, w, generator=g) + 0.05
    zero = torch.zeros_like(x, dtype=torch.bool)
    if edge == "zero_regions":  # all-zero blocks several pool windows wide: the pooled value there is the sqrt(1e-12) floor
        zero[:, :, 2:9, :] = True
        zero[:, :, :, 11:16] = True
        zero[:, 5] = True       # a dead channel
        x = x.masked_fill(zero, 0.0)
    elif edge == "tiny_values":  # 1e-4 .. 1e-3 throughout: the pooled value's lo half is a subnormal half
        x = 1e-4 + 9e-4 * torch.rand(n, c, h, w, generator=g)
    elif edge == "one_pixel_per_window":  # pixels four apart: no 3x3 window holds two of them
        keep = torch.zeros_like(x, dtype=torch.bool)
        keep[:, :, 1::4, 2::4] = True
        keep[:, 1::2] = keep[:, 1::2].roll((1, 1), (2, 3))  # odd channels: on even rows / odd columns instead
        zero = ~keep
        x = x.masked_fill(zero, 0.0)
    gy = torch.randn(n, c, (h + 1) // 2, (w + 1) // 2, generator=g)
    gy = gy * (256.0 / gy.abs().max())
    got, want = _l2pool_backward_case(x, gy, dev)
    assert torch.isfinite(got).all() and torch.isfinite(want).all()
    assert (got[zero] == 0).all() and (want[zero] == 0).all()  # exactly zero where the tap is zero
    err = (got.double() - want).abs().max().item() / want.abs().max().item()
    print(f"\nl2pool_backward {edge}: max|grad| {want.abs().max().item():.3e}  max err / max {err:.2e}")
    assert err < 1e-5, (edge, err)


@pytest.mark.parametrize("n,h,w", [(3, 1, 1), (3, 1, 9), (3, 9, 1), (3, 6, 5)])
def test_conv1_1_backward_smallest_maps(n, h, w, dev):
    from nerf_qa_amd import ops
    from oracle import dists_oracle as do
    g = torch.Generator().manual_seed(n * 100 + h * 10 + w)
    w0 = (torch.randn(64, 3, 3, 3, generator=g) * 0.2).double()
    img = torch.rand(n, 3, h, w, generator=g).double().requires_grad_()
    mean = torch.tensor(do.IMAGENET_MEAN, dtype=torch.float64).view(1, 3, 1, 1)
    std = torch.tensor(do.IMAGENET_STD, dtype=torch.float64).view(1, 3, 1, 1)
    out = F.conv2d((img - mean) / std, w0, padding=1)
    gm = torch.randn(out.shape, generator=g)
    (out * gm.double()).sum().backward()
    got = ops.conv1_1_backward(gm.permute(0, 2, 3, 1).contiguous().to(dev), w0.float().to(dev)).cpu()
    err = (got.double() - img.grad).abs().max().item() / img.grad.abs().max().item()
    assert got.shape == (n, 3, h, w) and err < 1e-5, err


def _convs_of(spec, dtype):
    """The oracle's (w, b) list for a "synth:<seed>[:<gain>]" weight spec, in `dtype`."""
    from nerf_qa_amd import synth
    from oracle import dists_oracle as do
    parts = spec.split(":")
    convs = do.convs_from_numpy(synth.vgg16_weights(int(parts[1]), float(parts[2]) if len(parts) > 2 else 1.0))
    return [(w.to(dtype), b.to(dtype)) for w, b in convs]


def _flip_shares(m, xn, yn, spec, dev):
    """Information, not a gate: the share of ReLU outputs (all 13 layers) whose sign differs between pyramid_keep's
    activations and the float64 oracle's, and the same for the float32 oracle against the float64 one."""
    import grad_replay
    from nerf_qa_amd import autograd, ops
    imgs = torch.cat([torch.from_numpy(xn), torch.from_numpy(yn)])
    a64, _ = grad_replay.oracle_acts(imgs.double(), _convs_of(spec, torch.float64))
    a32, _ = grad_replay.oracle_acts(imgs, _convs_of(spec, torch.float32))
    acts, _, _ = autograd.pyramid_keep(m, imgs.to(dev).contiguous())
    hip = f32 = total = 0
    for l in range(13):
        on = a64[l] > 0
        a = acts[l] if l in ops.TAP_LAYERS else ops.split16_decode(acts[l])
        hip += int(((a.cpu() > 0) != on).sum())
        f32 += int(((a32[l] > 0) != on).sum())
        total += on.numel()
    return hip / total, f32 / total


def _compare_grads(tag, pairs):
    for name, gd, gc in pairs:
        gd, gc = gd.cpu().double(), gc.double()
        scale = gc.abs().max().item()
        d = gd - gc
        err, rms = d.abs().max().item() / scale, d.pow(2).mean().sqrt().item() / gc.pow(2).mean().sqrt().item()
        cos = F.cosine_similarity(gd.flatten(), gc.flatten(), dim=0).item()
        print(f"{tag} d/d{name}: max|grad| {scale:.3e}  max err / max {err:.2e}  rms err / rms {rms:.2e}  cosine {cos:.8f}")
        # a ReLU whose pre-activation is within rounding of zero may switch sides between the float32 kernels and the
        # float64 reference (the reference's own float32 autograd has the same edge against float64, up to 6.5e-3 / 1.0e-3
        # on these pairs): isolated pixels, hence the looser max bound.  tests/test_gpu_grad_chain.py holds the same
        # kernels to float rounding with the masks pinned.
        assert torch.isfinite(gd).all() and err <= 2e-2 and rms <= 3e-3 and cos >= 0.99999, (name, err, rms, cos)


E2E_CASES = [  # (h, w, kinds of the pairs, weights); the first three as before, then NeRF content, a training patch, B = 3, gain 1.3
    (40, 56, ("noise10", "blur"), "synth:1234"), (33, 47, ("indep", "noise02"), "synth:1234"), (96, 112, ("blur", "noise10"), "synth:1234"),
    (64, 80, ("nerf_white", "nerf_float"), "synth:1234"), (256, 256, ("nerf_black",), "synth:1234"),
    (48, 64, ("noise02", "nerf_grad", "blur"), "synth:1234"), (40, 56, ("noise10", "blur"), "synth:1234:1.3")]
E2E_WEIGHTS = (1.0, 0.5, 0.75)  # unequal weights on the pairs


@pytest.mark.parametrize("h,w,kinds,spec", E2E_CASES,
                         ids=["40x56", "33x47_ragged", "96x112", "64x80_nerf", "256x256_nerf", "48x64_B3", "40x56_gain1.3"])
def test_image_gradients_match_autograd_over_the_oracle(h, w, kinds, spec, dev):
    """Reference: FLOAT64 autograd over the oracle (its own float32 run differs from that by the same ReLU flips the
    kernels have, so comparing two float32 evaluations would count the reference's flips too)."""
    from nerf_qa_amd import synth
    from nerf_qa_amd.DISTS_pytorch import DISTS
    m = DISTS(vgg16_path=spec).to(dev).eval()
    b = len(kinds)
    xn, yn = synth.frame_batch([11 + i for i in range(b)], h, w, list(kinds))
    alpha, beta = m.alpha.detach().cpu(), m.beta.detach().cpu()
    xc, yc = torch.from_numpy(xn).double().requires_grad_(), torch.from_numpy(yn).double().requires_grad_()
    wsum = torch.tensor(E2E_WEIGHTS[:b])
    ref = _oracle_score(xc, yc, _convs_of(spec, torch.float64), alpha.double(), beta.double())
    (ref * wsum.double()).sum().backward()
    with torch.no_grad():  # the VALUE against the float32 oracle, as everywhere else
        ref32 = _oracle_score(torch.from_numpy(xn), torch.from_numpy(yn), _convs_of(spec, torch.float32), alpha, beta)
    xd, yd = torch.from_numpy(xn).to(dev).requires_grad_(), torch.from_numpy(yn).to(dev).requires_grad_()
    got = m(xd, yd, require_grad=True)
    assert got.requires_grad and (got.detach().cpu() - ref32).abs().max().item() <= 1e-5
    assert (got.detach().cpu().double() - ref.detach()).abs().max().item() <= 1e-5
    (got * wsum.to(dev)).sum().backward()
    fh, f32 = _flip_shares(m, xn, yn, spec, dev)
    print(f"\nDISTS {h}x{w} B={b} {spec}: ReLU outputs on the other side of zero than float64: kernels {fh:.2e}, float32 oracle {f32:.2e}")
    _compare_grads(f"DISTS {h}x{w}", (("x", xd.grad, xc.grad), ("y", yd.grad, yc.grad)))


@pytest.mark.parametrize("metric", ["dists", "adists"])
def test_gradient_vanishes_at_x_equals_y(metric, dev, oracle_convs):
    """x == y: S1 = S2 = 1 is the maximum, so the gradient is analytically zero.  What the float32 oracle's autograd
    leaves of it on the CPU is the yardstick; the HIP gradient's largest entry may be 8 times the yardstick's largest
    entry (the factor of tests/grad_replay.py).  Both are printed relative to the largest gradient entry of the same x
    against a noise02 y: 'the gradient vanishes relative to a real one'."""
    import grad_replay
    from nerf_qa_amd import synth
    from nerf_qa_amd.ADISTS import ADISTS
    from nerf_qa_amd.DISTS_pytorch import DISTS
    from oracle import adists_oracle as ao
    from oracle import dists_oracle as do
    h, w = 64, 96
    m = (DISTS if metric == "dists" else ADISTS)(vgg16_path="synth:1234").to(dev).eval()

    def oracle(x, y):
        fx, fy = do.vgg_pyramid(x, oracle_convs), do.vgg_pyramid(y, oracle_convs)
        if metric == "adists":
            return ao.adists_from_feats(fx, fy, as_loss=True)
        return do.dists_score(*do.dists_stats(fx, fy), m.alpha.detach().cpu(), m.beta.detach().cpu()).sum()

    def hip(x, y):
        return m(x, y, require_grad=True).sum() if metric == "dists" else m(x, y)
    xn, yn = synth.frame_batch([11], h, w, ["noise02"])
    assert np.array_equal(xn, synth.frame_batch([11], h, w, ["same"])[1])
    xr, yr = torch.from_numpy(xn).requires_grad_(), torch.from_numpy(yn).requires_grad_()
    oracle(xr, yr).backward()
    real = max(xr.grad.abs().max().item(), yr.grad.abs().max().item())
    xc, yc = torch.from_numpy(xn).requires_grad_(), torch.from_numpy(xn.copy()).requires_grad_()
    oracle(xc, yc).backward()
    yard = max(xc.grad.abs().max().item(), yc.grad.abs().max().item())
    xd, yd = torch.from_numpy(xn).to(dev).requires_grad_(), torch.from_numpy(xn.copy()).to(dev).requires_grad_()
    hip(xd, yd).backward()
    assert torch.isfinite(xd.grad).all() and torch.isfinite(yd.grad).all()
    got = max(xd.grad.abs().max().item(), yd.grad.abs().max().item())
    print(f"\n{metric} x == y {h}x{w}: largest gradient entry / largest of x vs noise02 ({real:.3e}): "
          f"float32 oracle {yard / real:.2e}, HIP {got / real:.2e}")
    assert real > 0 and got <= grad_replay.HIP_FACTOR * yard, (got, yard, real)


def test_gradient_only_where_asked_and_with_alpha_beta(dev, oracle_convs):
    """y without grad: only x gets one; alpha/beta (the fine-tuning parameters) get theirs in the same backward;
    without require_grad=True nothing reaches the images (DISTS_pt.py:109-111 runs under no_grad)."""
    from nerf_qa_amd import synth
    from nerf_qa_amd.DISTS_pytorch.DISTS_pt_original import DISTS
    m = DISTS(vgg16_path="synth:1234").to(dev)
    m.alpha.requires_grad_(True)
    m.beta.requires_grad_(True)
    xn, yn = synth.frame_batch([3], 48, 40)
    xd = torch.from_numpy(xn).to(dev).requires_grad_()
    yd = torch.from_numpy(yn).to(dev)
    s = m(xd, yd, require_grad=True)  # (0-d for B = 1 in this variant)
    s.backward()
    assert xd.grad is not None and xd.grad.abs().max().item() > 0 and yd.grad is None
    assert m.alpha.grad is not None and m.alpha.grad.abs().max().item() > 0
    # the oracle's image gradient for the same pair (canonical weighted sum == this variant's with default config)
    xc = torch.from_numpy(xn).requires_grad_()
    ref = _oracle_score(xc, torch.from_numpy(yn), oracle_convs, m.alpha.detach().cpu(), m.beta.detach().cpu())
    ref.sum().backward()
    assert (xd.grad.cpu() - xc.grad).abs().max().item() <= 1e-2 * xc.grad.abs().max().item()
    assert F.cosine_similarity(xd.grad.cpu().flatten(), xc.grad.flatten(), dim=0).item() >= 0.99999
    x2 = torch.from_numpy(xn).to(dev).requires_grad_()
    s2 = m(x2, yd)  # require_grad=False: value only
    s2.backward()
    assert x2.grad is None and abs(s2.item() - s.item()) <= 1e-4


ADISTS_E2E_CASES = [  # the first three as before, then NeRF content, a training patch, B = 3, gain 1.3
    (40, 56, ("noise10", "blur"), "synth:1234"), (96, 112, ("blur", "noise10"), "synth:1234"), (63, 85, ("indep", "noise02"), "synth:1234"),
    (64, 80, ("nerf_white", "nerf_float"), "synth:1234"), (256, 256, ("noise10",), "synth:1234"),
    (48, 64, ("noise02", "nerf_grad", "blur"), "synth:1234"), (40, 56, ("noise10", "blur"), "synth:1234:1.3")]


@pytest.mark.parametrize("h,w,kinds,spec", ADISTS_E2E_CASES,
                         ids=["40x56", "96x112", "63x85_ragged", "64x80_nerf", "256x256", "48x64_B3", "40x56_gain1.3"])
def test_adists_loss_gradients_match_autograd_over_the_oracle(h, w, kinds, spec, dev):
    """ADISTS.forward(x, y) -- as_loss=True, the reference's default -- under autograd (ADISTS.py:139-141, 195): the loss
    and its image gradients against FLOAT64 torch autograd over the CPU oracle's pyramid + head (windowed stages and the
    global fall-back of the small deep maps both occur at these sizes)."""
    from nerf_qa_amd import synth
    from nerf_qa_amd.ADISTS import ADISTS
    from oracle import adists_oracle as ao
    from oracle import dists_oracle as do
    m = ADISTS(vgg16_path=spec).to(dev).eval()
    b = len(kinds)
    xn, yn = synth.frame_batch([21 + i for i in range(b)], h, w, list(kinds))
    c64 = _convs_of(spec, torch.float64)
    xc, yc = torch.from_numpy(xn).double().requires_grad_(), torch.from_numpy(yn).double().requires_grad_()
    ref = ao.adists_from_feats(do.vgg_pyramid(xc, c64), do.vgg_pyramid(yc, c64), as_loss=True)
    ref.backward()
    ref32 = ao.adists(torch.from_numpy(xn), torch.from_numpy(yn), _convs_of(spec, torch.float32), as_loss=True)
    xd, yd = torch.from_numpy(xn).to(dev).requires_grad_(), torch.from_numpy(yn).to(dev).requires_grad_()
    got = m(xd, yd)  # as_loss=True
    assert got.dim() == 0 and got.requires_grad and abs(got.item() - ref32.item()) <= 1e-4 and abs(got.item() - ref.item()) <= 1e-4
    with torch.no_grad():
        assert abs(got.item() - m(xd.detach(), yd.detach()).item()) <= 1e-7  # the value IS the scoring path's
    got.backward()
    fh, f32 = _flip_shares(m, xn, yn, spec, dev)
    print(f"\nA-DISTS {h}x{w} B={b} {spec}: ReLU outputs on the other side of zero than float64: kernels {fh:.2e}, float32 oracle {f32:.2e}")
    _compare_grads(f"A-DISTS {h}x{w}", (("x", xd.grad, xc.grad), ("y", yd.grad, yc.grad)))


def test_adists_gradient_only_where_asked(dev):
    from nerf_qa_amd import synth
    from nerf_qa_amd.ADISTS import ADISTS
    m = ADISTS(vgg16_path="synth:1234").to(dev).eval()
    xn, yn = synth.frame_batch([5], 48, 64)
    xd, yd = torch.from_numpy(xn).to(dev), torch.from_numpy(yn).to(dev).requires_grad_()
    loss = m(xd, yd)  # only the render carries a gradient (the NeRF-training use)
    loss.backward()
    assert yd.grad is not None and yd.grad.abs().max().item() > 0 and xd.grad is None
    with torch.no_grad():
        assert not m(xd, yd).requires_grad  # no grad mode: the fused kernel alone
    assert not m(xd, yd.detach()).requires_grad  # nothing requires grad: likewise
    s = m(xd, yd, as_loss=False)  # per-pair scores never carry a graph (ADISTS.py:142-145 runs them under no_grad)
    assert s.shape == (1,) and not s.requires_grad
