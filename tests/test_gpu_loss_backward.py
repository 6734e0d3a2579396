"""DISTS as a loss: `DISTS(x, y, require_grad=True)` inside an optimisation step (nerf_qa_amd/autograd.py: dists_backward,
pyramid_backward_device; csrc/nqa_loss_backward.hip and the scaled forms of csrc/nqa_backward.hip).

What is held here:
  * a loss step enqueues without one device -> host read (torch's sync debug mode set to "error");
  * a y that takes no gradient is left out of the chain, and x's gradient is then the two-sided call's bit for bit;
  * the gradient of a pair does not depend on what else is in the batch, bit for bit (per-image exponents);
  * the device-scaled chain against the float64 replay on its own masks (tests/grad_replay.py, the helpers and the cases
    of tests/test_gpu_grad_chain.py by import), to grad_replay.bound; bit-identical to the host-scaled chain on one image;
  * the NHWC statistics' gradient against float64 autograd of dists_oracle.dists_stats at the device taps, to the bound
    of tests/test_gpu_feats_grad.py: |g - g64| <= 1e-5 |g64| + 1e-6 max|g64| elementwise;
  * the exponent reduction and each scaled kernel on their own.

The bit-for-bit comparisons rest on every kernel of the chain (and of pyramid_keep) treating the images of a batch
independently.  One departure from the plan this was written to: the taps of the image that takes no gradient come
from pyramid_keep's own launches (autograd.pyramid_taps), not from ops.vgg_pyramid -- the fused forward runs stage 1
in another kernel, whose sums are ordered differently, and x's gradient would then differ in the last bits between the
one-sided and the two-sided call.

Measured on an MI355X (run with -s for the lines): the device-scaled chain on the eleven cases e_max 7.4e-8 .. 1.0e-6,
e_rms 6.7e-8 .. 1.2e-6 against float32-replay yardsticks of 3.1e-8 .. 5.6e-7 (bound in force 8e-6 throughout); the NHWC
statistics' gradient 5e-9 .. 6e-8 of the largest entry per tap and side, 2e-16 .. 1e-15 of a real gradient at x == y;
ops.vgg_pyramid's f32s taps against pyramid_keep's: no tap bit-equal, 5e-7 .. 2e-6 of the tap's maximum apart, while
an image alone and the same image inside a batch give bit-equal taps.  Every bit-for-bit comparison below holds as
stated: no kernel of the chain mixes the images of a batch.  Wall time of this file: 17 s.

x == y in the statistics' test: the true gradient is zero there, float64 autograd and the kernels both return rounding
residue (1e-16 of a real gradient), and `1e-6 max|g64|` of residue is no bound at all.  As in
test_gpu_grad_chain.test_stats_gradient_vanishes_at_x_equals_y the max|g64| of that one case is the float64 gradient of
the SAME x against a noise02 y, same tap and side: the gradient vanishes relative to a real one.
"""
import math

import pytest
import torch

import grad_replay
from grad_replay import bound, errors
from test_gpu_grad_chain import CASES, _convs, _forward, _random_g_taps, _real_g_taps, _score_grads

pytestmark = pytest.mark.gpu

SPEC = "synth:1234"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev):
    from nerf_qa_amd.DISTS_pytorch import DISTS
    return DISTS(vgg16_path=SPEC, precision="f32s").to(dev).eval()


def _pairs(seeds, h, w, kinds, dev):
    from nerf_qa_amd import synth
    xn, yn = synth.frame_batch(list(seeds), h, w, list(kinds))
    return torch.from_numpy(xn).to(dev), torch.from_numpy(yn).to(dev)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ---- 1. no host synchronisation -------------------------------------------------------------------------------------
def test_loss_step_enqueues_without_a_host_read(model, dev):
    """Forward and backward are both under the guard (the f32s forward has no synchronising call of its own)."""
    x0, y = _pairs((3, 4), 64, 80, ("noise10", "nerf_white"), dev)

    def step():
        x = x0.clone().requires_grad_()
        loss = model(x, y, require_grad=True, batch_average=True)
        loss.backward()
        return x.grad

    warm = step()  # packing, workspace, the backward's weight blobs
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = step()
    finally:
        torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
    assert torch.isfinite(got).all() and got.abs().max().item() > 0 and _same_bits(got, warm)


def test_adists_taps_backward_enqueues_without_a_host_read(dev):
    """PyramidTaps.backward (A-DISTS as a loss) runs the same device-scaled chain."""
    from nerf_qa_amd import autograd
    from nerf_qa_amd.ADISTS import ADISTS
    m = ADISTS(vgg16_path=SPEC).to(dev).eval()
    x0, _ = _pairs((5,), 48, 64, ("noise10",), dev)
    gen = torch.Generator().manual_seed(1)

    def step(grads):
        x = x0.clone().requires_grad_()
        taps = autograd.PyramidTaps.apply(x, m)
        torch.autograd.backward(taps, grads)
        return x.grad

    with torch.no_grad():
        shapes = [t.shape for t in autograd.PyramidTaps.apply(x0, m)]
    grads = [(torch.randn(s, generator=gen) * 1e-6).to(dev) for s in shapes]
    warm = step(grads)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = step(grads)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
    assert torch.isfinite(got).all() and got.abs().max().item() > 0 and _same_bits(got, warm)


# ---- 2. one-sided ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,kinds", [(40, 56, ("noise10", "blur")), (33, 47, ("nerf_white",)), (96, 112, ("nerf_float", "indep", "noise02"))])
def test_one_sided_gradient_is_the_two_sided_one_bit_for_bit(h, w, kinds, model, dev):
    from nerf_qa_amd import autograd
    x0, y0 = _pairs(range(11, 11 + len(kinds)), h, w, kinds, dev)
    wts = torch.tensor([1.0, 0.5, 0.75][:len(kinds)], device=dev)
    x2, y2 = x0.clone().requires_grad_(), y0.clone().requires_grad_()
    (model(x2, y2, require_grad=True) * wts).sum().backward()
    x1, y1 = x0.clone().requires_grad_(), y0.clone()
    (model(x1, y1, require_grad=True) * wts).sum().backward()
    assert y1.grad is None and x1.grad is not None and x2.grad.abs().max().item() > 0
    assert _same_bits(x1.grad, x2.grad)
    xb, yb = x0.clone(), y0.clone().requires_grad_()  # and the other side
    (model(xb, yb, require_grad=True) * wts).sum().backward()
    assert xb.grad is None and _same_bits(yb.grad, y2.grad)
    # dists_backward itself
    g1, g2 = _score_grads(model, len(kinds), dev)
    gx, gy = autograd.dists_backward(model, x0, y0, g1, g2, need=(True, False))
    assert gy is None and gx is not None and gx.shape == x0.shape
    fx, fy = autograd.dists_backward(model, x0, y0, g1, g2)
    assert _same_bits(gx, fx) and fy is not None
    hx, hy = autograd.dists_backward(model, x0, y0, g1, g2, need=(False, True))
    assert hx is None and _same_bits(hy, fy)
    assert autograd.dists_backward(model, x0, y0, g1, g2, need=(False, False)) == (None, None)
    # the first form stays callable (the baseline of tools/gpu_loss_step_bench.py) and agrees to rounding
    px, py = autograd.dists_backward(model, x0, y0, g1, g2, host_scaled=True)
    for new, old in ((fx, px), (fy, py)):
        assert (new - old).abs().max().item() <= 1e-4 * old.abs().max().item()


# ---- 3. batch independence ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(40, 56), (64, 96)])
def test_a_pairs_gradient_does_not_depend_on_its_batch_neighbour(h, w, model, dev):
    """Pair 0 alone against pair 0 next to a pair whose upstream gradient is 2^12 times larger."""
    x0, y0 = _pairs((21, 22), h, w, ("noise02", "nerf_grad"), dev)
    xa, ya = x0[:1].clone().requires_grad_(), y0[:1].clone().requires_grad_()
    model(xa, ya, require_grad=True).sum().backward()
    xb, yb = x0.clone().requires_grad_(), y0.clone().requires_grad_()
    (model(xb, yb, require_grad=True) * torch.tensor([1.0, 4096.0], device=dev)).sum().backward()
    assert xa.grad.abs().max().item() > 0 and xb.grad[1].abs().max().item() > 64 * xb.grad[0].abs().max().item()
    assert _same_bits(xa.grad[0], xb.grad[0]) and _same_bits(ya.grad[0], yb.grad[0])


# ---- 4. the device-scaled chain against the float64 replay ----------------------------------------------------------
@pytest.mark.parametrize("spec,h,w,kinds,gk", CASES,
                         ids=[f"{h}x{w}-n{2 * len(k)}-{'+'.join(k)}-g{s.split(':')[2] if s.count(':') > 1 else '1'}-{g}"
                              for s, h, w, k, g in CASES])
def test_device_scaled_chain_matches_float64_replay_on_its_own_masks(spec, h, w, kinds, gk, dev):
    from nerf_qa_amd import autograd
    m, b, imgs, acts, taps, pooled, acts_c, taps_c = _forward(spec, h, w, kinds, 31)
    g_taps = _real_g_taps(m, b, taps) if gk == "real" else _random_g_taps(taps, h * w)
    got = autograd.pyramid_backward_device(m, acts, taps, pooled, g_taps).cpu()
    g_c = [g.cpu() for g in g_taps]
    r64 = grad_replay.replay(acts_c, taps_c, g_c, _convs(spec), torch.float64)
    r32 = grad_replay.replay(acts_c, taps_c, g_c, _convs(spec), torch.float32)
    assert torch.isfinite(got).all() and torch.isfinite(r64).all() and r64.abs().max().item() > 0
    y_max, y_rms = errors(r32, r64)
    e_max, e_rms = errors(got, r64)
    print(f"\n[device chain] {h}x{w} n={2 * b} {'+'.join(kinds)} {spec} {gk}: float32 replay e_max {y_max:.2e} e_rms {y_rms:.2e}"
          f"  ->  HIP e_max {e_max:.2e} e_rms {e_rms:.2e}")
    assert e_max <= bound(y_max) and e_rms <= bound(y_rms), (e_max, bound(y_max), e_rms, bound(y_rms))
    again = autograd.pyramid_backward_device(m, acts, taps, pooled, g_taps).cpu()
    assert torch.equal(got, again)


@pytest.mark.parametrize("h,w,scale", [(1, 1, 1.0), (33, 47, 1e-8), (96, 112, 1e-8), (64, 96, 3e4)])
def test_device_and_host_scaled_chain_agree_bit_for_bit_on_one_image(h, w, scale, model, dev):
    """One image: the per-image exponents ARE the host path's batch exponents."""
    from nerf_qa_amd import autograd
    x, _ = _pairs((41,), h, w, ("nerf_white",), dev)
    acts, taps, pooled = autograd.pyramid_keep(model, x.contiguous())
    g_taps = [g * scale for g in _random_g_taps(taps, h + w)]
    host = autograd.pyramid_backward(model, acts, taps, pooled, g_taps)
    device = autograd.pyramid_backward_device(model, acts, taps, pooled, g_taps)
    assert torch.isfinite(host).all() and host.abs().max().item() > 0 and _same_bits(host, device)
    premasked = [g * (t > 0) for g, t in zip(g_taps, taps)]
    assert _same_bits(host, autograd.pyramid_backward_device(model, acts, taps, pooled, premasked, masked=True))


def test_huge_gradients_on_dead_channels_change_nothing_in_the_device_chain(dev):
    """The taps' ReLU masks come BEFORE the first exponent (A-DISTS hands dead channels gradients ~1e12 times the live)."""
    from nerf_qa_amd import autograd
    m, b, imgs, acts, taps, pooled, acts_c, taps_c = _forward(SPEC, 40, 56, ("nerf_white",), 31)
    g = [x * 1e-3 for x in _random_g_taps(taps, 9)]
    dead = [t == 0 for t in taps]
    assert all(int(d.sum()) > 0 for d in dead)
    g_huge = [torch.where(d, x * 1e8, x) for x, d in zip(g, dead)]
    g_zero = [torch.where(d, torch.zeros_like(x), x) for x, d in zip(g, dead)]
    a = autograd.pyramid_backward_device(m, acts, taps, pooled, g_huge)
    z = autograd.pyramid_backward_device(m, acts, taps, pooled, g_zero)
    assert torch.isfinite(a).all() and a.abs().max().item() > 0 and torch.equal(a, z)


# ---- 5. the statistics' gradient on NHWC taps -----------------------------------------------------------------------
def _close(got, want, what, scale=None):
    """|g - g64| <= 1e-5 |g64| + 1e-6 max|g64|, elementwise over one map (tests/test_gpu_feats_grad.py); scale: the
    max|g64| to use instead of want's own (x == y only, see the module docstring)."""
    g = got.detach().cpu().double()
    assert g.shape == want.shape and torch.isfinite(g).all(), what
    mx = want.abs().max() if scale is None else scale
    assert mx > 0, what
    tol = 1e-5 * want.abs() + 1e-6 * mx
    err = (g - want).abs()
    print(f"[nhwc stats] {what}: max|g64| {float(want.abs().max()):.2e}  max err / max {float(err.max() / mx):.2e}")
    assert bool((err <= tol).all()), (what, int((err > tol).sum()), (err / mx).max().item())


def _stats64(tx, ty, g1, g2):
    """float64 autograd of dists_oracle.dists_stats on CPU copies of NHWC taps, times the taps' ReLU masks: NHWC."""
    from oracle import dists_oracle as do
    fx = [t.cpu().double().permute(0, 3, 1, 2).contiguous().requires_grad_() for t in tx]
    fy = [t.cpu().double().permute(0, 3, 1, 2).contiguous().requires_grad_() for t in ty]
    s1, s2 = do.dists_stats(fx, fy)
    (s1 * g1.cpu().double() + s2 * g2.cpu().double()).sum().backward()
    return ([(f.grad * (f.detach() > 0)).permute(0, 2, 3, 1) for f in fx], [(f.grad * (f.detach() > 0)).permute(0, 2, 3, 1) for f in fy])


def _nhwc_case(h, w, kinds):
    from nerf_qa_amd import ops
    m, b, imgs, acts, taps, pooled, acts_c, taps_c = _forward(SPEC, h, w, kinds, 31)
    g1, g2 = _score_grads(m, b, taps[0].device)
    g1, g2 = g1[:, 3:].contiguous(), g2[:, 3:].contiguous()  # the five taps' columns
    tx, ty = [t[:b] for t in taps], [t[b:] for t in taps]
    got, off = [], 0
    for fx, fy in zip(tx, ty):
        gx, gy = ops.dists_stats_nhwc_backward(fx, fy, g1, g2, off)
        ax, ay = ops.dists_stats_nhwc_backward(fx, fy, g1, g2, off)
        assert _same_bits(gx, ax) and _same_bits(gy, ay)  # two runs
        ox, none = ops.dists_stats_nhwc_backward(fx, fy, g1, g2, off, need_y=False)
        assert none is None and _same_bits(ox, gx)
        none, oy = ops.dists_stats_nhwc_backward(fx, fy, g1, g2, off, need_x=False)
        assert none is None and _same_bits(oy, gy)
        got.append((gx, gy))
        off += fx.shape[-1]
    return tx, ty, got, _stats64(tx, ty, g1, g2)


@pytest.mark.parametrize("h,w,kinds", [(40, 56, ("noise10", "blur")), (40, 56, ("nerf_white", "nerf_float")), (40, 56, ("nerf_black", "nerf_grad")),
                                      (33, 47, ("indep", "nerf_white", "noise02")), (1, 1, ("noise10",))])
def test_nhwc_stats_gradient_matches_float64_autograd(h, w, kinds, dev):
    print()
    tx, ty, got, (rx, ry) = _nhwc_case(h, w, kinds)
    for k in range(5):
        if h * w == 1 and float(rx[k].abs().max()) == 0 and float(ry[k].abs().max()) == 0:
            assert float(got[k][0].abs().max()) == 0 and float(got[k][1].abs().max()) == 0  # one pixel: no variance, no gradient left
            continue
        _close(got[k][0], rx[k], f"{h}x{w} {'+'.join(kinds)} tap {k + 1} d/dx")
        _close(got[k][1], ry[k], f"{h}x{w} {'+'.join(kinds)} tap {k + 1} d/dy")
        for g, t in ((got[k][0], tx[k]), (got[k][1], ty[k])):
            assert bool((g[t == 0] == 0).all())  # the tap's ReLU mask, exactly


def test_nhwc_stats_gradient_vanishes_at_x_equals_y(dev):
    print()
    _, _, _, (dx, dy) = _nhwc_case(40, 56, ("noise02",))
    _, _, got, (rx, ry) = _nhwc_case(40, 56, ("same",))
    for k in range(5):
        _close(got[k][0], rx[k], f"40x56 x == y tap {k + 1} d/dx", scale=dx[k].abs().max())
        _close(got[k][1], ry[k], f"40x56 x == y tap {k + 1} d/dy", scale=dy[k].abs().max())


@pytest.mark.parametrize("c", [64, 128, 512])
def test_nhwc_stats_gradient_is_exactly_zero_on_dead_channels(c, dev):
    """Channels that are exactly dead in x, in y, or in both (every NeRF-like pair has them): the gradient with respect
    to a dead map is exactly 0 there, and the live side is still right."""
    from nerf_qa_amd import ops
    gen = torch.Generator().manual_seed(c)
    b, h, w = 2, 9, 13
    tx = torch.randn(b, h, w, c, generator=gen).clamp_min(0)
    ty = (tx + 0.3 * torch.randn(b, h, w, c, generator=gen)).clamp_min(0)
    tx[..., 3] = 0
    ty[..., 7] = 0
    tx[..., 9] = 0
    ty[..., 9] = 0
    tx[1, ..., 20] = 0  # dead in one pair only
    g1, g2 = torch.randn(b, c + 5, generator=gen), torch.randn(b, c + 5, generator=gen)
    gx, gy = ops.dists_stats_nhwc_backward(tx.to(dev), ty.to(dev), g1.to(dev), g2.to(dev), 5)
    (rx,), (ry,) = _stats64([tx], [ty], g1[:, 5:], g2[:, 5:])
    _close(gx, rx, f"C={c} d/dx")
    _close(gy, ry, f"C={c} d/dy")
    gx, gy = gx.cpu(), gy.cpu()
    assert float(gx[..., 3].abs().max()) == 0 and float(gx[..., 9].abs().max()) == 0 and float(gx[1, ..., 20].abs().max()) == 0
    assert float(gy[..., 7].abs().max()) == 0 and float(gy[..., 9].abs().max()) == 0
    assert float(gy[..., 3].abs().max()) > 0 and float(gx[..., 7].abs().max()) > 0 and float(gx[0, ..., 20].abs().max()) > 0


# ---- 6. the exponents and the scaled kernels on their own -----------------------------------------------------------
def _want_k(mx):
    return 8 - math.frexp(mx)[1] if mx > 0 and math.isfinite(mx) else 0


@pytest.mark.parametrize("shape", [(7, 1, 1, 64), (7, 5, 9, 64), (7, 40, 56, 128)])
def test_grad_exponent_against_frexp(shape, dev):
    from nerf_qa_amd import ops
    gen = torch.Generator().manual_seed(shape[1])
    g = torch.randn(shape, generator=gen)
    g[0] *= 1e-8
    g[1] = 0
    g[2] *= 1e-3
    g[2].view(-1)[17] = float("inf")
    g[3] *= 3e5
    g[4] *= 1e-3
    g[4].view(-1)[-1] = float("nan")
    g[5] = 0
    g[5].view(-1)[-3] = -2.0 ** -130  # a subnormal float, negative, the only entry
    g[6] = 0
    g[6].view(-1)[0] = -256.0  # exactly a power of two: [128, 256) is half open
    want = []
    for i in range(shape[0]):
        a = g[i].abs()
        want.append(0 if bool(torch.isnan(a).any()) else _want_k(a.max().item()))
    assert want[1] == 0 and want[2] == 0 and want[4] == 0 and want[5] == 137 and want[6] == -1 and want[0] > 20 and want[3] < -5
    k = torch.full((shape[0],), 99, dtype=torch.int32, device=dev)
    total = torch.arange(shape[0], dtype=torch.int32, device=dev)
    gd = g.to(dev)
    ops.grad_exponent(gd, k, total)
    assert k.cpu().tolist() == want
    assert total.cpu().tolist() == [i + v for i, v in enumerate(want)]
    ops.grad_exponent(gd, k, total)  # the running total accumulates
    assert total.cpu().tolist() == [i + 2 * v for i, v in enumerate(want)]
    k2 = torch.empty_like(k)
    ops.grad_exponent(gd, k2)  # no total
    assert k2.cpu().tolist() == want
    for i in (0, 3):  # the rule itself: max |g| 2^k in [128, 256)
        assert 128 <= g[i].abs().max().item() * 2.0 ** want[i] < 256


def _pow2(k):
    """2^k[i] as a float32 (n,1,1,1) tensor, exact (|k| < 127 here)."""
    return torch.ldexp(torch.ones(k.numel(), device=k.device), k).view(-1, 1, 1, 1)


@pytest.mark.parametrize("n,h,w", [(3, 1, 1), (3, 5, 7), (2, 33, 47)])
def test_scaled_kernels_equal_their_plain_forms_on_prescaled_inputs(n, h, w, dev):
    from nerf_qa_amd import ops
    gen = torch.Generator().manual_seed(n * 100 + h)
    k = torch.tensor([27, -9, 0][:n], dtype=torch.int32, device=dev)
    K = torch.tensor([41, -3, 13][:n], dtype=torch.int32, device=dev)
    # relu_mask_split16: float and split16 activations
    for c in (64, 256):
        act = torch.randn(n, h, w, c, generator=gen).clamp_min(0).to(dev)
        g = (torch.randn(n, h, w, c, generator=gen) * 1e-6).to(dev)
        for split in (False, True):
            a = ops.split16_encode(act) if split else act
            assert _same_bits(ops.relu_mask_split16_scaled(g, a, split, k), ops.relu_mask_split16(g * _pow2(k), a, split))
    # l2pool_backward: the tap's own gradient in the running scale + the pool gradient
    c = 64
    tap = (torch.rand(n, h, w, c, generator=gen) * (torch.rand(n, h, w, c, generator=gen) > 0.3)).to(dev)
    gp = (torch.randn(n, (h + 1) // 2, (w + 1) // 2, c, generator=gen) * 100).to(dev)
    gt = (torch.randn(n, h, w, c, generator=gen) * 1e-9).to(dev)
    want = (gt * _pow2(K)).contiguous()
    ops.l2pool_backward(tap, ops.l2pool(tap, "f32s"), gp, want)
    assert _same_bits(ops.l2pool_backward_scaled(tap, gp, gt, K), want)
    # conv1_1_backward: pending exponent and ReLU mask on the way in, the total taken out at the end
    w0 = (torch.randn(64, 3, 3, 3, generator=gen) * 0.2).to(dev)
    act0 = ops.split16_encode(torch.randn(n, h, w, 64, generator=gen).clamp_min(0).to(dev))
    g = (torch.randn(n, h, w, 64, generator=gen) * 1e-7).to(dev)
    gm = (g * _pow2(k)) * (ops.split16_decode(act0) > 0)
    want = ops.conv1_1_backward(gm, w0) * _pow2(-K)
    assert _same_bits(ops.conv1_1_backward_scaled(g, act0, w0, k, K), want)
    assert _same_bits(ops.conv1_1_backward_scaled(g, None, w0, k, K), ops.conv1_1_backward(g * _pow2(k), w0) * _pow2(-K))
