"""The statistics of a loss against a prepared target on their own (include/nqa.h: nqa_dists_stats_target,
nqa_dists_stats_nhwc_backward_from; csrc/nqa_loss_backward.hip: loss_stats_sums_kernel reused, loss_stats_fold_kernel new).

  * S1 / S2 against the same formula in float64 torch on the maps read back, |dS| <= 2.4e-7: two float32 steps at 1.0.
    The one rounding to float is 6e-8; the fp64 sums' cancellation against c = 1e-6 stays below 1e-9.  Channels dead in
    both maps give S1 = S2 = 1 exactly; nothing outside the tap's columns is written.
  * the backward started from the forward's partials equals nqa_dists_stats_nhwc_backward on the same maps and upstream
    gradients bit for bit: gx and gy together, and each alone with the other null.

Shapes: the tap sizes of the frames of tests/test_gpu_target_loss.py where the kernels can go wrong -- H*W no multiple of
the pixel lanes (33x47, 17x24, 9x13, 5x7), a block range shorter than its lanes (3x4, 1x1), more than one block (33x47 at
C=64 is 13 blocks of 128 pixels) -- with B = 2 and the columns at an offset inside wider rows, so that the batch stride and
s_stride are exercised.

Measured on an MI355X: see DESIGN.md 4.15."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SPEC = "synth:1234"
S_BOUND = 2.4e-7  # two float32 steps at 1.0 (2 * 2^-23)
SHAPES = [(64, 33, 47), (64, 40, 56), (128, 17, 24), (256, 9, 13), (512, 5, 7), (512, 3, 4), (512, 1, 1), (64, 1, 1),
          (16, 6, 5), (1024, 2, 3)]  # (C, H, W); the last two: the ends of the C range the entry points take


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _s64(tx, ty):
    """S1, S2 (B, C) of float NHWC maps by the kernels' own formula (DISTS_pt.py:131-139 from the five sums), float64."""
    x, y = tx.detach().cpu().double().flatten(1, 2), ty.detach().cpu().double().flatten(1, 2)
    mx, my = x.mean(1), y.mean(1)
    vx, vy, cov = (x * x).mean(1) - mx * mx, (y * y).mean(1) - my * my, (x * y).mean(1) - mx * my
    c = 1e-6
    return (2 * mx * my + c) / (mx * mx + my * my + c), (2 * cov + c) / (vx + vy + c)


def _random_maps(c, h, w, gen):
    """Non-negative maps like a ReLU output, y a distorted x; channel 3 dead in x, 7 in y, 9 in both, 11 in both for
    pair 1 only."""
    tx = torch.randn(2, h, w, c, generator=gen).clamp_min(0)
    ty = (tx + 0.3 * torch.randn(2, h, w, c, generator=gen)).clamp_min(0)
    tx[..., 3] = 0
    ty[..., 7] = 0
    tx[..., 9] = 0
    ty[..., 9] = 0
    tx[1, ..., 11] = 0
    ty[1, ..., 11] = 0
    return tx, ty


def _check_s(what, tx, ty, col, pad, dev):
    """Runs nqa_dists_stats_target into columns col .. col + C of rows `pad` wider than C; returns (S1, S2) of the tap."""
    from nerf_qa_amd import ops
    b, c = tx.shape[0], tx.shape[-1]
    s1 = torch.full((b, c + pad), -7.0, device=dev)
    s2 = torch.full((b, c + pad), -9.0, device=dev)
    part = ops.dists_stats_target(tx, ty, s1, s2, col)
    assert part.dtype == torch.uint8 and part.numel() == ops.lib().nqa_dists_stats_target_bytes(b, *tx.shape[1:])
    s1, s2 = s1.cpu(), s2.cpu()
    for s, fill in ((s1, -7.0), (s2, -9.0)):  # one writer per output, and nothing else written
        assert bool((s[:, :col] == fill).all()) and bool((s[:, col + c:] == fill).all())
    g1, g2 = s1[:, col:col + c], s2[:, col:col + c]
    w1, w2 = _s64(tx, ty)
    e1, e2 = (g1.double() - w1).abs().max().item(), (g2.double() - w2).abs().max().item()
    print(f"[target stats] {what}: max|dS1| {e1:.2e}  max|dS2| {e2:.2e}  (bound {S_BOUND:.1e})")
    assert torch.isfinite(g1).all() and torch.isfinite(g2).all()
    assert e1 <= S_BOUND and e2 <= S_BOUND, (what, e1, e2)
    return g1, g2


@pytest.mark.parametrize("c,h,w", SHAPES, ids=[f"C{c}-{h}x{w}" for c, h, w in SHAPES])
def test_s1_s2_of_random_maps_against_float64(c, h, w, dev):
    print()
    gen = torch.Generator().manual_seed(1000 * c + h)
    tx, ty = _random_maps(c, h, w, gen)
    g1, g2 = _check_s(f"random C={c} {h}x{w}", tx.to(dev), ty.to(dev), 5, 8, dev)
    for s in (g1, g2):  # dead in both maps: (0 + c) / (0 + c)
        assert bool((s[:, 9] == 1).all()) and bool((s[1, 11] == 1).all())
    if h * w >= 12:  # (enough pixels that a channel drawn live is live)
        assert float(g2[0, 11]) != 1 and float(g1[0, 3]) != 1  # live in pair 0; dead on one side only


def test_s1_s2_of_real_taps_against_float64(dev):
    """The taps of a nerf_white pair beside a nerf_float one: constant backgrounds, exactly dead channels of their own."""
    from nerf_qa_amd import autograd, synth
    from nerf_qa_amd.DISTS_pytorch import DISTS
    print()
    m = DISTS(vgg16_path=SPEC, precision="f32s").to(dev).eval()
    xn, yn = synth.frame_batch([54, 55], 40, 56, ["nerf_white", "nerf_float"])
    tx = autograd.pyramid_taps(m, torch.from_numpy(xn).to(dev))
    ty = autograd.pyramid_taps(m, torch.from_numpy(yn).to(dev))
    dead = 0
    for k, (fx, fy) in enumerate(zip(tx, ty)):
        g1, g2 = _check_s(f"40x56 nerf_white+nerf_float tap {k + 1} {tuple(fx.shape)}", fx, fy, 3, 3, dev)
        both = ((fx.flatten(1, 2) == 0).all(1) & (fy.flatten(1, 2) == 0).all(1)).cpu()
        dead += int(both.sum())
        assert bool((g1[both] == 1).all()) and bool((g2[both] == 1).all())
    assert dead > 0


@pytest.mark.parametrize("c,h,w", SHAPES, ids=[f"C{c}-{h}x{w}" for c, h, w in SHAPES])
def test_backward_from_the_forwards_partials_is_the_whole_backward_bit_for_bit(c, h, w, dev):
    from nerf_qa_amd import ops
    gen = torch.Generator().manual_seed(2000 * c + w)
    tx, ty = (t.to(dev) for t in _random_maps(c, h, w, gen))
    g1, g2 = torch.randn(2, c + 8, generator=gen).to(dev), torch.randn(2, c + 8, generator=gen).to(dev)
    s1, s2 = torch.empty(2, c, device=dev), torch.empty(2, c, device=dev)
    part = ops.dists_stats_target(tx, ty, s1, s2, 0)
    kept = part.clone()
    wx, wy = ops.dists_stats_nhwc_backward(tx, ty, g1, g2, 5)
    gx, gy = ops.dists_stats_nhwc_backward_from(tx, ty, part, g1, g2, 5)
    assert torch.isfinite(wx).all() and torch.isfinite(wy).all()
    assert h * w == 1 or (wx.abs().max().item() > 0 and wy.abs().max().item() > 0)
    assert _same_bits(gx, wx) and _same_bits(gy, wy)
    ox, none = ops.dists_stats_nhwc_backward_from(tx, ty, part, g1, g2, 5, need_y=False)
    assert none is None and _same_bits(ox, wx)
    none, oy = ops.dists_stats_nhwc_backward_from(tx, ty, part, g1, g2, 5, need_x=False)
    assert none is None and _same_bits(oy, wy)
    assert torch.equal(part, kept)  # the partials are read, never written: a second backward starts from the same numbers
