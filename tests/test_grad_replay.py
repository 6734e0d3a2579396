"""The gradient tests' float64 reference (tests/grad_replay.py) proved on the CPU: with the ReLU masks and taps of a
float64 oracle forward, the layer-by-layer replay IS float64 torch autograd of dists_oracle.vgg_pyramid -- the same
arithmetic in another order -- so the two agree to 1e-10 of the largest gradient (float64 epsilon 1.1e-16 times the
few thousand terms of a 512-channel 3x3 sum, twelve layers deep, leaves orders of magnitude of room)."""
import pytest
import torch

import grad_replay
from oracle import dists_oracle as do


def _convs64(oracle_convs):
    return [(w.double(), b.double()) for w, b in oracle_convs]


@pytest.mark.parametrize("kinds", [("noise10", "blur"), ("nerf_white", "nerf_float")], ids=["texture", "nerf"])
@pytest.mark.parametrize("g_kind", ["random", "stats"])
def test_replay_is_float64_autograd_of_the_oracle_pyramid(kinds, g_kind, oracle_convs, alpha_beta):
    from nerf_qa_amd import synth
    h, w = 33, 47  # ragged at every stage
    xn, yn = synth.frame_batch([11, 12], h, w, list(kinds))
    imgs = torch.cat([torch.from_numpy(xn), torch.from_numpy(yn)]).double().requires_grad_()  # (4,3,h,w): x0 x1 y0 y1
    convs = _convs64(oracle_convs)
    feats = do.vgg_pyramid(imgs, convs)
    acts, taps = grad_replay.oracle_acts(imgs.detach(), convs)
    for k in range(5):
        assert torch.equal(taps[k].permute(0, 3, 1, 2), feats[k + 1].detach())  # the kept forward is the oracle's
    if g_kind == "random":
        gen = torch.Generator().manual_seed(5)
        g_nchw = [torch.randn(f.shape, generator=gen, dtype=torch.float64) for f in feats[1:]]
    else:  # the gradients a DISTS score sends down: d(score)/d(taps) through dists_stats, the raw-image tap left out
        alpha, beta = (t.double() for t in alpha_beta)
        det = [f.detach().requires_grad_() for f in feats]
        s1, s2 = do.dists_stats([f[:2] for f in det], [f[2:] for f in det])
        g_nchw = list(torch.autograd.grad(do.dists_score(s1, s2, alpha, beta).sum(), det[1:]))
    want, = torch.autograd.grad(sum((f * g).sum() for f, g in zip(feats[1:], g_nchw)), imgs)
    got = grad_replay.replay(acts, taps, [g.permute(0, 2, 3, 1) for g in g_nchw], convs, torch.float64)
    assert got.dtype == torch.float64 and got.shape == imgs.shape
    assert torch.isfinite(got).all() and torch.isfinite(want).all() and want.abs().max().item() > 0
    e_max, e_rms = grad_replay.errors(got, want)
    print(f"\nreplay vs float64 autograd, {kinds} {g_kind}: max|grad| {want.abs().max().item():.3e}  e_max {e_max:.2e}  e_rms {e_rms:.2e}")
    assert e_max <= 1e-10 and e_rms <= 1e-10, (e_max, e_rms)


def test_oracles_run_in_float64_and_agree_with_float32(oracle_convs, alpha_beta):
    """Every constant of the two oracles follows the input's dtype: a float64 call stays float64 end to end and lands
    on the float32 result to float32 rounding."""
    from nerf_qa_amd import synth
    from oracle import adists_oracle as ao
    xn, yn = synth.frame_batch([1, 2], 40, 56)
    x, y = torch.from_numpy(xn), torch.from_numpy(yn)
    a, b = alpha_beta
    s32 = do.dists(x, y, oracle_convs, a, b)
    s64 = do.dists(x.double(), y.double(), _convs64(oracle_convs), a.double(), b.double())
    assert s32.dtype == torch.float32 and s64.dtype == torch.float64
    assert (s32.double() - s64).abs().max().item() <= 1e-5
    for kw in ({}, {"as_loss": True}, {"as_map": True}):
        a32 = ao.adists(x, y, oracle_convs, **kw)
        a64 = ao.adists(x.double(), y.double(), _convs64(oracle_convs), **kw)
        assert a32.dtype == torch.float32 and a64.dtype == torch.float64
        assert (a32.double() - a64).abs().max().item() <= 1e-4
