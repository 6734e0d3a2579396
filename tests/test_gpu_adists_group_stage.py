"""The group instances of the A-DISTS window pass and the group form of its probability chain (include/nqa.h:
nqa_adists_window_stage_group, nqa_adists_chain_group) against the pairwise entry points on the same data, BIT FOR BIT.

A pair of a group is computed by the pairwise kernel's own row body, from reference r = b // K where the pairwise call
reads x image b; the chain's probability part runs once per reference and the K renders' sums are taken against it in
the pairwise kernel's order.  So the pairwise calls on `ref.repeat_interleave(K)` / `gamma.repeat_interleave(K)` must give
the same bits: tw, sw and d for every pair, gamma and ps_prod of reference r those of pair r * K.  No tolerance anywhere.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

# (R, K, H, W, forced strip): one 64-row group with a ragged 4-column block; two strips, the first flushing two groups;
# the global branch
WINDOW_SHAPES = [(2, 3, 41, 37, 0), (1, 2, 150, 30, 70), (2, 2, 19, 25, 0)]
WINDOW_MODES = [(3, "f32"), (64, "f32"), (128, "f32"), (64, "f16")]
CHAIN_FRAMES = [(2, 3, 130, 95), (2, 2, 33, 47), (3, 2, 17, 23)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _stage_inputs(R, K, H, W, C, prec, dev):
    """Reference maps (R), render maps (R*K), q (8, R*K, C) as the preparation kernel would leave it for these maps and
    wgt (R, C): non-negative maps with dead spots, like taps behind a ReLU."""
    g = torch.Generator().manual_seed(1000 * C + 10 * H + R + K)
    B = R * K
    x = torch.relu(torch.randn(R, C, H, W, generator=g) + 0.3)
    y = torch.relu(x.repeat_interleave(K, 0) + 0.4 * torch.randn(B, C, H, W, generator=g))
    if prec == "f16":
        x, y = x.half(), y.half()
    xd, yd = x.double().repeat_interleave(K, 0).flatten(2), y.double().flatten(2)
    mx, my = xd.mean(2), yd.mean(2)
    q = torch.stack([1 / xd.norm(dim=2).clamp_min(1e-12), 1 / yd.norm(dim=2).clamp_min(1e-12), xd.sum(2), mx, my,
                     (xd * xd).mean(2) - mx * mx, (yd * yd).mean(2) - my * my, (xd * yd).mean(2) - mx * my]).float()
    wgt = torch.rand(R, C, generator=g)
    wgt = wgt / wgt.sum(1, keepdim=True)
    if C != 3:  # NHWC taps in the mode's storage type; the image planes stay NCHW float
        x, y = x.permute(0, 2, 3, 1), y.permute(0, 2, 3, 1)
    return [t.contiguous().to(dev) for t in (x, y, q, wgt)]


@pytest.mark.parametrize("C,prec", WINDOW_MODES, ids=lambda v: str(v))
@pytest.mark.parametrize("shape", WINDOW_SHAPES, ids=lambda s: "R%dK%d_%dx%d_strip%d" % s)
def test_window_stage_group_is_the_pairwise_stage_bit_for_bit(shape, C, prec, dev):
    from nerf_qa_amd import ops
    R, K, H, W, strip = shape
    x, y, q, wgt = _stage_inputs(R, K, H, W, C, prec, dev)
    gg, gt, gs = ops.adists_window_stage_group(x, y, q, wgt, prec, strip)
    pg, pt, ps = ops.adists_window_stage(x.repeat_interleave(K, 0).contiguous(), y, q,
                                         wgt.repeat_interleave(K, 0).contiguous(), prec, strip)
    windowed = H >= 21 and W >= 21
    mh, mw = (H - 20, W - 20) if windowed else (1, 1)
    assert gg.shape == (R, mh, mw) and gt.shape == gs.shape == (R * K, mh, mw)
    assert torch.isfinite(gt).all() and torch.isfinite(gs).all() and torch.isfinite(gg).all()
    assert gt.abs().max().item() > 0 and not torch.equal(gt[0], gt[-1])  # (the maps hold something, and pairs differ)
    assert torch.equal(gt, pt) and torch.equal(gs, ps)
    assert torch.equal(gg, pg[::K])
    if windowed and C >= 64 and prec == "f32":  # the LDS kernel ran, on the grid the shape list promises
        nbx, nby, st = ops.adists_window_grid(R * K, H, W, C, prec, strip)
        assert (nbx, nby, st) == ((mw + 3) // 4, -(-mh // (strip or st)), strip or st)
        if strip:
            assert nby == 2 and strip > 64


@pytest.mark.parametrize("frame", CHAIN_FRAMES, ids=lambda s: "R%dK%d_%dx%d" % s)
def test_chain_group_is_the_pairwise_chain_bit_for_bit(frame, dev):
    from nerf_qa_amd import ops
    R, K, H, W = frame
    dims, nwin = ops.adists_chain_dims(H, W)
    assert nwin == {(130, 95): 4, (33, 47): 2, (17, 23): 0}[(H, W)]
    g = torch.Generator().manual_seed(H * W + K)
    gamma = [(0.05 + torch.rand((R,) + d, generator=g)).to(dev) for d in dims]
    tw = [torch.rand((R * K,) + d, generator=g).to(dev) for d in dims]
    sw = [(2 * torch.rand((R * K,) + d, generator=g) - 0.5).to(dev) for d in dims]
    ps_g, d_g = ops.adists_chain_group(gamma, tw, sw, H, W)
    ps_p, d_p, _ = ops.adists_chain([t.repeat_interleave(K, 0).contiguous() for t in gamma], tw, sw, H, W, with_map=False)
    assert d_g.shape == (R * K,) and torch.isfinite(d_g).all() and d_g.unique().numel() == R * K
    assert torch.equal(d_g, d_p)
    for k in range(6):
        assert ps_g[k].shape == (R,) + dims[k]
        assert torch.equal(ps_g[k], ps_p[k][::K]), k
