"""The accumulating DISTS tap gradient on its own (include/nqa.h: nqa_dists_stats_nhwc_grad_y_add;
csrc/nqa_loss_backward.hip: loss_stats_grad_y_add_kernel): gy_inout += the gy of nqa_dists_stats_nhwc_backward_from.

The contract is an equality, so the check is one: the result torch.equal's g_in + gy_existing, gy_existing from
ops.dists_stats_nhwc_backward_from(need_x=False) on the same partials.  Both sides round the same fp64 chain to float
once and then do ONE IEEE float add, which has one answer.  Also: no NaN, a second call on a fresh copy gives the same
bits, and pair 0 does not change when pair 1's upstream is 2^12 times larger.

Maps: random post-ReLU maps (exact zeros from the clamp) with dead channels; g_in random and 0 where y <= 0, as a masked
producer (nqa_adists_ts_backward with mask = 1) leaves it.  Upstream: columns of a (B, 1475) tensor at a nonzero offset,
so g_stride = 1475.  Shapes (C, H, W): one pixel; a pixel count that fills neither a block nor a thread row (35 pixels
against PL = 64 lanes of 8 pixels at C = 16); a real tap, several blocks (64, 40, 56); a ragged one (128, 33, 47: 1551
pixels, 8 lanes); the narrowest layout, one pixel lane of 256 channel groups (1024, 3, 5)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(16, 1, 1), (16, 5, 7), (64, 40, 56), (128, 33, 47), (1024, 3, 5)]
B, CTOT = 2, 1475


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _case(c, h, w, dev):
    gen = torch.Generator().manual_seed(3000 * c + 10 * h + w)
    tx = torch.randn(B, h, w, c, generator=gen).clamp_min(0)
    ty = (tx + 0.3 * torch.randn(B, h, w, c, generator=gen)).clamp_min(0)
    tx[..., 3] = 0          # dead in x
    ty[..., 7] = 0          # dead in y
    tx[..., 9] = 0          # dead in both
    ty[..., 9] = 0
    tx[1, ..., 11] = 0      # dead in both, pair 1 only
    ty[1, ..., 11] = 0
    g_in = torch.randn(B, h, w, c, generator=gen) * (ty > 0)
    col = 5 if c == 1024 else 67
    g1, g2 = torch.randn(B, CTOT, generator=gen), torch.randn(B, CTOT, generator=gen)
    return tuple(t.to(dev) for t in (tx, ty, g_in, g1, g2)) + (col,)


@pytest.mark.parametrize("c,h,w", SHAPES, ids=[f"C{c}-{h}x{w}" for c, h, w in SHAPES])
def test_accumulated_gradient_is_the_existing_gradient_plus_one_float_add(c, h, w, dev):
    from nerf_qa_amd import ops
    tx, ty, g_in, g1, g2, col = _case(c, h, w, dev)
    assert bool((ty == 0).any()) and g1.shape[1] == CTOT and col > 0
    s1, s2 = torch.empty(B, c, device=dev), torch.empty(B, c, device=dev)
    part = ops.dists_stats_target(tx, ty, s1, s2, 0)
    kept = part.clone()
    _, gy_existing = ops.dists_stats_nhwc_backward_from(tx, ty, part, g1, g2, col, need_x=False)
    want = g_in + gy_existing
    acc = g_in.clone()
    got = ops.dists_stats_nhwc_grad_y_add(tx, ty, part, g1, g2, col, acc)
    assert got.data_ptr() == acc.data_ptr()
    assert not torch.isnan(got).any() and not torch.isnan(want).any() and torch.isfinite(got).all()
    assert h * w == 1 or gy_existing.abs().max().item() > 0
    assert torch.equal(got, want)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))  # (and the sign of every zero)
    assert bool((got[ty <= 0] == 0).all())  # the mask holds in the sum
    assert torch.equal(part, kept)  # the partials are read, never written
    # repeatable
    again = ops.dists_stats_nhwc_grad_y_add(tx, ty, part, g1, g2, col, g_in.clone())
    assert torch.equal(again.view(torch.int32), got.view(torch.int32))
    # pair 0 does not read pair 1's numbers
    h1, h2 = g1.clone(), g2.clone()
    h1[1] *= 4096.0
    h2[1] *= 4096.0
    other = ops.dists_stats_nhwc_grad_y_add(tx, ty, part, h1, h2, col, g_in.clone())
    assert torch.equal(other[0].view(torch.int32), got[0].view(torch.int32))
    assert h * w == 1 or not torch.equal(other[1], got[1])


def test_wrapper_refuses_what_is_not_a_gradient_of_the_tap(dev):
    from nerf_qa_amd import ops
    tx, ty, g_in, g1, g2, col = _case(16, 5, 7, dev)
    s1, s2 = torch.empty(B, 16, device=dev), torch.empty(B, 16, device=dev)
    part = ops.dists_stats_target(tx, ty, s1, s2, 0)
    with pytest.raises(ValueError):
        ops.dists_stats_nhwc_grad_y_add(tx, ty, part, g1, g2, CTOT - 8, g_in.clone())  # the columns run off the row
    with pytest.raises(AssertionError):
        ops.dists_stats_nhwc_grad_y_add(tx, ty, part, g1, g2, col, g_in[:1].clone())
    with pytest.raises(AssertionError):
        ops.dists_stats_nhwc_grad_y_add(tx, ty, part, g1, g2, col, g_in.permute(0, 3, 1, 2))
