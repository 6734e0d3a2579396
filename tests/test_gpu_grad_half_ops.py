"""Each kernel of the half gradient chain (grad_precision="f16") on its own, through its entry point of include/nqa.h.

nqa_conv3x3_half against a float64 3x3 cross-correlation (padding 1) of the SAME half operands.  Per element
    |got - ref| <= 2^-11 |ref| + 2^-24 + 2 (9 cin) 2^-24 A,      A = the same convolution of |in| with |w|:
one half rounding of the output, the half subnormal step, and float32 accumulation of 9 cin products (each exact in
float32: a product of two halves has 22 significant bits) with a factor 2 for the MFMA's internal order.  Derived, not fitted.
The shapes cover both tile widths (W <= 16: 16-wide tiles), one pixel, ragged edges past one 32-wide tile, the 64-channel
tiles on the 32x32x16 MFMA (cout 64) and the 128-channel ones on 16x16x32 (cout 256, 512), 2 .. 16 input chunks.

The mask + encode kernel, the exponent reduction, the pool seam and conv1_1's step are exact statements: torch.equal
to the defining expression, or to the float entry point on the halves converted to float."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---- nqa_conv3x3_half ---------------------------------------------------------------------------------------------------
def _octave_inputs(shape, seed):
    """Signed halves in [-16, 16] spread evenly over 20 octaves: 16 * 2^-20 = 1.5e-5 up, so the lowest two octaves are
    half subnormals (below 2^-14)."""
    gen = torch.Generator().manual_seed(seed)
    mag = 16.0 * torch.exp2(-20.0 * torch.rand(shape, generator=gen, dtype=torch.float64))
    sign = torch.where(torch.rand(shape, generator=gen) < 0.5, -1.0, 1.0).double()
    x = (mag * sign).to(torch.float16)
    assert int(((x != 0) & (x.abs().float() < 2.0 ** -14)).sum()) > 0 or x.numel() < 200
    return x


@functools.lru_cache(maxsize=None)
def _layer(cin, cout):
    """(weights rounded to half as float64 OIHW, the packed blob on the device)."""
    from nerf_qa_amd import ops
    gen = torch.Generator().manual_seed(cin * 1000 + cout)
    w = torch.randn((cout, cin, 3, 3), generator=gen) * 0.03
    return w.to(torch.float16).double(), ops.pack_conv_half(w).to(DEV)


@pytest.mark.parametrize("h,w", [(1, 1), (5, 7), (3, 40), (17, 33)])
@pytest.mark.parametrize("cin,cout", [(64, 64), (128, 64), (512, 256), (512, 512)])
def test_conv3x3_half_against_float64_on_the_same_halves(cin, cout, h, w):
    from nerf_qa_amd import ops
    n = 2
    w64, blob = _layer(cin, cout)
    x = _octave_inputs((n, h, w, cin), cin + cout + h * w)
    xd = x.to(DEV)
    got = ops.conv3x3_half(xd, blob, cout)
    again = ops.conv3x3_half(xd, blob, cout)
    zero = ops.conv3x3_half(torch.zeros_like(xd), blob, cout)
    torch.cuda.synchronize()
    assert got.dtype == torch.float16 and got.shape == (n, h, w, cout)
    assert torch.equal(got.view(torch.int16), again.view(torch.int16))      # bit-equal
    assert not zero.view(torch.int16).bitwise_and(0x7fff).any()             # all zero (either sign)
    x64 = x.double().permute(0, 3, 1, 2)
    ref = torch.nn.functional.conv2d(x64, w64, padding=1).permute(0, 2, 3, 1)
    a = torch.nn.functional.conv2d(x64.abs(), w64.abs(), padding=1).permute(0, 2, 3, 1)
    g = got.cpu().double()
    assert not torch.isnan(g).any()
    in_range = ref.abs() < 65504.0
    assert in_range.all() and not torch.isinf(g[in_range]).any()
    bound = 2.0 ** -11 * ref.abs() + 2.0 ** -24 + 2.0 * (9 * cin) * 2.0 ** -24 * a
    err = (g - ref).abs()
    worst = (err / bound).max().item()
    print(f"\n[conv3x3_half] {cin}->{cout} {h}x{w}: max|ref| {ref.abs().max().item():.3g}  max err/bound {worst:.3f}  "
          f"max err/|ref|max {err.max().item() / ref.abs().max().item():.2e}")
    assert (err <= bound).all(), worst


# ---- nqa_relu_mask_f16_scaled -------------------------------------------------------------------------------------------
def _mask_case(n, pix, c, ks, g_half, seed):
    gen = torch.Generator().manual_seed(seed)
    shape = (n, pix, 1, c)
    act = torch.relu(torch.randn(shape, generator=gen))  # about half of the entries exactly dead
    g = torch.randn(shape, generator=gen) * torch.exp2(torch.randint(-24, 5, shape, generator=gen).float())
    for i, k in enumerate(ks):
        flat = g[i].view(-1)
        if not g_half:
            flat[0::7] = 1.0 + 2.0 ** -11              # exact round-to-even ties of the float -> half conversion:
            flat[1::7] = 1.0 + 3 * 2.0 ** -11          # down to 1, and up to 1 + 2^-9
            flat[2::7] = -(2.0 ** -14) * (1.0 + 2.0 ** -11)
            flat[3::7] = 3.3e-6                        # results in the half subnormal range at k = 0 and k = 7
        elif k == -30:                                 # halves scale exactly unless the result is subnormal:
            flat[0::7] = 32768.0 * (1.0 + 2.0 ** -10)  # 2^-15 (1 + 2^-10) = 512.5 subnormal steps, a tie (-> 512)
            flat[1::7] = -32768.0 * (1.0 + 3 * 2.0 ** -10)  # 513.5 steps (-> 514)
            flat[2::7] = 60000.0                       # near the top of the half range
        else:
            flat[0::7] = 2.0 ** -24                    # the smallest subnormal half
    if g_half:
        g = g.to(torch.float16)
    huge = 60000.0 if g_half else 1e30
    g = torch.where(act > 0, g, torch.full_like(g, huge))  # dead entries: exactly 0 whatever stands there
    return g.contiguous(), act.contiguous()


@pytest.mark.parametrize("act_split", [False, True], ids=["act-float", "act-split16"])
@pytest.mark.parametrize("g_half", [False, True], ids=["g-float", "g-half"])
@pytest.mark.parametrize("n,pix,c,ks", [(2, 1, 64, (-30, 7)), (3, 35, 128, (-30, 0, 7)), (2, 561, 512, (0, 7))])
def test_relu_mask_f16_scaled_is_the_defining_expression(n, pix, c, ks, g_half, act_split):
    from nerf_qa_amd import ops
    g, act = _mask_case(n, pix, c, ks, g_half, n * pix + c)
    g, act = g.to(DEV), act.to(DEV)
    k = torch.tensor(ks, dtype=torch.int32, device=DEV)
    if act_split:
        act_in = ops.split16_encode(act)
        act_val = ops.split16_decode(act_in)
    else:
        act_in = act_val = act
    got = ops.relu_mask_f16_scaled(g, act_in, act_split, k)
    want = (torch.ldexp(g.float(), k.view(n, 1, 1, 1)) * (act_val > 0)).half()
    torch.cuda.synchronize()
    assert got.dtype == torch.float16 and got.shape == g.shape
    assert torch.isfinite(want).all() and int((want != 0).sum()) > 0
    assert torch.equal(got, want)
    dead = ~(act_val > 0)
    assert int(dead.sum()) > 0 and not got[dead].view(torch.int16).bitwise_and(0x7fff).any()
    if not g_half and 0 in ks:
        sub = (want != 0) & (want.abs().float() < 2.0 ** -14)
        assert int(sub.sum()) > 0  # the subnormal range is reached


# ---- nqa_grad_exponent_half ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g_half", [False, True], ids=["g-float", "g-half"])
@pytest.mark.parametrize("per", [64, 4 * 35 * 128])
def test_grad_exponent_half_is_the_float_exponent_minus_four(per, g_half):
    from nerf_qa_amd import ops
    gen = torch.Generator().manual_seed(per)
    base = torch.randn((3, per), generator=gen)
    for scales, special in (((3e-7, 1.0, 5e3), None), ((0.02, 1.0, 7.0), "zero+inf")):
        g = base * torch.tensor(scales).view(3, 1)
        if special:
            g[1] = 0.0
            g[2, per // 3] = float("inf")
        g = (g.to(torch.float16) if g_half else g).to(DEV).contiguous()
        k = torch.full((3,), 99, dtype=torch.int32, device=DEV)
        start = torch.tensor([5, -3, 0], dtype=torch.int32, device=DEV)
        K = start.clone()
        ops.grad_exponent_half(g, k, K)
        kf = torch.empty(3, dtype=torch.int32, device=DEV)
        ops.grad_exponent(g.float().contiguous(), kf, None)
        torch.cuda.synchronize()
        if special:
            assert k[0].item() == kf[0].item() - 4 and k[1].item() == 0 and k[2].item() == 0, (k, kf)
        else:
            assert torch.equal(k, kf - 4), (k, kf)
            mx = g.float().abs().amax(dim=1).double() * torch.exp2(k.double())
            assert ((mx >= 8) & (mx < 16)).all(), mx
        assert torch.equal(K, start + k)
        ops.grad_exponent_half(g, k, K)  # the running total accumulates
        ops.grad_exponent_half(g, k, None)  # and may be left out
        torch.cuda.synchronize()
        assert torch.equal(K, start + 2 * k)


# ---- the pool seam and conv1_1's step: the float entry points on the halves converted to float, bit for bit ---------------
@pytest.mark.parametrize("c", [64, 256])
@pytest.mark.parametrize("h,w", [(1, 1), (5, 7), (33, 47)])
def test_l2pool_backward_scaled_half_equals_the_float_form(h, w, c):
    from nerf_qa_amd import ops
    n = 2
    gen = torch.Generator().manual_seed(h * w + c)
    tap = torch.relu(torch.randn((n, h, w, c), generator=gen)).to(DEV)
    g_tap = (torch.randn((n, h, w, c), generator=gen) * 1e-6).to(DEV)
    gp = (torch.randn((n, (h + 1) // 2, (w + 1) // 2, c), generator=gen) * 9.0).to(torch.float16).to(DEV)
    K = torch.tensor([17, 21], dtype=torch.int32, device=DEV)
    got = ops.l2pool_backward_scaled(tap, gp, g_tap, K)
    want = ops.l2pool_backward_scaled(tap, gp.float(), g_tap, K)
    torch.cuda.synchronize()
    assert torch.isfinite(want).all() and want.abs().max().item() > 0
    assert torch.equal(got, want)


@pytest.mark.parametrize("masked", [True, False], ids=["mask", "no-mask"])
@pytest.mark.parametrize("h,w", [(1, 1), (5, 7), (33, 47)])
def test_conv1_1_backward_scaled_half_equals_the_float_form(h, w, masked):
    from nerf_qa_amd import ops
    n = 2
    gen = torch.Generator().manual_seed(h * w)
    g = (torch.randn((n, h, w, 64), generator=gen) * 0.3).to(torch.float16).to(DEV)
    act0 = ops.split16_encode(torch.relu(torch.randn((n, h, w, 64), generator=gen)).to(DEV)) if masked else None
    w0 = (torch.randn((64, 3, 3, 3), generator=gen) * 0.1).to(DEV)
    k = torch.tensor([4, -2], dtype=torch.int32, device=DEV)
    K = torch.tensor([30, 11], dtype=torch.int32, device=DEV)
    got = ops.conv1_1_backward_scaled(g, act0, w0, k, K)
    want = ops.conv1_1_backward_scaled(g.float(), act0, w0, k, K)
    torch.cuda.synchronize()
    assert got.shape == (n, 3, h, w) and torch.isfinite(want).all() and want.abs().max().item() > 0
    assert torch.equal(got, want)
