"""One stage of the A-DISTS head's backward towards y for a window of n taps (ops.adists_ts_backward(window=n),
nqa_adists_ts_backward_n): the coefficient, dot, fold, apply and global kernels of csrc/nqa_adists_backward.hip around the
generic window moments of csrc/nqa_window_moments_n.hip.

Reference: float64 torch autograd of the stage's D term on the CPU over the same float32 maps (the slice form of
head._window_mean with head.gauss_1d(n); plain means in the global branch).  Yardstick: the SAME expression in float32 on
the CPU against that float64 run; the HIP gradient's max and rms error (grad_replay.errors) may be
grad_replay.bound(yardstick), exactly as tests/test_gpu_adists_loss_y.py holds the 21-tap stage.  Every output sits
NaN-filled between guard fences and the workspace is handed out NaN-filled (tests/poison.py)."""
import pytest
import torch
import torch.nn.functional as F

import window_moments_n_refs as R

pytestmark = pytest.mark.gpu

EPS = 1e-6


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def stage_d(X, Y, w, p, n):
    """D_b's term of one stage (ADISTS.py:165-191) with a window of n taps, as head.adists_d forms it: (B,)."""
    from nerf_qa_amd.ADISTS import head
    fx, fy = F.normalize(X, dim=(2, 3)), F.normalize(Y, dim=(2, 3))
    if X.shape[2] >= n and X.shape[3] >= n:
        g = head.gauss_1d(n, X)
        xm, ym = head._window_mean(fx, g), head._window_mean(fy, g)
        xv = head._window_mean(fx * fx, g) - xm * xm
        yv = head._window_mean(fy * fy, g) - ym * ym
        cov = head._window_mean(fx * fy, g) - xm * ym
    else:
        xm, ym = fx.mean(dim=(2, 3), keepdim=True), fy.mean(dim=(2, 3), keepdim=True)
        xv = ((fx - xm) ** 2).mean(dim=(2, 3), keepdim=True)
        yv = ((fy - ym) ** 2).mean(dim=(2, 3), keepdim=True)
        cov = (fx * fy).mean(dim=(2, 3), keepdim=True) - xm * ym
    t = (2 * xm * ym + EPS) / (xm * xm + ym * ym + EPS)
    s = (2 * cov + EPS) / (xv + yv + EPS)
    ps = p.unsqueeze(1)
    d_map = (((1 - ps) * t + ps * s) * w[:, :, None, None]).sum(dim=1, keepdim=True)
    return d_map.mean(dim=(2, 3)).sum(dim=1)


def stage_grad(X, Y, w, p, u, mask, n, dtype):
    X, w, p, u = (t.detach().cpu().to(dtype) for t in (X, w, p, u))
    Y = Y.detach().cpu().to(dtype).requires_grad_()
    (g,) = torch.autograd.grad((u * stage_d(X, Y, w, p, n)).sum(), Y)
    return g * (Y > 0) if mask else g


def stage_q(X, Y):
    """q (8,B,C) float32 of a stage on its own: rows 0, 1 = 1 / max(||.||, 1e-12), rows 3..7 = mean_x mean_y var_x var_y
    cov (population) of the raw maps, formed in float64 and rounded once."""
    xd, yd = X.double(), Y.double()
    b, c = X.shape[:2]
    q = torch.zeros(8, b, c, dtype=torch.float64)
    q[0] = 1 / xd.flatten(2).norm(dim=2).clamp_min(1e-12)
    q[1] = 1 / yd.flatten(2).norm(dim=2).clamp_min(1e-12)
    mx, my = xd.mean(dim=(2, 3)), yd.mean(dim=(2, 3))
    q[3], q[4] = mx, my
    q[5] = (xd * xd).mean(dim=(2, 3)) - mx * mx
    q[6] = (yd * yd).mean(dim=(2, 3)) - my * my
    q[7] = (xd * yd).mean(dim=(2, 3)) - mx * my
    return q.float()


def relu_maps(shape, gen):
    return torch.rand(shape, generator=gen).sub_(0.3).clamp_(min=0)


def _run(args, dev, shape, nhwc, **kw):
    """ops.adists_ts_backward into a fenced NaN-filled output with a NaN-filled workspace."""
    import poison
    from nerf_qa_amd import ops
    b, c, h, w = shape
    out = R.Fenced((b, h, w, c) if nhwc else (b, c, h, w), dev)
    ws = poison.PoisonWorkspace(0xFF)
    got = ops.adists_ts_backward(*args, nhwc=nhwc, ws=ws, out=out.view, **kw)
    assert got.data_ptr() == out.view.data_ptr() and ws.gets == 1
    return out.check(f"stage {shape} {kw}").clone()


STAGE_CASES = [
    # (n, B, C, H, W, mask, u, special)
    (7, 2, 64, 16, 24, True, (-0.7, 0.4), "dead"),     # 16-byte rows, planar and NHWC, a dead channel of Y
    (4, 2, 3, 9, 13, False, (-0.5, -0.5), None),       # the image: no mask, an even window, the scalar path
    (33, 1, 32, 40, 56, True, (-1.0,), "deadx"),       # (n - 1) % 4 == 0: 16-byte window-mean maps; a dead channel of X
    (12, 2, 64, 11, 20, True, (-0.5, -0.25), "dead"),  # H = n - 1: the global branch
    (12, 1, 32, 12, 15, True, (-1.0,), None),          # H = n exactly: one row of windows, an even window, odd width
    (4, 2, 32, 9, 12, True, (-0.5, -1.0), "dead"),     # W % 4 == 0 with maps of 6 x 9 = 54 floats: 16-byte rows, but the
                                                       # planes of window means are no multiple of 16 bytes
    (12, 2, 64, 33, 24, True, (-0.5, -0.5), None),     # the same at 22 x 13 = 286 floats (relu2_2 of a 66 x 49 frame)
]
STAGE_IDS = ["n7-2x64x16x24", "n4-2x3x9x13_nomask", "n33-1x32x40x56", "n12-2x64x11x20_global", "n12-1x32x12x15",
             "n4-2x32x9x12_ragged_planes", "n12-2x64x33x24_ragged_planes"]


@pytest.mark.parametrize("n,b,c,h,w,mask,u,special", STAGE_CASES, ids=STAGE_IDS)
def test_stage_backward_n_against_float64_autograd(n, b, c, h, w, mask, u, special, dev):
    import grad_replay as gr
    from nerf_qa_amd import ops
    gen = torch.Generator().manual_seed(2000 + 31 * n + c + h)
    X, Y = relu_maps((b, c, h, w), gen), relu_maps((b, c, h, w), gen)
    if special == "dead":
        Y[:, 1] = 0
    if special == "deadx":
        X[:, 2] = 0
    windowed = h >= n and w >= n
    p = torch.rand((b, h - n + 1, w - n + 1) if windowed else (b, 1, 1), generator=gen)
    wgt = (torch.rand((b, c), generator=gen) + 0.5) / 1475
    u = torch.tensor(u)
    q = stage_q(X, Y)
    g64 = stage_grad(X, Y, wgt, p, u, mask, n, torch.float64)
    g32 = stage_grad(X, Y, wgt, p, u, mask, n, torch.float32)
    (ym, yr) = gr.errors(g32, g64)
    args = [t.to(dev).contiguous() for t in (X, Y, q, wgt, p, u)]
    print(f"\nstage n={n} {b}x{c}x{h}x{w} ({'windowed' if windowed else 'global'}), workspace "
          f"{ops.lib().nqa_adists_ts_backward_bytes_n(b, c, h, w, n)} bytes; yardstick max {ym:.3e} rms {yr:.3e}")
    bad, planar = [], None
    for nhwc in ((False, True) if c % 32 == 0 or not windowed else (False,)):
        got = _run(args, dev, (b, c, h, w), nhwc, mask=mask, window=n)
        assert torch.equal(got, _run(args, dev, (b, c, h, w), nhwc, mask=mask, window=n))  # bitwise repeatable
        if nhwc:
            got = got.permute(0, 3, 1, 2)
            assert torch.equal(got, planar)  # the two layouts hold the same numbers
        else:
            planar = got
        if special == "dead":
            assert (got[:, 1] == 0).all()  # exactly zero under the mask, whatever 1 / 1e-12 did upstream
        em, er = gr.errors(got, g64)
        print(f"  {'nhwc' if nhwc else 'planar'}: HIP max {em:.3e} rms {er:.3e}; bound max {gr.bound(ym):.3e} "
              f"rms {gr.bound(yr):.3e} ({em / gr.bound(ym):.2f}, {er / gr.bound(yr):.2f} of it)")
        if not (em <= gr.bound(ym) and er <= gr.bound(yr)):
            bad.append((nhwc, em, er, ym, yr))
    assert not bad, bad


def test_channel_offset_inside_a_wider_ctot_and_batch_independence(dev):
    """coff > 0 inside the 1475-wide q and wgt gives the result of the contiguous slices bit for bit; pair 0 of a batch is
    pair 0 on its own; window=21 is the default call."""
    n, b, c, h, w = 7, 2, 64, 16, 24
    gen = torch.Generator().manual_seed(78)
    X, Y = relu_maps((b, c, h, w), gen), relu_maps((b, c, h, w), gen)
    p, u = torch.rand((b, h - n + 1, w - n + 1), generator=gen), torch.tensor([-0.5, -0.25])
    q = torch.rand((8, b, 1475), generator=gen)
    wgt = torch.rand((b, 1475), generator=gen) / 1475
    q[:, :, 3:67] = stage_q(X, Y)
    X, Y, p, u, q, wgt = (t.to(dev) for t in (X, Y, p, u, q, wgt))
    full = _run((X, Y, q, wgt, p, u), dev, (b, c, h, w), True, mask=True, coff=3, window=n)
    part = _run((X, Y, q[:, :, 3:67].contiguous(), wgt[:, 3:67].contiguous(), p, u), dev, (b, c, h, w), True, mask=True,
                window=n)
    assert torch.equal(full, part)
    one = _run((X[:1].contiguous(), Y[:1].contiguous(), q[:, :1].contiguous(), wgt[:1].contiguous(), p[:1].contiguous(),
                u[:1].contiguous()), dev, (1, c, h, w), True, mask=True, coff=3, window=n)
    assert torch.equal(full[:1], one)


def test_window_21_is_the_21_tap_stage_and_bit_4096_stays_inside_the_bound(dev):
    import grad_replay as gr
    from nerf_qa_amd import ops
    n, b, c, h, w = 21, 1, 64, 30, 44
    gen = torch.Generator().manual_seed(79)
    X, Y = relu_maps((b, c, h, w), gen), relu_maps((b, c, h, w), gen)
    p, u = torch.rand((b, h - 20, w - 20), generator=gen), torch.tensor([-1.0])
    wgt = (torch.rand((b, c), generator=gen) + 0.5) / 1475
    q = stage_q(X, Y)
    g64 = stage_grad(X, Y, wgt, p, u, True, n, torch.float64)
    ym, yr = gr.errors(stage_grad(X, Y, wgt, p, u, True, n, torch.float32), g64)
    args = [t.to(dev).contiguous() for t in (X, Y, q, wgt, p, u)]
    default = ops.adists_ts_backward(*args, mask=True)
    assert torch.equal(default, _run(args, dev, (b, c, h, w), False, mask=True, window=21))
    try:
        ops.set_conv_variant(ops.DEFAULT_CONV_VARIANT | ops.CONV_MOMENTS_GENERIC)
        generic = _run(args, dev, (b, c, h, w), False, mask=True, window=21)
    finally:
        ops.set_conv_variant(ops.DEFAULT_CONV_VARIANT)
    for name, got in (("21-tap kernels", default), ("generic kernels", generic)):
        em, er = gr.errors(got, g64)
        print(f"\nstage n=21 {name}: max {em:.3e} rms {er:.3e}; bound max {gr.bound(ym):.3e} rms {gr.bound(yr):.3e}")
        assert em <= gr.bound(ym) and er <= gr.bound(yr)


def test_the_old_stage_entry_point_ignores_bit_4096(dev):
    """nqa_adists_ts_backward (no window argument) keeps the 21-tap window-moments kernels whatever the bit says: equal
    bits with and without it, and the bits of ops.adists_ts_backward(window=21) without it.  1 x 64 x 30 x 44 is the
    smallest windowed stage on the 16-byte path (10 x 24 windows)."""
    import poison
    from nerf_qa_amd import ops
    b, c, h, w = 1, 64, 30, 44
    gen = torch.Generator().manual_seed(79)
    X, Y = relu_maps((b, c, h, w), gen), relu_maps((b, c, h, w), gen)
    p, u = torch.rand((b, h - 20, w - 20), generator=gen), torch.tensor([-1.0])
    wgt = (torch.rand((b, c), generator=gen) + 0.5) / 1475
    args = [t.to(dev).contiguous() for t in (X, Y, stage_q(X, Y), wgt, p, u)]
    xd, yd, qd, wd, pd, ud = args

    def old():
        out = R.Fenced((b, c, h, w), dev)
        buf = poison.PoisonWorkspace(0xFF).get(ops.lib().nqa_adists_ts_backward_bytes(b, c, h, w), dev)
        ops._call(dev, ops.lib().nqa_adists_ts_backward, ops.ptr(xd), ops.ptr(yd), b, c, h, w, ops.ptr(qd), ops.ptr(wd), c, 0,
                  ops.ptr(pd), ops.ptr(ud), 1, 0, ops.ptr(buf), buf.numel(), ops.ptr(out.view), ops.stream_ptr(dev))
        return out.check("old stage backward").clone()
    try:
        ops.set_conv_variant(ops.DEFAULT_CONV_VARIANT | ops.CONV_MOMENTS_GENERIC)
        with_bit = old()
    finally:
        ops.set_conv_variant(ops.DEFAULT_CONV_VARIANT)
    without = old()
    assert torch.equal(with_bit, without)
    assert torch.equal(without, _run(args, dev, (b, c, h, w), False, mask=True, window=21))
