"""A-DISTS as a loss with the gradient on y alone: the one-sided HIP backward (csrc/nqa_adists_backward.hip,
ops.adists_ts_backward, autograd.adists_backward_y / AdistsLossY, ADISTS(loss_head="auto")).

Stage and head level: the reference is float64 torch autograd on the CPU over the same float32 maps (the slice form of
head._window_mean; plain means in the global branch); the yardstick is the SAME expression evaluated in float32 on the
CPU against that float64 run, and the HIP gradient's max and rms error (grad_replay.errors) may be
grad_replay.bound(yardstick): HIP_FACTOR 8 with the 1e-6 floor, the project's fixed rule for another summation order.
Module level: float64 autograd over the CPU oracle with the bounds of test_gpu_backward._compare_grads."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CHNS = (3, 64, 128, 256, 512, 512)
OFFS = (0, 3, 67, 195, 451, 963)
EPS = 1e-6


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ---- the stage's D term in torch (any dtype, CPU) ------------------------------------------------------------------
def stage_d(X, Y, w, p):
    """D_b's term of one stage (ADISTS.py:165-191) from raw maps X, Y (B,C,H,W), channel weights w (B,C) and the stage's
    probability map p (B,mh,mw), as head.adists_d forms it: (B,)."""
    from nerf_qa_amd.ADISTS import head
    fx, fy = F.normalize(X, dim=(2, 3)), F.normalize(Y, dim=(2, 3))
    if X.shape[2] >= 21 and X.shape[3] >= 21:
        g = head.gauss_1d(21, X)
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


def stage_grad(X, Y, w, p, u, mask, dtype):
    """d(sum_b u_b D_b)/dY in `dtype` on the CPU, times the ReLU mask of Y when asked."""
    X, w, p, u = (t.detach().cpu().to(dtype) for t in (X, w, p, u))
    Y = Y.detach().cpu().to(dtype).requires_grad_()
    (g,) = torch.autograd.grad((u * stage_d(X, Y, w, p)).sum(), Y)
    return g * (Y > 0) if mask else g


def stage_q(X, Y):
    """q (8,B,C) float32 for a stage on its own (ctot = C): rows 0, 1 = 1 / max(||.||, 1e-12) and rows 3..7 = mean_x
    mean_y var_x var_y cov (population) of the raw maps, all formed in float64 and rounded once."""
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
    """rand - 0.3 clamped at 0, as the head tests use."""
    return torch.rand(shape, generator=gen).sub_(0.3).clamp_(min=0)


STAGE_CASES = [
    # (B, C, H, W, mask, u, special)
    (2, 3, 21, 21, False, (-0.5, -0.5), None),          # one window, the image stage: no mask
    (1, 64, 22, 37, True, (-1.0,), "dead"),             # odd width: the scalar path; one dead channel of Y
    (2, 64, 45, 85, True, (-0.7, 0.4), "deadx"),        # crosses the moments kernels' 24 x 64 tiles; two different u_b;
                                                        # a dead channel of X beside a live one of Y (1e12-sized g4)
    (1, 128, 21, 40, True, (-1.0,), "same"),            # H exactly 21, W % 4 == 0: the 16-byte path; X == Y
    (2, 512, 13, 17, True, (-0.5, -0.25), "dead"),      # global branch
    (1, 512, 3, 4, True, (-1.0,), None),                # global branch, the deepest map of a small frame
    (1, 64, 96, 112, True, (-1.0,), "dead"),            # 10 752 elements per plane: three blocks of the dot product
    (1, 3, 40, 56, False, (-1.0,), None),               # planar output of a windowed stage on the 16-byte path
    (1, 64, 40, 56, True, (-1.0,), "close"),            # a render close to the frame: the X - Y form of the passes
]
STAGE_IDS = ["2x3x21x21_nomask", "1x64x22x37", "2x64x45x85", "1x128x21x40_same", "2x512x13x17_global", "1x512x3x4_global",
             "1x64x96x112", "1x3x40x56_nomask", "1x64x40x56_close"]


def _check_against_yardstick(name, got, g32, g64):
    import grad_replay as gr
    (em, er), (ym, yr) = gr.errors(got, g64), gr.errors(g32, g64)
    print(f"  {name}: HIP max {em:.3e} rms {er:.3e}; yardstick max {ym:.3e} rms {yr:.3e}; "
          f"bound max {gr.bound(ym):.3e} rms {gr.bound(yr):.3e}")
    assert torch.isfinite(got).all(), name
    return [] if em <= gr.bound(ym) and er <= gr.bound(yr) else [(name, em, er, ym, yr)]


@pytest.mark.parametrize("b,c,h,w,mask,u,special", STAGE_CASES, ids=STAGE_IDS)
def test_stage_backward_against_float64_autograd(b, c, h, w, mask, u, special, dev):
    from nerf_qa_amd import ops
    gen = torch.Generator().manual_seed(1000 + c + h)
    X = relu_maps((b, c, h, w), gen)
    Y = X.clone() if special == "same" else relu_maps((b, c, h, w), gen)
    if special == "dead":
        Y[:, 1] = 0
    if special == "deadx":
        X[:, 2] = 0
    if special == "close":
        Y = (X + 0.02 * torch.randn(X.shape, generator=gen)).clamp_(min=0)
    windowed = h >= 21 and w >= 21
    p = torch.rand((b, h - 20, w - 20) if windowed else (b, 1, 1), generator=gen)
    wgt = (torch.rand((b, c), generator=gen) + 0.5) / 1475
    u = torch.tensor(u)
    q = stage_q(X, Y)
    g64 = stage_grad(X, Y, wgt, p, u, mask, torch.float64)
    g32 = stage_grad(X, Y, wgt, p, u, mask, torch.float32)
    args = [t.to(dev).contiguous() for t in (X, Y, q, wgt, p, u)]
    print(f"\nstage {b}x{c}x{h}x{w} ({'windowed' if windowed else 'global'}), workspace "
          f"{ops.lib().nqa_adists_ts_backward_bytes(b, c, h, w)} bytes")
    bad = []
    layouts = (False, True) if c % 32 == 0 or not windowed else (False,)
    for nhwc in layouts:
        got = ops.adists_ts_backward(*args, mask=mask, nhwc=nhwc)
        again = ops.adists_ts_backward(*args, mask=mask, nhwc=nhwc)
        assert torch.equal(got, again)  # bitwise repeatable
        if nhwc:
            assert got.shape == (b, h, w, c)
            got = got.permute(0, 3, 1, 2)
            assert torch.equal(got, planar)  # the two layouts hold the same numbers
        else:
            planar = got
        if special == "dead":
            assert (got[:, 1] == 0).all()  # exactly zero under the mask, whatever 1 / 1e-12 did upstream
        bad += _check_against_yardstick("nhwc" if nhwc else "planar", got.cpu(), g32, g64)
    assert not bad, bad


def test_stage_backward_with_channel_offset_and_batch_independence(dev):
    """The forward's ctot / coff convention: the stage's channels inside the 1475-wide q and wgt give the result of the
    contiguous slices, bit for bit; and pair 0 of a batch is pair 0 on its own."""
    from nerf_qa_amd import ops
    gen = torch.Generator().manual_seed(77)
    b, c, h, w = 2, 64, 30, 44
    X, Y = relu_maps((b, c, h, w), gen), relu_maps((b, c, h, w), gen)
    p, u = torch.rand((b, h - 20, w - 20), generator=gen), torch.tensor([-0.5, -0.25])
    q = torch.rand((8, b, 1475), generator=gen)
    wgt = torch.rand((b, 1475), generator=gen) / 1475
    q[:, :, 3:67] = stage_q(X, Y)
    X, Y, p, u, q, wgt = (t.to(dev) for t in (X, Y, p, u, q, wgt))
    full = ops.adists_ts_backward(X, Y, q, wgt, p, u, mask=True, coff=3, nhwc=True)
    part = ops.adists_ts_backward(X, Y, q[:, :, 3:67].contiguous(), wgt[:, 3:67].contiguous(), p, u, mask=True, nhwc=True)
    assert torch.equal(full, part)
    one = ops.adists_ts_backward(X[:1].contiguous(), Y[:1].contiguous(), q[:, :1].contiguous(), wgt[:1].contiguous(),
                                 p[:1].contiguous(), u[:1].contiguous(), mask=True, coff=3, nhwc=True)
    assert torch.equal(full[:1], one)


# ---- head level ---------------------------------------------------------------------------------------------------
def _hip_head(m, x, y, fx, fy):
    """(six y-side gradients of 1 - mean(D) as NCHW, the loss value) from the staged HIP entries and the new stage
    backward, on the float32 NCHW taps fx, fy (image first)."""
    from nerf_qa_amd import ops
    dev, b = x.device, x.shape[0]
    h, w = x.shape[-2:]
    nhwc = [torch.cat([a, c]).permute(0, 2, 3, 1).contiguous() for a, c in zip(fx[1:], fy[1:])]
    q, wgt = ops.adists_front(x, y, nhwc, "f32s")
    gam, tw, sw, off = [], [], [], 0
    for k, c in enumerate(CHNS):
        a, bb = (x, y) if k == 0 else (nhwc[k - 1][:b].contiguous(), nhwc[k - 1][b:].contiguous())
        g, t, s = ops.adists_window_stage(a, bb, q[:, :, off:off + c].contiguous(), wgt[:, off:off + c].contiguous(), "f32s")
        gam.append(g), tw.append(t), sw.append(s)
        off += c
    ps, d, _ = ops.adists_chain(gam, tw, sw, h, w, with_map=False)
    u = torch.full((b,), -1.0 / b, device=dev)
    grads = [ops.adists_ts_backward(fx[k], fy[k], q, wgt, ps[k], u, mask=False, coff=OFFS[k]) for k in range(6)]
    return grads, (1 - d.mean()).item()


@pytest.mark.parametrize("h,w", [(96, 112), (64, 80)])
def test_head_y_gradients_against_float64_head(h, w, dev):
    """1 - mean(D) on fixed float32 taps, gradients towards y's six maps (no ReLU mask: the taps are leaves here, as in
    test_head_gradients_against_float64_head): x's ps_prod, wgt and q from the staged HIP entries, the new stage
    backward against head.adists_d in float64 on the CPU.  Measured: the taps at 2e-8 .. 2.6e-6; the image map is the
    tight one, rms 1.15e-3 at 64x80 (yardstick 1.5e-4, bound 1.20e-3) and 7.7e-4 at 96x112 (yardstick 4.6e-4): on the
    flat white background S = eps / eps and every upstream is 1 / eps-sized."""
    from nerf_qa_amd import synth
    from nerf_qa_amd.ADISTS import ADISTS, head
    m = ADISTS(vgg16_path="synth:1234").to(dev).eval()
    xn, yn = synth.frame_batch([21, 22], h, w, ["nerf_white", "nerf_float"])
    x, y = torch.from_numpy(xn).to(dev), torch.from_numpy(yn).to(dev)
    with torch.no_grad():
        fx = [t.float().contiguous() for t in m.forward_once(x)]
        fy = [t.float().contiguous() for t in m.forward_once(y)]

    def run(dtype):
        ax = [t.detach().cpu().to(dtype) for t in fx]
        ay = [t.detach().cpu().to(dtype).requires_grad_() for t in fy]
        loss = 1 - head.adists_d(ax, ay, 21, window_impl="slices").mean()
        return loss.item(), torch.autograd.grad(loss, ay)

    l64, g64 = run(torch.float64)
    l32, g32 = run(torch.float32)
    ghip, lhip = _hip_head(m, x, y, fx, fy)
    print(f"\nhead {h}x{w}: loss float64 {l64!r}, float32 slices (CPU) {l32!r}, staged HIP entries {lhip!r}")
    assert abs(lhip - l64) <= 1e-6
    bad = []
    for k in range(6):
        bad += _check_against_yardstick(f"map y{k}", ghip[k].cpu(), g32[k], g64[k])
    assert not bad, bad


# ---- module level --------------------------------------------------------------------------------------------------
def _convs_of(spec, dtype):
    from nerf_qa_amd.vgg_weights import load_vgg16_convs
    convs, _ = load_vgg16_convs(spec)
    return [(w.to(dtype), b.to(dtype)) for w, b in convs]


def _compare(tag, gd, gc):
    """The bounds of test_gpu_backward._compare_grads."""
    gd, gc = gd.cpu().double(), gc.double()
    scale = gc.abs().max().item()
    d = gd - gc
    err, rms = d.abs().max().item() / scale, d.pow(2).mean().sqrt().item() / gc.pow(2).mean().sqrt().item()
    cos = F.cosine_similarity(gd.flatten(), gc.flatten(), dim=0).item()
    print(f"{tag}: max|grad| {scale:.3e}  max err / max {err:.2e}  rms err / rms {rms:.2e}  cosine {cos:.8f}")
    assert torch.isfinite(gd).all() and err <= 2e-2 and rms <= 3e-3 and cos >= 0.99999, (tag, err, rms, cos)


def _is_ours(loss):
    from nerf_qa_amd import autograd
    return isinstance(loss.grad_fn, autograd.AdistsLossY._backward_cls)


MODULE_CASES = [(40, 56, ("noise10", "blur")), (63, 85, ("indep", "noise02")), (96, 112, ("blur", "noise10")),
                (48, 64, ("noise02", "nerf_grad", "blur"))]


@pytest.mark.parametrize("h,w,kinds", MODULE_CASES, ids=["40x56", "63x85_ragged", "96x112", "48x64_B3"])
def test_module_y_gradient_matches_autograd_over_the_oracle(h, w, kinds, dev):
    from nerf_qa_amd import autograd, synth
    from nerf_qa_amd.ADISTS import ADISTS
    from oracle import adists_oracle as ao
    from oracle import dists_oracle as do
    spec = "synth:1234"
    b = len(kinds)
    xn, yn = synth.frame_batch([21 + i for i in range(b)], h, w, list(kinds))
    c64 = _convs_of(spec, torch.float64)
    xc, yc = torch.from_numpy(xn).double(), torch.from_numpy(yn).double().requires_grad_()
    ref = ao.adists_from_feats(do.vgg_pyramid(xc, c64), do.vgg_pyramid(yc, c64), as_loss=True)
    ref.backward()
    for head_kind in ("auto", "torch"):
        m = ADISTS(vgg16_path=spec, loss_head=head_kind).to(dev).eval()
        xd, yd = torch.from_numpy(xn).to(dev), torch.from_numpy(yn).to(dev).requires_grad_()
        loss = m(xd, yd)
        assert loss.dim() == 0 and loss.requires_grad and abs(loss.item() - ref.item()) <= 1e-4
        assert _is_ours(loss) == (head_kind == "auto"), (head_kind, loss.grad_fn)
        with torch.no_grad():
            assert abs(loss.item() - m(xd, yd).item()) <= 1e-7  # the value IS the scoring path's
        loss.backward()
        assert xd.grad is None and yd.grad is not None
        _compare(f"A-DISTS {h}x{w} B={b} loss_head={head_kind} d/dy", yd.grad, yc.grad)


def test_x_requiring_grad_keeps_the_torch_head(dev):
    from nerf_qa_amd import autograd, synth
    from nerf_qa_amd.ADISTS import ADISTS
    m = ADISTS(vgg16_path="synth:1234", loss_head="auto").to(dev).eval()
    xn, yn = synth.frame_batch([5], 40, 56)
    for gx, gy in ((True, False), (True, True)):
        xd = torch.from_numpy(xn).to(dev).requires_grad_(gx)
        yd = torch.from_numpy(yn).to(dev).requires_grad_(gy)
        loss = m(xd, yd)
        assert loss.requires_grad and not _is_ours(loss)


# ---- behaviour -----------------------------------------------------------------------------------------------------
def _step(m, x, y):
    yd = y.detach().clone().requires_grad_()
    loss = m(x, yd)
    loss.backward()
    return loss.detach(), yd.grad


def test_step_is_sync_free_repeatable_and_batch_independent(dev):
    from nerf_qa_amd import synth
    from nerf_qa_amd.ADISTS import ADISTS
    m = ADISTS(vgg16_path="synth:1234", loss_head="auto").to(dev).eval()
    xn, yn = synth.frame_batch([31, 32], 48, 64, ["noise10", "nerf_grad"])
    x, y = torch.from_numpy(xn).to(dev), torch.from_numpy(yn).to(dev)
    l1, g1 = _step(m, x, y)  # warm-up: packs the weights, sizes the scratch
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        l2, g2 = _step(m, x, y)  # no device -> host read anywhere in the step
    finally:
        torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
    assert torch.isfinite(g1).all() and g1.abs().max().item() > 0
    assert torch.equal(g1, g2) and torch.equal(l1, l2)
    l3, g3 = _step(m, x, y)
    assert torch.equal(g1, g3)
    # pair 0 on its own, with the u it has in the batch
    from nerf_qa_amd import autograd
    u = torch.full((2,), -0.5, device=dev)
    both = autograd.adists_backward_y(m, x, y, u)
    one = autograd.adists_backward_y(m, x[:1], y[:1], u[:1])
    assert torch.equal(both, g3) and torch.equal(both[:1], one)
    # and through the module: 1 - D_0 against 1 - (D_0 + D_1) / 2 makes u_0 twice the batch's, an exact power of two all
    # the way down the linear chain
    _, g_one = _step(m, x[:1].contiguous(), y[:1].contiguous())
    assert torch.equal(g_one * 0.5, g3[:1])
