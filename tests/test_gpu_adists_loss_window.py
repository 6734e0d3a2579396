"""ADISTS(window_size=n, loss_head="hip"): the loss step, prepared targets, the DISTS + A-DISTS pair step and the f16
gradient chain at window sizes other than 21, on the generic window-moments kernels (csrc/nqa_window_moments_n.hip,
nqa_adists_ts_backward_n).

Module level: y.grad against FLOAT64 autograd over the CPU oracle (oracle.adists_oracle.adists_from_feats(..., n,
as_loss=True) on oracle.dists_oracle.vgg_pyramid) inside the project's end-to-end gradient bounds (tests/test_gpu_backward.py:
max err / max <= 2e-2, rms err / rms <= 3e-3).  Head level (gradients towards x as well: the torch head with HIP window
moments): the criterion of tests/test_gpu_window_moments.py::test_head_gradients_against_float64_head, HIP_FACTOR times
the float32 slice form's own distance from the float64 head.  Scratch independence by the method of
tests/test_gpu_scratch_independence.py: equal bits under a 0x00 fill, a 0xFF fill and no fill of every workspace buffer
and every torch.empty tensor."""
import warnings

import pytest
import torch

import poison

pytestmark = pytest.mark.gpu

SPEC = "synth:1234"
MAX_ERR, RMS_ERR = 2e-2, 3e-3  # tests/test_gpu_backward.py _compare_grads


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _adists(dev, **kw):
    from nerf_qa_amd.ADISTS import ADISTS
    return ADISTS(vgg16_path=SPEC, **kw).to(dev).eval()


def _dists(dev, **kw):
    from nerf_qa_amd.DISTS_pytorch import DISTS
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return DISTS(vgg16_path=SPEC, precision="f32s", **kw).to(dev).eval()


_FRAMES, _FEATS, _REF = {}, {}, {}


def _frames(h, w):
    from nerf_qa_amd import synth
    if (h, w) not in _FRAMES:
        xn, yn = synth.frame_batch([21, 22], h, w, ["noise10", "blur"])
        _FRAMES[(h, w)] = (torch.from_numpy(xn), torch.from_numpy(yn))
    return _FRAMES[(h, w)]


def _reference(h, w, n):
    """(loss, d loss / dy) of the float64 oracle at window n, computed once per (frame, n); the float64 pyramids once per
    frame."""
    from nerf_qa_amd.vgg_weights import load_vgg16_convs
    from oracle import adists_oracle as ao
    from oracle import dists_oracle as do
    if (h, w) not in _FEATS:
        c64 = [(a.double(), b.double()) for a, b in load_vgg16_convs(SPEC)[0]]
        x, y = _frames(h, w)
        yc = y.double().requires_grad_()
        with torch.no_grad():
            fx = do.vgg_pyramid(x.double(), c64)
        _FEATS[(h, w)] = (fx, do.vgg_pyramid(yc, c64), yc)
    if (h, w, n) not in _REF:
        fx, fy, yc = _FEATS[(h, w)]
        ref = ao.adists_from_feats(fx, fy, n, as_loss=True)
        (g,) = torch.autograd.grad(ref, yc, retain_graph=True)
        _REF[(h, w, n)] = (ref.item(), g)
    return _REF[(h, w, n)]


def _errors(got, ref):
    gd, gc = got.detach().cpu().double(), ref.double()
    d = gd - gc
    return d.abs().max().item() / gc.abs().max().item(), d.pow(2).mean().sqrt().item() / gc.pow(2).mean().sqrt().item()


def _inside(tag, got, ref):
    err, rms = _errors(got, ref)
    print(f"{tag}: max err / max {err:.2e} ({err / MAX_ERR:.3f} of the bound)  rms err / rms {rms:.2e} "
          f"({rms / RMS_ERR:.3f} of the bound)")
    assert torch.isfinite(got).all() and err <= MAX_ERR and rms <= RMS_ERR, (tag, err, rms)


def _is_loss_y(loss):
    from nerf_qa_amd import autograd
    return isinstance(loss.grad_fn, autograd.AdistsLossY._backward_cls)


def _step(m, x, y):
    yd = y.detach().clone().requires_grad_()
    loss = m(x, yd)
    loss.backward()
    return loss.detach(), yd.grad


@pytest.mark.parametrize("n,h,w", [(7, 40, 56), (12, 66, 49), (33, 40, 56)], ids=["n7-40x56", "n12-66x49", "n33-40x56"])
def test_hip_loss_step_matches_float64_autograd_over_the_oracle(n, h, w, dev):
    """Gradient on y alone: AdistsLossY at every window.  At n = 12 on 66 x 49 and n = 33 on 40 x 56 the deeper stages lie
    under the window and take the global branch."""
    ref, gref = _reference(h, w, n)
    x, y = (t.to(dev) for t in _frames(h, w))
    m = _adists(dev, window_size=n, loss_head="hip")
    yd = y.clone().requires_grad_()
    loss = m(x, yd)
    assert loss.dim() == 0 and loss.requires_grad and _is_loss_y(loss), loss.grad_fn
    with torch.no_grad():
        assert abs(loss.item() - m(x, y).item()) <= 1e-7  # the value is the scoring path's
    assert abs(loss.item() - ref) <= 1e-4
    loss.backward()
    assert x.grad is None
    print()
    _inside(f"A-DISTS n={n} {h}x{w} B=2 loss_head=hip d/dy", yd.grad, gref)


def test_hip_loss_step_with_ragged_window_mean_planes(dev):
    """B = 1 at 41 x 56, n = 7: W % 4 == 0 moves rows as 16-byte accesses, but the image stage's window means are planes of
    35 x 50 = 1750 floats -- no multiple of 16 bytes -- and its probability map starts 8 bytes off a 16-byte boundary
    inside the chain's buffer (at 21, W % 4 == 0 makes both whole; 1080p at n = 7 has such a stage at 135 x 240)."""
    n, h, w = 7, 41, 56
    ref, gref = _reference(h, w, n)
    x, y = (t[:1].contiguous().to(dev) for t in _frames(h, w))
    m = _adists(dev, window_size=n, loss_head="hip")
    yd = y.clone().requires_grad_()
    loss = m(x, yd)
    assert _is_loss_y(loss)
    loss.backward()
    # pair 0 of the float64 batch of two: 1 - mean(D) over B = 2 halves pair 0's weight
    print()
    _inside(f"A-DISTS n={n} {h}x{w} B=1 loss_head=hip d/dy", yd.grad * 0.5, gref[:1])
    t = m.prepare_target(x)
    yt = y.clone().requires_grad_()
    m.forward_target(t, yt).backward()
    assert torch.equal(yt.grad, yd.grad)


def test_forward_target_differentiates_at_7(dev):
    n, h, w = 7, 40, 56
    x, y = (t.to(dev) for t in _frames(h, w))
    m = _adists(dev, window_size=n, loss_head="hip")
    loss, grad = _step(m, x, y)
    t = m.prepare_target(x)
    yd = y.clone().requires_grad_()
    lt = m.forward_target(t, yd)
    lt.backward()
    assert torch.equal(yd.grad, grad)
    with torch.no_grad():
        assert torch.equal(lt.detach(), m.forward_target(t, y))
    assert abs(lt.item() - loss.item()) <= 1e-6  # (the staged head's value against the fused kernel's)
    # as_loss=False with a vector upstream: the rows of 1 - D, each with its own weight
    yv = y.clone().requires_grad_()
    per = m.forward_target(t, yv, as_loss=False)
    assert per.shape == (2,)
    up = torch.tensor([0.25, -1.5], device=dev)
    per.backward(up)
    assert torch.isfinite(yv.grad).all()
    # pair b's gradient is that of 1 - mean(D) times B * up_b (the chain renormalises by powers of two: float rounding)
    for b in range(2):
        e, r = _errors(yv.grad[b], (grad[b] * (2 * up[b])).cpu())
        assert e <= 1e-4 and r <= 1e-4, (b, e, r)
    # "auto" and "torch" keep today's refusal
    for kind in ("auto", "torch"):
        other = _adists(dev, window_size=n, loss_head=kind)
        with pytest.raises(ValueError, match=r"adists\(x, y\)"):
            other.forward_target(other.prepare_target(x), y.clone().requires_grad_())


def test_pair_forward_target_at_7(dev):
    from nerf_qa_amd import pair
    n, h, w = 7, 40, 56
    x, y = (t.to(dev) for t in _frames(h, w))
    m, dm = _adists(dev, window_size=n, loss_head="hip"), _dists(dev)
    t = m.prepare_target(x)
    wd, wa = 0.75, 1.25
    y1 = y.clone().requires_grad_()
    d1 = dm.forward_target(dm.prepare_target(x), y1, require_grad=True, batch_average=True)
    (gd,) = torch.autograd.grad(d1, y1)
    y2 = y.clone().requires_grad_()
    a1 = m.forward_target(t, y2)
    (ga,) = torch.autograd.grad(a1, y2)
    yp = y.clone().requires_grad_()
    d, a = pair.forward_target(dm, m, t, yp, batch_average=True)
    assert torch.equal(d.detach(), d1.detach()) and torch.equal(a.detach(), a1.detach())
    (wd * d + wa * a).backward()
    print()
    _inside(f"pair step n={n} {h}x{w} against the two modules' gradients", yp.grad, (wd * gd + wa * ga).cpu())
    # a value the loss does not use costs nothing, and y.grad is then the other module's own
    yq = y.clone().requires_grad_()
    _, a2 = pair.forward_target(dm, m, t, yq, batch_average=True)
    a2.backward()
    assert torch.equal(yq.grad, ga)


def test_gradient_on_x_and_y_takes_the_torch_head_on_hip_moments(dev, monkeypatch):
    """n = 7 under "hip" with x requiring grad: the torch head, its window means from the HIP kernels.  The head's twelve
    gradients stay within HIP_FACTOR times the float32 slice form's own distance from the float64 head."""
    import grad_replay as gr
    from nerf_qa_amd import ops
    from nerf_qa_amd.ADISTS import head
    n, h, w = 7, 40, 56
    x, y = (t.to(dev) for t in _frames(h, w))
    m = _adists(dev, window_size=n, loss_head="hip")
    seen = []
    orig = ops.window_moments
    monkeypatch.setattr(ops, "window_moments", lambda a, b=None, window=21: (seen.append(window), orig(a, b, window))[1])
    xd, yd = x.clone().requires_grad_(), y.clone().requires_grad_()
    loss = m(xd, yd)
    assert loss.requires_grad and not _is_loss_y(loss)
    loss.backward()
    assert seen and set(seen) == {n}  # every windowed stage went through the HIP moments, at this window
    assert torch.isfinite(xd.grad).all() and torch.isfinite(yd.grad).all() and xd.grad.abs().max().item() > 0
    ref, gref = _reference(h, w, n)
    assert abs(loss.item() - ref) <= 1e-4
    print()
    _inside(f"A-DISTS n={n} {h}x{w} loss_head=hip, x and y require grad: d/dy", yd.grad, gref)
    monkeypatch.undo()
    with torch.no_grad():
        fx = [t.float().contiguous() for t in m.forward_once(x)]
        fy = [t.float().contiguous() for t in m.forward_once(y)]

    def run(cast, impl):
        ax, ay = [cast(t).requires_grad_() for t in fx], [cast(t).requires_grad_() for t in fy]
        val = 1 - head.adists_d(ax, ay, n, window_impl=impl).mean()
        return val.item(), torch.autograd.grad(val, ax + ay)

    l64, g64 = run(lambda t: t.detach().cpu().double(), "slices")
    l32, g32 = run(lambda t: t.detach().cpu().clone(), "slices")
    lhip, ghip = run(lambda t: t.detach().clone(), "hip")
    print(f"head n={n} {h}x{w}: loss float64 {l64!r}, float32 slices (CPU) {l32!r}, HIP moments {lhip!r}")
    assert abs(lhip - l64) <= 1e-6
    bad = []
    for k, (a, b, c) in enumerate(zip(ghip, g32, g64)):
        (em, er), (ym, yr) = gr.errors(a, c), gr.errors(b, c)
        print(f"  map {'xy'[k // 6]}{k % 6}: HIP max {em:.3e} rms {er:.3e}; yardstick max {ym:.3e} rms {yr:.3e}")
        assert torch.isfinite(a).all()
        if em > gr.bound(ym) or er > gr.bound(yr):
            bad.append((k, em, er, ym, yr))
    assert not bad, bad


def test_21_hip_is_auto_and_bit_4096_stays_inside_the_bounds(dev):
    from nerf_qa_amd import ops
    n, h, w = 21, 40, 56
    ref, gref = _reference(h, w, n)
    x, y = (t.to(dev) for t in _frames(h, w))
    la, ga = _step(_adists(dev, loss_head="auto"), x, y)
    mh = _adists(dev, loss_head="hip")
    lh, gh = _step(mh, x, y)
    assert torch.equal(la, lh) and torch.equal(ga, gh)
    # launch for launch: the same number of A-DISTS-class launches in a step
    counts = []
    for m in (_adists(dev, loss_head="auto"), mh):
        _step(m, x, y)
        torch.cuda.synchronize()
        ops.lib().nqa_timing_enable(1)
        try:
            _step(m, x, y)
            torch.cuda.synchronize()
            import ctypes
            launches, ms = (ctypes.c_int * 7)(), (ctypes.c_double * 7)()
            assert ops.lib().nqa_timing_collect(launches, ms) == 0
        finally:
            ops.lib().nqa_timing_enable(0)
        counts.append(list(launches))
    assert counts[0] == counts[1] and sum(counts[0]) > 0, counts
    try:
        ops.set_conv_variant(ops.DEFAULT_CONV_VARIANT | ops.CONV_MOMENTS_GENERIC)
        lg, gg = _step(mh, x, y)
        t = mh.prepare_target(x)
        yd = y.clone().requires_grad_()
        mh.forward_target(t, yd).backward()
    finally:
        ops.set_conv_variant(ops.DEFAULT_CONV_VARIANT)
    assert torch.equal(lg, lh)  # (the value comes from the scoring path, which the bit does not touch)
    print()
    _inside("A-DISTS n=21 loss_head=hip, 21-tap kernels", gh, gref)
    _inside("A-DISTS n=21 loss_head=hip, generic kernels (bit 4096)", gg, gref)
    assert torch.equal(yd.grad, gg)


def test_f16_gradient_chain_composes_with_hip_at_7(dev):
    n, h, w = 7, 40, 56
    ref, gref = _reference(h, w, n)
    x, y = (t.to(dev) for t in _frames(h, w))
    m = _adists(dev, window_size=n, loss_head="hip", grad_precision="f16")
    yd = y.clone().requires_grad_()
    loss = m(x, yd)
    assert _is_loss_y(loss)
    loss.backward()
    print()
    _inside(f"A-DISTS n={n} {h}x{w} loss_head=hip grad_precision=f16 d/dy", yd.grad, gref)
    full = _step(_adists(dev, window_size=n, loss_head="hip"), x, y)
    assert torch.equal(loss.detach(), full[0])  # the same value: only the chain behind the head changes


# ---- scratch independence (the method of tests/test_gpu_scratch_independence.py) ---------------------------------------
def _bytes(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


@pytest.mark.parametrize("step", ["hip_loss", "hip_target"])
def test_hip_steps_ignore_what_their_scratch_held(step, dev, monkeypatch):
    n, h, w = 7, 40, 56
    x, y = (t.to(dev) for t in _frames(h, w))
    m = _adists(dev, window_size=n, loss_head="hip", precision="f32s")

    def call():
        yd = y.detach().clone().requires_grad_()
        loss = m(x, yd) if step == "hip_loss" else m.forward_target(m.prepare_target(x), yd)
        loss.backward()
        torch.cuda.synchronize()
        return [loss.detach(), yd.grad]

    runs = {}
    print()
    for byte in poison.FILLS:
        with poison.poisoned(byte, m, monkeypatch=monkeypatch) as p:
            runs[byte] = call()
        print(f"  {step} n={n}: {p.report()}")
        p.require()
    assert not hasattr(torch.empty, "__wrapped__")
    runs[None] = call()
    for key, got in runs.items():
        for i, (a, b) in enumerate(zip(got, runs[None])):
            assert not torch.isnan(a).any(), (step, key, i)
            assert torch.equal(_bytes(a), _bytes(b)), (step, key, i, int((a != b).sum()))
    assert runs[None][1].abs().max().item() > 0
