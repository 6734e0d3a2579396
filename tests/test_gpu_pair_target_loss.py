"""DISTS + A-DISTS as ONE loss against a prepared target: pair.forward_target (nerf_qa_amd/pair.py;
autograd.PairTargetLoss, pair_target_forward / pair_target_backward).

What is held here:
  * with one metric used, y.grad is that module's own forward_target step bit for bit (the other metric arrives as None
    and runs nothing);
  * both values are the two modules' forward_target returns bit for bit, whichever module prepared the target;
  * with both used, L = wd d + wa a, y.grad against float64 autograd over the CPU oracle (dists_oracle.vgg_pyramid,
    adists_oracle.adists_from_feats, the DISTS score formula).  The project's per-metric bounds
    (test_gpu_backward._compare_grads: max error <= 2e-2 of the maximum, rms error <= 3e-3 of the rms) add by the triangle
    inequality: max|g - (wd gD + wa gA)| <= 2e-2 (wd max|gD| + wa max|gA|), rms likewise with 3e-3.  No cosine bound:
    cosine does not add;
  * alpha / beta get the gradients they get from dists_model.forward_target;
  * the step's forward runs the conv launches of ONE pyramid_keep and its backward those of ONE chain, both measured
    on a DISTS target step in the same test;
  * a whole step enqueues without one device -> host read;
  * batch independence, slices and gathers, the errors of the interface.

Weights synth:1234, B = 2, pairs from nerf_qa_amd/synth.py with the seeds of tests/test_gpu_target_loss.py (PAIR_SEED).
Shapes: 40x56 (windowed and global A-DISTS stages), 96x112 (three windowed stages), 20x20 (every stage global), 1x1
(DISTS only), 63x85 (ragged at every level).

Measured on an MI355X: see DESIGN.md 4.16."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SPEC = "synth:1234"
S_TOL = 5e-4  # tests/test_gpu_target_loss.py
PAIR_SEED = {"noise10": 51, "blur": 52, "indep": 53, "nerf_white": 54, "nerf_float": 55}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev):
    from nerf_qa_amd.DISTS_pytorch import DISTS
    return DISTS(vgg16_path=SPEC, precision="f32s").to(dev).eval()


@pytest.fixture(scope="module")
def amodel(dev):
    from nerf_qa_amd.ADISTS import ADISTS
    return ADISTS(vgg16_path=SPEC, loss_head="auto").to(dev).eval()


def _pairs_np(h, w, kinds):
    from nerf_qa_amd import synth
    return synth.frame_batch([PAIR_SEED[k] for k in kinds], h, w, list(kinds))


def _pairs(h, w, kinds, dev):
    xn, yn = _pairs_np(h, w, kinds)
    return torch.from_numpy(xn).to(dev), torch.from_numpy(yn).to(dev)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _pair_step(model, amodel, target, y, wd, wa, **kw):
    """(d, a, y.grad) of L = wd d + wa a; a weight of None leaves that value out of the loss altogether."""
    from nerf_qa_amd import pair
    yd = y.detach().clone().requires_grad_()
    d, a = pair.forward_target(model, amodel, target, yd, **kw)
    loss = 0
    if wd is not None:
        loss = loss + (wd * d).sum()
    if wa is not None:
        loss = loss + (wa * a).sum()
    loss.backward()
    return d.detach(), a.detach(), yd.grad


# ---- 1. one metric used: that module's own step, bit for bit ----------------------------------------------------------
DISTS_ONLY = [(40, 56, ("noise10", "blur")), (96, 112, ("nerf_float", "noise10")), (20, 20, ("indep", "nerf_white")),
              (1, 1, ("noise10", "indep"))]
ADISTS_ONLY = [(40, 56, ("noise10", "nerf_white")), (96, 112, ("blur", "nerf_float")), (20, 20, ("indep", "nerf_white"))]


@pytest.mark.parametrize("h,w,kinds", DISTS_ONLY, ids=[f"{h}x{w}" for h, w, _ in DISTS_ONLY])
def test_dists_value_alone_gives_the_dists_target_gradient_bit_for_bit(h, w, kinds, model, amodel, dev):
    from nerf_qa_amd import autograd, pair
    x, y = _pairs(h, w, kinds, dev)
    target = model.prepare_target(x)
    yd = y.clone().requires_grad_()
    d, a = pair.forward_target(model, amodel, target, yd, batch_average=True)
    node = autograd.PairTargetLoss._backward_cls
    assert d.dim() == 0 and a.dim() == 0 and isinstance(a.grad_fn, node)
    d.backward()
    yw = y.clone().requires_grad_()
    want = model.forward_target(target, yw, require_grad=True, batch_average=True)
    want.backward()
    assert torch.isfinite(yd.grad).all() and yw.grad.abs().max().item() > 0
    assert _same_bits(d.detach(), want.detach()) and _same_bits(yd.grad, yw.grad)


@pytest.mark.parametrize("h,w,kinds", ADISTS_ONLY, ids=[f"{h}x{w}" for h, w, _ in ADISTS_ONLY])
def test_adists_value_alone_gives_the_adists_target_gradient_bit_for_bit(h, w, kinds, model, amodel, dev):
    x, y = _pairs(h, w, kinds, dev)
    target = model.prepare_target(x)
    _, a, g = _pair_step(model, amodel, target, y, None, 1.0)
    yw = y.clone().requires_grad_()
    want = amodel.forward_target(amodel.prepare_target(x), yw)
    want.backward()
    assert torch.isfinite(g).all() and yw.grad.abs().max().item() > 0
    assert _same_bits(a, want.detach()) and _same_bits(g, yw.grad)


# ---- 2. both values are the modules' own; either module's target ------------------------------------------------------
@pytest.mark.parametrize("batch_average,as_loss", [(False, True), (True, False), (False, False), (True, True)])
def test_values_are_the_two_modules_values_bit_for_bit(batch_average, as_loss, model, amodel, dev):
    from nerf_qa_amd import pair
    x, y = _pairs(40, 56, ("noise10", "nerf_white"), dev)
    td, ta = model.prepare_target(x), amodel.prepare_target(x)
    assert all(_same_bits(p, q) for p, q in zip(td.taps, ta.taps))
    yw = y.clone().requires_grad_()
    want_d = model.forward_target(td, yw, require_grad=True, batch_average=batch_average)
    want_a = amodel.forward_target(ta, yw, as_loss=as_loss)
    upstream = torch.tensor([1.0, 0.5], device=dev)
    results = []
    for target in (td, ta):
        yd = y.clone().requires_grad_()
        d, a = pair.forward_target(model, amodel, target, yd, batch_average=batch_average, as_loss=as_loss)
        assert d.shape == want_d.shape and a.shape == want_a.shape and d.dtype == want_d.dtype and a.dtype == want_a.dtype
        assert d.requires_grad and a.requires_grad
        assert _same_bits(d.detach(), want_d.detach()) and _same_bits(a.detach(), want_a.detach())
        ((d if batch_average else d * upstream).sum() + (a if as_loss else a * upstream).sum()).backward()
        assert torch.isfinite(yd.grad).all() and yd.grad.abs().max().item() > 0
        results.append(yd.grad)
        with torch.no_grad():  # no gradient to form: the modules' own no-grad values (DISTS' score kernel) from y's taps
            d0, a0 = pair.forward_target(model, amodel, target, y, batch_average=batch_average, as_loss=as_loss)
            none_d = model.forward_target(td, y, require_grad=True, batch_average=batch_average)
            none_a = amodel.forward_target(ta, y, as_loss=as_loss)
        assert d0.grad_fn is None and a0.grad_fn is None
        assert _same_bits(d0, none_d) and _same_bits(a0, none_a) and _same_bits(a0, want_a.detach())
    assert _same_bits(results[0], results[1])  # a DISTS target and an A-DISTS target: the same bits


# ---- 3. both metrics used: float64 autograd over the oracle -----------------------------------------------------------
BOTH_SHAPES = {(40, 56): ("noise10", "blur"), (63, 85): ("indep", "noise10")}
_ORACLE = {}


def _oracle_grads(h, w, model):
    """(gD64, gA64): d(mean DISTS score)/dy and d(1 - mean D)/dy by float64 autograd on the CPU, once per shape."""
    if (h, w) not in _ORACLE:
        from nerf_qa_amd.vgg_weights import load_vgg16_convs
        from oracle import adists_oracle as ao
        from oracle import dists_oracle as do
        convs, _ = load_vgg16_convs(SPEC)
        c64 = [(wt.double(), bs.double()) for wt, bs in convs]
        xn, yn = _pairs_np(h, w, BOTH_SHAPES[(h, w)])
        xc, yc = torch.from_numpy(xn).double(), torch.from_numpy(yn).double().requires_grad_()
        with torch.no_grad():
            fx = do.vgg_pyramid(xc, c64)
        fy = do.vgg_pyramid(yc, c64)
        s1, s2 = do.dists_stats(fx, fy)
        d64 = do.dists_score(s1, s2, model.alpha.detach().cpu().double(), model.beta.detach().cpu().double()).mean()
        a64 = ao.adists_from_feats(fx, fy, as_loss=True)
        (gd,) = torch.autograd.grad(d64, yc, retain_graph=True)
        (ga,) = torch.autograd.grad(a64, yc)
        _ORACLE[(h, w)] = (gd, ga, d64.item(), a64.item())
    return _ORACLE[(h, w)]


@pytest.mark.parametrize("wd,wa", [(1.0, 1.0), (0.25, 2.0)])
@pytest.mark.parametrize("h,w", list(BOTH_SHAPES), ids=["40x56", "63x85_ragged"])
def test_weighted_sum_of_both_against_float64_autograd_over_the_oracle(h, w, wd, wa, model, amodel, dev):
    gd64, ga64, d64, a64 = _oracle_grads(h, w, model)
    x, y = _pairs(h, w, BOTH_SHAPES[(h, w)], dev)
    d, a, g = _pair_step(model, amodel, model.prepare_target(x), y, wd, wa, batch_average=True)
    assert abs(d.item() - d64) <= 1e-4 and abs(a.item() - a64) <= 1e-4
    g = g.cpu().double()
    err = g - (wd * gd64 + wa * ga64)
    rms = lambda t: t.pow(2).mean().sqrt().item()
    max_scale = wd * gd64.abs().max().item() + wa * ga64.abs().max().item()
    rms_scale = wd * rms(gd64) + wa * rms(ga64)
    e_max, e_rms = err.abs().max().item() / max_scale, rms(err) / rms_scale
    print(f"\n[pair loss] {h}x{w} wd={wd} wa={wa}: max|gD| {gd64.abs().max().item():.3e} max|gA| "
          f"{ga64.abs().max().item():.3e}  max err / bound scale {e_max:.2e} (<= 2e-2)  rms err / bound scale {e_rms:.2e} "
          f"(<= 3e-3)")
    assert torch.isfinite(g).all()
    assert e_max <= 2e-2 and e_rms <= 3e-3, (e_max, e_rms)


# ---- 4. alpha / beta ---------------------------------------------------------------------------------------------------
def test_pair_step_reaches_alpha_and_beta(amodel, dev):
    """The tolerance of tests/test_gpu_target_loss.py::test_dists_target_reaches_alpha_and_beta: two S1 / S2 each within
    S_TOL of one oracle are 2 S_TOL apart per entry, the gradients 2 * 2 S_TOL / w (w = sum alpha + sum beta)."""
    from nerf_qa_amd import pair
    from nerf_qa_amd.DISTS_pytorch import DISTS
    m = DISTS(vgg16_path=SPEC, precision="f32s").to(dev).eval()
    m.alpha.requires_grad_(True)
    m.beta.requires_grad_(True)
    x, y = _pairs(40, 56, ("noise10", "blur"), dev)
    target = m.prepare_target(x)
    yd = y.clone().requires_grad_()
    d, a = pair.forward_target(m, amodel, target, yd, batch_average=True)
    (d + a).backward()
    ga, gb = m.alpha.grad.clone(), m.beta.grad.clone()
    m.alpha.grad = m.beta.grad = None
    yw = y.clone().requires_grad_()
    m.forward_target(target, yw, require_grad=True, batch_average=True).backward()
    assert ga.abs().max().item() > 0 and gb.abs().max().item() > 0
    tol = 4 * S_TOL / (m.alpha.sum() + m.beta.sum()).item()
    assert (ga - m.alpha.grad).abs().max().item() <= tol and (gb - m.beta.grad).abs().max().item() <= tol


# ---- 5. one pyramid, one chain -----------------------------------------------------------------------------------------
def _counted(fn):
    """(fn's result, conv launches, statistics launches) of the calling thread."""
    from nerf_qa_amd import ops
    ops.timing_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        kt = ops.timing_collect()
    finally:
        ops.timing_enable(False)
    return out, kt["conv1_1"][0] + kt["conv_igemm"][0], kt["stats"][0]


def test_pair_step_runs_one_pyramid_and_one_chain(model, amodel, dev):
    """The launch counters are per thread and autograd runs a backward on a thread of its own, so the two halves of the
    step are called here as the Function calls them (autograd.pair_target_forward / pair_target_backward), beside the
    halves of a DISTS target step on the same pairs."""
    from nerf_qa_amd import autograd
    x, y = _pairs(40, 56, ("noise10", "blur"), dev)
    target = model.prepare_target(x)
    b = x.shape[0]
    al, bt = model._score_weights()
    g1, g2 = (-(al / b)).expand(b, -1).contiguous().to(dev), (-(bt / b)).expand(b, -1).contiguous().to(dev)
    u = torch.full((b,), -1.0 / b, device=dev)
    (_, _, dstate), n_dfwd, st_dfwd = _counted(lambda: autograd.dists_target_forward(model, target, y))
    gd, n_dbwd, st_dbwd = _counted(lambda: autograd.dists_target_backward(model, target, dstate, g1, g2))
    (_, astate), n_afwd, _ = _counted(lambda: autograd.adists_target_d(amodel, target, y, keep=True))
    assert n_dfwd == 13 and n_dbwd > 0 and n_afwd == n_dfwd
    (s1, s2, dd, state), n_fwd, st_fwd = _counted(lambda: autograd.pair_target_forward(amodel, target, y))
    gy, n_bwd, st_bwd = _counted(lambda: autograd.pair_target_backward(amodel, target, y, state, g1, g2, u))
    assert n_fwd == n_dfwd  # ONE kept pyramid of y for both heads
    assert n_bwd == n_dbwd  # ONE chain for both metrics' tap gradients
    assert st_bwd == st_dbwd  # per tap the coefficient launch and ONE gradient launch, accumulating or not
    assert st_fwd >= st_dfwd
    assert torch.isfinite(gy).all() and gy.abs().max().item() > 0
    # one metric alone through the same halves: the single steps' bits
    ga = autograd.adists_y_backward(amodel, target.x, list(target.taps), y, astate, u)
    assert _same_bits(autograd.pair_target_backward(amodel, target, y, state, g1, g2, None), gd)
    assert _same_bits(autograd.pair_target_backward(amodel, target, y, state, None, None, u), ga)


# ---- 6. no host read ---------------------------------------------------------------------------------------------------
def test_pair_step_enqueues_without_a_host_read(model, amodel, dev):
    x, y = _pairs(48, 64, ("noise10", "nerf_float"), dev)
    target = amodel.prepare_target(x)
    step = lambda: _pair_step(model, amodel, target, y, 1.0, 1.0, batch_average=True)
    warm = step()  # packing, workspace, the backward's weight blobs, the weights comparison
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = step()
    finally:
        torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
    assert torch.isfinite(got[2]).all() and got[2].abs().max().item() > 0
    assert all(_same_bits(p, q) for p, q in zip(got, warm))


# ---- 7. batch handling -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(40, 56), (33, 47)])
def test_a_pairs_gradient_does_not_depend_on_its_batch_neighbour(h, w, model, amodel, dev):
    """Pair 0 alone against pair 0 beside a pair whose upstream gradients, of both metrics, are 2^12 times larger."""
    from nerf_qa_amd import pair
    x, y = _pairs(h, w, ("noise10", "nerf_float"), dev)
    target = model.prepare_target(x)
    ya = y[:1].clone().requires_grad_()
    d, a = pair.forward_target(model, amodel, target[0:1], ya, as_loss=False)
    (d + a).sum().backward()
    yb = y.clone().requires_grad_()
    d, a = pair.forward_target(model, amodel, target, yb, as_loss=False)
    ((d + a) * torch.tensor([1.0, 4096.0], device=dev)).sum().backward()
    assert ya.grad.abs().max().item() > 0 and yb.grad[1].abs().max().item() > 64 * yb.grad[0].abs().max().item()
    assert _same_bits(ya.grad[0], yb.grad[0])


def test_slices_and_gathers_of_a_target(model, amodel, dev):
    x, y = _pairs(40, 56, ("nerf_white", "blur"), dev)
    for owner in (model, amodel):
        target = owner.prepare_target(x)
        step = lambda t, yy: _pair_step(model, amodel, t, yy, 1.0, 1.0, as_loss=False)
        _, _, g_slice = step(target[1:2], y[1:2])
        _, _, g_fresh = step(owner.prepare_target(x[1:2]), y[1:2])
        assert g_fresh.abs().max().item() > 0 and _same_bits(g_slice, g_fresh)
        idx = torch.tensor([1, 0])
        _, _, g_sel = step(target.select(idx), y[[1, 0]])
        _, _, g_fresh = step(owner.prepare_target(x[[1, 0]]), y[[1, 0]])
        assert _same_bits(g_sel, g_fresh)


# ---- 8. errors ---------------------------------------------------------------------------------------------------------
def test_errors_of_the_interface(model, amodel, dev, monkeypatch):
    from nerf_qa_amd import pair
    from nerf_qa_amd._lib import NqaError
    from nerf_qa_amd.ADISTS import ADISTS
    from nerf_qa_amd.DISTS_pytorch import DISTS
    x, y = _pairs(40, 56, ("noise10", "blur"), dev)
    target = model.prepare_target(x)
    other = ADISTS(vgg16_path="synth:7", loss_head="auto").to(dev).eval()
    with pytest.raises(NqaError, match="different VGG-16 weights"):
        pair.forward_target(model, other, target, y)
    with pytest.raises(NqaError, match="GPU only"):
        pair.forward_target(model, amodel, target, y.cpu())
    third = DISTS(vgg16_path=SPEC, precision="f32s").to(dev).eval()
    with pytest.raises(ValueError, match="another module"):
        pair.forward_target(model, amodel, third.prepare_target(x), y)
    with pytest.raises(ValueError, match="prepare_target returned"):
        pair.forward_target(model, amodel, x, y)
    with pytest.raises(ValueError, match="shape"):
        pair.forward_target(model, amodel, target, y[:1])
    with pytest.raises(ValueError, match="shape"):
        pair.forward_target(model, amodel, target, y[:, :, :32])
    # a stale target: one conv weight of its owner changed in place after preparing
    stale = third.prepare_target(x)
    with torch.no_grad():
        third._conv_modules()[3].weight.mul_(1.0)
    with pytest.raises(ValueError, match="weights changed"):
        pair.forward_target(third, amodel, stale, y)
    pair.forward_target(third, amodel, third.prepare_target(x), y)  # prepared again: accepted
    # a batch whose A-DISTS scratch passes the workspace budget
    monkeypatch.setenv("NQA_MAX_WORKSPACE_GB", "0.0001")
    with pytest.raises(NqaError, match=r"target\[i:j\]"):
        pair.forward_target(model, amodel, target, y)
    monkeypatch.delenv("NQA_MAX_WORKSPACE_GB")
    # the single-metric interface goes on refusing the other module's targets
    with pytest.raises(ValueError, match="another module"):
        model.forward_target(amodel.prepare_target(x), y)
    with pytest.raises(ValueError, match="another module"):
        amodel.forward_target(target, y)
    # score_pair is as it was
    with pytest.raises(ValueError, match="does not differentiate"):
        pair.score_pair(model, amodel, x, y.clone().requires_grad_())
