"""A loss against a PREPARED TARGET: DISTS.prepare_target / forward_target and ADISTS.prepare_target / forward_target
(nerf_qa_amd/target.py; autograd.DistsTargetSimilarities, autograd.AdistsTargetLoss).

What is held here:
  * y.grad of a target step equals y.grad of the existing one-sided step (forward(x, y, require_grad=True) /
    ADISTS(loss_head="auto")(x, y)) bit for bit: both run the same kernels on the same operands, and the upstream
    gradients of S1 / S2 depend on alpha / beta alone;
  * the values: DISTS scores within SCORE_TOL["f32s"] = 1e-4 and S1 / S2 within the f32s s_tol = 5e-4 (per-channel
    maximum) of the CPU oracle, both constants as they stand in tests/test_gpu_dists.py; A-DISTS 1 - D within
    SCORE_TOL["f32s"] = 1e-4 of oracle/adists_oracle.py, the bound of tests/test_gpu_adists.py.  The oracle runs in
    float64;
  * a whole target step enqueues without one device -> host read, for both metrics;
  * a DISTS target step runs the conv launches of one pyramid_keep and one backward chain, nothing more;
  * slices and gathers of a target, and a pair alone against the pair beside a neighbour, bit for bit;
  * the errors of the interface.

Weights synth:1234; pairs from nerf_qa_amd/synth.py, one seed per content kind (PAIR_SEED); B = 2 with two different
kinds.  Shapes: 33x47 (every level odd: 33 17 9 5 3), 40x56 (the last tap is 3x4), 96x112 (the first three A-DISTS
stages windowed, the rest global), 1x1, and 20x20 for A-DISTS (every stage global).  The A-DISTS VALUES take 88x88 in
the place of 96x112: the same paths (88, 44 and 22 windowed, 11 and 6 global) at a quarter of the float64 oracle's time
on the CPU (2.7 s against 11 s; the gradient comparison, which needs no oracle, stays at 96x112).

The A-DISTS pairs were checked on the CPU before they were chosen, as small frames sit near the dead-channel
discontinuity (AUTO_EXACT_PIXELS in ADISTS.py): oracle/adists_oracle.py in float32 against float64 on each of the five
kinds with its seed at 20x20, 33x47, 40x56 and 96x112 differs by 1.2e-10 .. 6.2e-7 in 1 - D (worst: nerf_float at 33x47),
and by 2.8e-8 on the blur + nerf_float batch at 88x88, far inside the 1e-4 bound; no pair had to be dropped or replaced.
(84x84 was tried first and dropped as a SHAPE: its third stage is a single 21x21 window, and the oracle's texture
probabilities are NaN there -- the standard deviation of a one-element map, the reference's own behaviour.)  The DISTS
oracle's own float32 run is 3.2e-6 .. 1.2e-4 from its float64 run in max |dS| on the same pairs (worst: S2 of nerf_float
at 96x112), inside s_tol.

Measured on an MI355X: see DESIGN.md 4.15."""
import pickle

import pytest
import torch

pytestmark = pytest.mark.gpu

SPEC = "synth:1234"
SCORE_TOL = 1e-4  # tests/test_gpu_dists.py SCORE_TOL["f32s"]; tests/test_gpu_adists.py SCORE_TOL["f32s"]
S_TOL = 5e-4      # tests/test_gpu_dists.py test_dists_vs_golden, s_tol of "f32s": the per-channel maximum
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


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _convs64():
    from nerf_qa_amd.vgg_weights import load_vgg16_convs
    convs, _ = load_vgg16_convs(SPEC)
    return [(w.double(), b.double()) for w, b in convs]


def _dists_target_grad(model, target, y, **kw):
    yd = y.detach().clone().requires_grad_()
    loss = model.forward_target(target, yd, require_grad=True, batch_average=True, **kw)
    loss.backward()
    return loss.detach(), yd.grad


def _dists_grad(model, x, y):
    yd = y.detach().clone().requires_grad_()
    loss = model(x, yd, require_grad=True, batch_average=True)
    loss.backward()
    return loss.detach(), yd.grad


def _adists_target_grad(m, target, y):
    yd = y.detach().clone().requires_grad_()
    loss = m.forward_target(target, yd)
    loss.backward()
    return loss.detach(), yd.grad


def _adists_grad(m, x, y):
    yd = y.detach().clone().requires_grad_()
    loss = m(x, yd)
    loss.backward()
    return loss.detach(), yd.grad


# ---- 1. the gradient is the existing step's, bit for bit --------------------------------------------------------------
DISTS_CASES = [(33, 47, ("nerf_white", "indep")), (40, 56, ("noise10", "blur")), (96, 112, ("nerf_float", "noise10")),
               (1, 1, ("noise10", "indep"))]


@pytest.mark.parametrize("h,w,kinds", DISTS_CASES, ids=[f"{h}x{w}" for h, w, _ in DISTS_CASES])
def test_dists_target_gradient_is_the_one_sided_gradient_bit_for_bit(h, w, kinds, model, dev):
    x, y = _pairs(h, w, kinds, dev)
    target = model.prepare_target(x)
    assert tuple(target.shape) == tuple(x.shape) and len(target) == 2
    assert target.nbytes == 4 * (x.numel() + sum(t.numel() for t in target.taps)) and len(target.taps) == 5
    assert not target.x.requires_grad and target.x.data_ptr() != x.data_ptr() and torch.equal(target.x, x)
    lt, gt = _dists_target_grad(model, target, y)
    lw, gw = _dists_grad(model, x, y)
    assert torch.isfinite(gt).all() and gw.abs().max().item() > 0
    assert _same_bits(gt, gw)
    assert abs(lt.item() - lw.item()) <= 2 * SCORE_TOL  # (the fused forward's value; each is held to SCORE_TOL of one oracle)
    again = _dists_target_grad(model, target, y)
    assert _same_bits(again[1], gt) and torch.equal(again[0], lt)  # repeatable, and the target is left as it was
    # per-pair scores and per-pair upstream gradients
    yd = y.clone().requires_grad_()
    score = model.forward_target(target, yd, require_grad=True)
    assert score.shape == (2,) and score.requires_grad
    (score * torch.tensor([1.0, 0.5], device=dev)).sum().backward()
    yw = y.clone().requires_grad_()
    (model(x, yw, require_grad=True) * torch.tensor([1.0, 0.5], device=dev)).sum().backward()
    assert _same_bits(yd.grad, yw.grad)


def test_dists_target_reaches_alpha_and_beta(dev):
    """alpha / beta get their gradients through _weighted as in forward.  The two S1 / S2 come from different forwards,
    each within S_TOL of one oracle, so at most 2 S_TOL apart per entry; d(score)/d(alpha_c) = -(S1_c - sum) / w with
    sum = (alpha . S1 + beta . S2) / w a weighted mean of the entries, so the gradients are at most 2 * 2 S_TOL / w
    apart (w = sum alpha + sum beta)."""
    from nerf_qa_amd.DISTS_pytorch import DISTS
    m = DISTS(vgg16_path=SPEC, precision="f32s").to(dev).eval()
    m.alpha.requires_grad_(True)
    m.beta.requires_grad_(True)
    x, y = _pairs(40, 56, ("noise10", "blur"), dev)
    target = m.prepare_target(x)
    m.forward_target(target, y, batch_average=True).backward()  # y takes no gradient: nothing kept, alpha / beta still do
    ga, gb = m.alpha.grad.clone(), m.beta.grad.clone()
    m.alpha.grad = m.beta.grad = None
    m(x, y, batch_average=True).backward()
    assert ga.abs().max().item() > 0 and gb.abs().max().item() > 0
    tol = 4 * S_TOL / (m.alpha.sum() + m.beta.sum()).item()
    assert (ga - m.alpha.grad).abs().max().item() <= tol and (gb - m.beta.grad).abs().max().item() <= tol


ADISTS_CASES = [(40, 56, ("noise10", "nerf_white")), (96, 112, ("blur", "nerf_float")), (20, 20, ("indep", "nerf_white"))]


@pytest.mark.parametrize("h,w,kinds", ADISTS_CASES, ids=[f"{h}x{w}" for h, w, _ in ADISTS_CASES])
def test_adists_target_gradient_is_the_one_sided_gradient_bit_for_bit(h, w, kinds, amodel, dev):
    from nerf_qa_amd import autograd
    x, y = _pairs(h, w, kinds, dev)
    target = amodel.prepare_target(x)
    yd = y.clone().requires_grad_()
    loss = amodel.forward_target(target, yd)
    assert loss.dim() == 0 and isinstance(loss.grad_fn, autograd.AdistsTargetLoss._backward_cls)
    loss.backward()
    lw, gw = _adists_grad(amodel, x, y)
    assert torch.isfinite(yd.grad).all() and gw.abs().max().item() > 0
    assert _same_bits(yd.grad, gw)
    assert abs(loss.item() - lw.item()) <= 2 * SCORE_TOL  # (the fused kernel's value; each is held to SCORE_TOL of one oracle)
    # as_loss=False: 1 - D per pair; with the upstream 1 / B it is the loss's gradient (u = -1 / B either way)
    yp = y.clone().requires_grad_()
    per = amodel.forward_target(target, yp, as_loss=False)
    assert per.shape == (2,)
    (per * 0.5).sum().backward()
    assert _same_bits(yp.grad, gw)


# ---- 2. values ---------------------------------------------------------------------------------------------------------
VALUE_CASES = [(33, 47, ("nerf_white", "indep")), (40, 56, ("noise10", "blur")), (96, 112, ("nerf_float", "noise10"))]


@pytest.mark.parametrize("h,w,kinds", VALUE_CASES, ids=[f"{h}x{w}" for h, w, _ in VALUE_CASES])
def test_dists_target_values_against_the_cpu_oracle(h, w, kinds, model, dev):
    from nerf_qa_amd import autograd
    from oracle import dists_oracle as do
    xn, yn = _pairs_np(h, w, kinds)
    x, y = torch.from_numpy(xn).to(dev), torch.from_numpy(yn).to(dev)
    c64 = _convs64()
    with torch.no_grad():
        w1, w2 = do.dists_stats(do.vgg_pyramid(torch.from_numpy(xn).double(), c64),
                                do.vgg_pyramid(torch.from_numpy(yn).double(), c64))
        want = do.dists_score(w1, w2, model.alpha.detach().cpu().double(), model.beta.detach().cpu().double())
    target = model.prepare_target(x)
    with torch.no_grad():
        score = model.forward_target(target, y)
        s1, s2 = autograd.dists_target_similarities(model, target, y)
    k1, k2, _ = autograd.dists_target_forward(model, target, y)  # the kept-pyramid forward gives the same numbers
    assert _same_bits(k1, s1) and _same_bits(k2, s2)
    d = (score.cpu().double() - want).abs().max().item()
    e1, e2 = (s1.cpu().double() - w1).abs().max().item(), (s2.cpu().double() - w2).abs().max().item()
    print(f"\n[target values] DISTS {h}x{w} {'+'.join(kinds)}: |dscore| {d:.2e}  max|dS1| {e1:.2e}  max|dS2| {e2:.2e}")
    assert d <= SCORE_TOL and e1 <= S_TOL and e2 <= S_TOL, (d, e1, e2)


ADISTS_VALUE_CASES = [(40, 56, ("noise10", "nerf_white")), (88, 88, ("blur", "nerf_float")), (20, 20, ("indep", "nerf_white"))]


@pytest.mark.parametrize("h,w,kinds", ADISTS_VALUE_CASES, ids=[f"{h}x{w}" for h, w, _ in ADISTS_VALUE_CASES])
def test_adists_target_values_against_the_cpu_oracle(h, w, kinds, amodel, dev):
    from oracle import adists_oracle as ao
    xn, yn = _pairs_np(h, w, kinds)
    x, y = torch.from_numpy(xn).to(dev), torch.from_numpy(yn).to(dev)
    with torch.no_grad():
        want = ao.adists(torch.from_numpy(xn).double(), torch.from_numpy(yn).double(), _convs64(), as_loss=False)
    target = amodel.prepare_target(x)
    with torch.no_grad():
        per = amodel.forward_target(target, y, as_loss=False)
        loss = amodel.forward_target(target, y)
    yd = y.clone().requires_grad_()
    kept = amodel.forward_target(target, yd, as_loss=False)
    assert _same_bits(kept.detach(), per)
    d = (per.cpu().double() - want.flatten()).abs().max().item()
    dl = abs(loss.item() - want.mean().item())
    print(f"\n[target values] A-DISTS {h}x{w} {'+'.join(kinds)}: max|d(1 - D)| {d:.2e}  |dloss| {dl:.2e}")
    assert per.shape == (2,) and loss.dim() == 0
    assert d <= SCORE_TOL and dl <= SCORE_TOL, (d, dl)


# ---- 3. no host read ---------------------------------------------------------------------------------------------------
def _sync_free(step):
    warm = step()  # packing, workspace, the backward's weight blobs
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = step()
    finally:
        torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
    assert torch.isfinite(got[1]).all() and got[1].abs().max().item() > 0
    assert _same_bits(got[1], warm[1]) and torch.equal(got[0], warm[0])


def test_dists_target_step_enqueues_without_a_host_read(model, dev):
    x, y = _pairs(64, 80, ("noise10", "nerf_white"), dev)
    target = model.prepare_target(x)
    _sync_free(lambda: _dists_target_grad(model, target, y))


def test_adists_target_step_enqueues_without_a_host_read(amodel, dev):
    x, y = _pairs(48, 64, ("noise10", "nerf_float"), dev)
    target = amodel.prepare_target(x)
    _sync_free(lambda: _adists_target_grad(amodel, target, y))


# ---- 4. one pyramid per step -------------------------------------------------------------------------------------------
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


def test_dists_target_step_runs_one_pyramid(model, dev):
    """The launch counters are per thread and autograd runs a backward on a thread of its own, so the two halves of the
    step are called here as the Function calls them (autograd.dists_target_forward / dists_target_backward)."""
    from nerf_qa_amd import autograd, ops
    x, y = _pairs(40, 56, ("noise10", "blur"), dev)
    target = model.prepare_target(x)
    b = x.shape[0]
    a, bt = model._score_weights()
    g1, g2 = (-(a / b)).expand(b, -1).contiguous().to(dev), (-(bt / b)).expand(b, -1).contiguous().to(dev)
    (acts, taps, pooled), n_keep, _ = _counted(lambda: autograd.pyramid_keep(model, y))
    _, n_taps, _ = _counted(lambda: autograd.pyramid_taps(model, x))
    g_taps = [torch.ones_like(t) for t in taps]
    _, n_chain, _ = _counted(lambda: autograd.pyramid_backward_device(model, acts, taps, pooled, g_taps))
    assert n_keep == 13 and n_taps == n_keep and n_chain > 0  # conv1_1 + twelve layers, layer by layer
    # the target step
    (s1, s2, state), n_fwd, st_fwd = _counted(lambda: autograd.dists_target_forward(model, target, y))
    gy, n_bwd, st_bwd = _counted(lambda: autograd.dists_target_backward(model, target, state, g1, g2))
    assert n_fwd == n_keep  # ONE kept pyramid, nothing of x
    assert n_bwd == n_chain  # no pyramid in the backward
    # the existing one-sided step on the same pair: the fused forward, then pyramid_taps(x) + pyramid_keep(y) + the chain
    packed = model._packed_weights(dev, "f32s")
    _, n_fused, _ = _counted(lambda: ops.dists_forward(x, y, packed, "f32s", model._ws))
    (_, wy), n_old, st_old = _counted(lambda: autograd.dists_backward(model, x, y, g1, g2, need=(False, True)))
    assert n_fused > 0 and n_old == n_taps + n_keep + n_chain  # what falls out of a step: n_fused + n_taps conv launches
    # the statistics run once: per tap sums + fold | coefficients + gradient against sums + coefficients + gradient (the
    # fold is the one launch more, five taps), tap 0 the same launches split between forward and backward
    assert st_fwd + st_bwd == st_old + 5
    assert _same_bits(gy, wy)


# ---- 5. batch handling -------------------------------------------------------------------------------------------------
def test_slices_and_gathers_of_a_target(model, amodel, dev):
    x, y = _pairs(40, 56, ("nerf_white", "blur"), dev)
    for m, grad in ((model, _dists_target_grad), (amodel, _adists_target_grad)):
        target = m.prepare_target(x)
        sl = target[1:2]
        assert len(sl) == 1 and tuple(sl.shape) == (1, 3, 40, 56) and sl.nbytes * 2 == target.nbytes
        assert sl.x.data_ptr() == target.x[1:2].data_ptr()  # views, no copy
        assert all(a.data_ptr() == t[1:2].data_ptr() for a, t in zip(sl.taps, target.taps))
        _, g_slice = grad(m, sl, y[1:2])
        _, g_fresh = grad(m, m.prepare_target(x[1:2]), y[1:2])
        assert g_fresh.abs().max().item() > 0 and _same_bits(g_slice, g_fresh)
        idx = torch.tensor([1, 0])
        sel = target.select(idx)
        assert len(sel) == 2 and sel.x.data_ptr() != target.x.data_ptr() and torch.equal(sel.x, x[[1, 0]])
        _, g_sel = grad(m, sel, y[[1, 0]])
        _, g_fresh = grad(m, m.prepare_target(x[[1, 0]]), y[[1, 0]])
        assert _same_bits(g_sel, g_fresh)
        with pytest.raises(TypeError):
            target[0]
        with pytest.raises(ValueError):
            target[2:2]
        with pytest.raises(ValueError):
            target.select(torch.tensor([0.0]))
        with pytest.raises(TypeError, match="does not pickle"):
            pickle.dumps(target)


@pytest.mark.parametrize("h,w", [(40, 56), (33, 47)])
def test_a_pairs_target_gradient_does_not_depend_on_its_batch_neighbour(h, w, model, amodel, dev):
    """Pair 0 alone against pair 0 next to a pair whose upstream gradient is 2^12 times larger (DISTS); A-DISTS: the
    loss of one pair has u_0 twice the batch's, an exact power of two all the way down the linear chain."""
    x, y = _pairs(h, w, ("noise10", "nerf_float"), dev)
    target = model.prepare_target(x)
    ya = y[:1].clone().requires_grad_()
    model.forward_target(target[0:1], ya, require_grad=True).sum().backward()
    yb = y.clone().requires_grad_()
    (model.forward_target(target, yb, require_grad=True) * torch.tensor([1.0, 4096.0], device=dev)).sum().backward()
    assert ya.grad.abs().max().item() > 0 and yb.grad[1].abs().max().item() > 64 * yb.grad[0].abs().max().item()
    assert _same_bits(ya.grad[0], yb.grad[0])
    at = amodel.prepare_target(x)
    _, g_both = _adists_target_grad(amodel, at, y)
    _, g_one = _adists_target_grad(amodel, at[0:1], y[:1])
    assert g_one.abs().max().item() > 0 and _same_bits(g_one * 0.5, g_both[:1])


# ---- 6. errors ---------------------------------------------------------------------------------------------------------
def test_errors_of_the_interface(model, amodel, dev):
    from nerf_qa_amd._lib import NqaError
    from nerf_qa_amd.ADISTS import ADISTS
    from nerf_qa_amd.DISTS_pytorch import DISTS
    x, y = _pairs(40, 56, ("noise10", "blur"), dev)
    for cls, kw, other in ((DISTS, {"precision": "f32s"}, model), (ADISTS, {}, amodel)):
        m = cls(vgg16_path=SPEC, **kw).to(dev).eval()  # (its own instance: a weight is touched below)
        target = m.prepare_target(x)
        with pytest.raises(ValueError, match="another module"):
            other.forward_target(target, y)
        with pytest.raises(ValueError, match="shape"):
            m.forward_target(target, y[:1])
        with pytest.raises(ValueError, match="shape"):
            m.forward_target(target, y[:, :, :32])
        with pytest.raises(NqaError, match="GPU only"):
            m.forward_target(target, y.cpu())
        with pytest.raises(NqaError, match="GPU only"):
            m.prepare_target(x.cpu())
        with pytest.raises(ValueError, match="prepare_target"):
            m.prepare_target(x.clone().requires_grad_())
        with pytest.raises(ValueError):
            m.prepare_target(x[0])
        with pytest.raises(ValueError, match="prepare_target returned"):
            m.forward_target(x, y)
        # a y that requires grad with grad mode off: a value, nothing kept
        yd = y.clone().requires_grad_()
        with torch.no_grad():
            v = m.forward_target(target, yd, require_grad=True) if cls is DISTS else m.forward_target(target, yd)
        assert v.grad_fn is None and not v.requires_grad and torch.isfinite(v).all()
        if cls is DISTS:  # require_grad=False: as forward, no graph over the images (alpha / beta may still ask)
            v = m.forward_target(target, yd, batch_average=True)
            if v.requires_grad:
                v.backward()
            assert yd.grad is None
        # a stale weights key: one conv weight changed in place after preparing
        with torch.no_grad():
            m._conv_modules()[3].weight.mul_(1.0)
        with pytest.raises(ValueError, match="weights changed"):
            m.forward_target(target, y)
        m.forward_target(m.prepare_target(x), y)  # prepared again: accepted
    # a DISTS target is not an A-DISTS target
    with pytest.raises(ValueError, match="another module"):
        amodel.forward_target(model.prepare_target(x), y)
