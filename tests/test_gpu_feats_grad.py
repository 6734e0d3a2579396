"""DISTS.forward_from_feats under autograd: the HIP backward of the per-channel statistics onto caller-provided feature
maps (csrc/nqa_stats_backward.hip, autograd.FeatsSimilarities) -- the training loss of the reference's no-reference
models (nerf_qa/model_nr_v8.py:258-265).  Reference gradients: float64 torch autograd over the CPU oracle's
dists_stats / dists_score on CPU copies of the same float32 maps."""
import warnings

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CHNS = (3, 64, 128, 256, 512, 512)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev):
    from nerf_qa_amd.DISTS_pytorch import DISTS
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return DISTS(precision="f32s").to(dev).eval()


@pytest.fixture(scope="module")
def taps256(model, dev):
    """forward_once of two 256 x 256 stand-in pairs: the NR encoder's DISTS maps at their real size."""
    from nerf_qa_amd import synth
    x, y = synth.frame_batch([11, 12], 256, 256)
    with torch.no_grad():
        f0 = model.forward_once(torch.from_numpy(x).to(dev))
        f1 = model.forward_once(torch.from_numpy(y).to(dev))
    return [f.detach().clone() for f in f0], [f.detach().clone() for f in f1]


def _leaves(fs, need):
    return [f.detach().clone().requires_grad_(bool(n)) for f, n in zip(fs, need)]


def _close(got, want, what):
    """|g - g64| <= 1e-5 |g64| + 1e-6 max|g64|, elementwise over one map."""
    assert got is not None, what
    g = got.detach().cpu().double()
    assert g.shape == want.shape, (what, g.shape, want.shape)
    tol = 1e-5 * want.abs() + 1e-6 * want.abs().max()
    err = (g - want).abs()
    assert bool((err <= tol).all()), (what, int((err > tol).sum()), (err / want.abs().max().clamp_min(1e-300)).max().item())


def _ref_stats_grads(f0, f1, g1, g2, need0, need1):
    from oracle import dists_oracle as do
    x0 = [f.detach().cpu().double().requires_grad_(bool(n)) for f, n in zip(f0, need0)]
    x1 = [f.detach().cpu().double().requires_grad_(bool(n)) for f, n in zip(f1, need1)]
    s1, s2 = do.dists_stats(x0, x1)
    ((s1 * g1.cpu().double()).sum() + (s2 * g2.cpu().double()).sum()).backward()
    return [x.grad for x in x0], [x.grad for x in x1]


def _check_sims(f0, f1, need0, need1, seed=0):
    """FeatsSimilarities with random upstream dL/dS1, dL/dS2 against float64 autograd; None where not asked."""
    from nerf_qa_amd.autograd import FeatsSimilarities
    a0, a1 = _leaves(f0, need0), _leaves(f1, need1)
    s1, s2 = FeatsSimilarities.apply(*a0, *a1)
    gen = torch.Generator().manual_seed(seed)
    g1, g2 = torch.randn(s1.shape, generator=gen), torch.randn(s2.shape, generator=gen)
    grads = torch.autograd.grad((s1, s2), [t for t in a0 + a1 if t.requires_grad], (g1.to(s1.device), g2.to(s2.device)))
    r0, r1 = _ref_stats_grads(f0, f1, g1, g2, need0, need1)
    it = iter(grads)  # (in the order asked for: feats0's maps, then feats1's)
    for side, need, ref in ((0, need0, r0), (1, need1, r1)):
        for k in range(6):
            if need[k]:
                _close(next(it), ref[k], f"feats{side}[{k}]")
    # the ops layer returns None for a map that needs no gradient, and computes nothing for it
    from nerf_qa_amd import ops
    _, _, scratch = ops.dists_stats_nchw(f0, f1, keep_scratch=True)
    q0, q1 = ops.dists_stats_nchw_backward(f0, f1, scratch, g1.to(s1.device), g2.to(s1.device), need0, need1)
    for k in range(6):
        assert (q0[k] is None) == (not need0[k]) and (q1[k] is None) == (not need1[k])


ALL, NONE = (1,) * 6, (0,) * 6


@pytest.mark.parametrize("need0,need1", [(ALL, ALL), (ALL, NONE), (NONE, ALL), ((0, 1, 1, 0, 1, 1), (0, 1, 0, 1, 1, 1))],
                         ids=["both", "feats0", "feats1", "subset"])
def test_stats_grad_on_forward_once_taps(taps256, need0, need1):
    f0, f1 = taps256
    _check_sims(f0, f1, need0, need1)


def _ragged(dev, b, seed):
    dims = [(1, 1), (3, 5), (255, 3), (7, 9), (2, 2), (1, 3)]
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(b, c, h, w, generator=gen).to(dev) for c, (h, w) in zip(CHNS, dims)]


def test_stats_grad_ragged_signed(dev):
    f0, f1 = _ragged(dev, 3, 1), _ragged(dev, 3, 2)
    _check_sims(f0, f1, ALL, ALL, seed=1)


def test_stats_grad_near_identical_and_constant_planes(dev):
    gen = torch.Generator().manual_seed(3)
    dims = [(64, 64), (64, 64), (32, 32), (16, 16), (8, 8), (4, 4)]
    f0 = [torch.rand(2, c, h, w, generator=gen) * 2 for c, (h, w) in zip(CHNS, dims)]
    f1 = [f + 1e-3 * torch.randn(f.shape, generator=gen) for f in f0]  # the cancellation case: S2 near 1
    for k in (0, 2, 5):  # constant planes (zero variance) on both sides, equal and unequal levels
        f0[k][:, 1] = 0.7
        f1[k][:, 1] = 0.3
        f0[k][0, 2] = 0.5
        f1[k][0, 2] = 0.5
    _check_sims([f.to(dev) for f in f0], [f.to(dev) for f in f1], ALL, ALL, seed=3)


def _ref_score(f0, f1, alpha, beta, batch_average):
    from oracle import dists_oracle as do
    s1, s2 = do.dists_stats(f0, f1)
    return do.dists_score(s1, s2, alpha, beta, batch_average)


@pytest.mark.parametrize("batch_average", [False, True])
def test_module_gradients_with_alpha_beta(model, dev, batch_average):
    from nerf_qa_amd.DISTS_pytorch import DISTS
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = DISTS(precision="f32s").to(dev)
    f0, f1 = _ragged(dev, 2, 5), _ragged(dev, 2, 6)
    f1 = [(a + 0.3 * b).abs() for a, b in zip(f0, f1)]
    a0, a1 = _leaves(f0, ALL), _leaves(f1, ALL)
    m.zero_grad()
    score = m.forward_from_feats(a0, a1, batch_average=batch_average)
    w = torch.arange(1.0, 3.0, device=dev)
    (score.sum() if batch_average else (score * w).sum()).backward()
    # float64 reference
    r0 = [f.detach().cpu().double().requires_grad_() for f in f0]
    r1 = [f.detach().cpu().double().requires_grad_() for f in f1]
    ra = m.alpha.detach().cpu().double().requires_grad_()
    rb = m.beta.detach().cpu().double().requires_grad_()
    ref = _ref_score(r0, r1, ra, rb, batch_average)
    (ref.sum() if batch_average else (ref * w.cpu().double()).sum()).backward()
    assert (score.detach().cpu().double() - ref.detach()).abs().max().item() < 2e-6
    for k in range(6):
        _close(a0[k].grad, r0[k].grad, f"feats0[{k}]")
        _close(a1[k].grad, r1[k].grad, f"feats1[{k}]")
    for got, want, name in ((m.alpha.grad, ra.grad, "alpha"), (m.beta.grad, rb.grad, "beta")):
        assert got is not None and got.shape == want.shape, name
        assert (got.cpu().double() - want).abs().max().item() <= 1e-5 * want.abs().max().item(), name


def test_nr_loss_pattern(model, dev):
    """NRModel.losses, nerf_qa/model_nr_v8.py:258-265: an L1 between the score predicted from the decoder's maps and a
    no-grad ground-truth score, plus the batch-averaged predicted-reference-to-reference term; then .backward()."""
    from nerf_qa_amd import synth
    x, y = synth.frame_batch([21, 22], 64, 96)
    z, _ = synth.frame_batch([23, 24], 64, 96)
    with torch.no_grad():
        render_feats = model.forward_once(torch.from_numpy(y).to(dev))   # dists_feats (encoder, no grad)
        gt_feats = model.forward_once(torch.from_numpy(x).to(dev))       # gt_dists_feats
        pred0 = model.forward_once(torch.from_numpy(z).to(dev))          # stands in for the decoder's output
    pred = [p.detach().clone().requires_grad_() for p in pred0]
    coeff = 0.3
    predicted_score = model.forward_from_feats(render_feats, pred, batch_average=False)
    with torch.no_grad():
        gt_score = model.forward_from_feats(gt_feats, render_feats, batch_average=False)
    l1_loss = F.l1_loss(predicted_score, gt_score)
    pref2ref = model.forward_from_feats(pred, gt_feats, batch_average=True)
    loss = coeff * pref2ref + (1 - coeff) * l1_loss
    loss.backward()
    # float64
    alpha, beta = model.alpha.detach().cpu().double(), model.beta.detach().cpu().double()
    d = lambda fs: [f.detach().cpu().double() for f in fs]
    rp = [f.requires_grad_() for f in d(pred0)]
    ps = _ref_score(d(render_feats), rp, alpha, beta, False)
    gs = _ref_score(d(gt_feats), d(render_feats), alpha, beta, False)
    ref = coeff * _ref_score(rp, d(gt_feats), alpha, beta, True) + (1 - coeff) * (ps - gs).abs().mean()
    assert torch.equal(torch.sign(predicted_score.detach().cpu() - gt_score.cpu()), torch.sign(ps - gs).float())
    ref.backward()
    assert abs(loss.item() - ref.item()) < 2e-6
    for k in range(6):
        _close(pred[k].grad, rp[k].grad, f"pred[{k}]")


def test_values_bitwise_and_backward_repeatable(model, dev, taps256):
    from nerf_qa_amd import ops
    from nerf_qa_amd.autograd import FeatsSimilarities
    f0, f1 = taps256
    with torch.no_grad():
        n1, n2 = ops.dists_stats_nchw(f0, f1)
        s_nograd = model.forward_from_feats(f0, f1)
    a0, a1 = _leaves(f0, ALL), _leaves(f1, ALL)
    s1, s2 = FeatsSimilarities.apply(*a0, *a1)
    assert torch.equal(s1.detach(), n1) and torch.equal(s2.detach(), n2)  # the same forward kernel
    score = model.forward_from_feats(a0, a1)
    assert score.requires_grad
    assert torch.equal(score.detach(), model._weighted(n1, n2, False).detach())  # same S, same torch expression
    assert (score.detach() - s_nograd).abs().max().item() < 2e-6  # (the no-grad call's fused score kernel: fp64 sum)
    gen = torch.Generator().manual_seed(9)
    g1, g2 = torch.randn(s1.shape, generator=gen).to(dev), torch.randn(s2.shape, generator=gen).to(dev)
    first = torch.autograd.grad((s1, s2), a0 + a1, (g1, g2), retain_graph=True)
    second = torch.autograd.grad((s1, s2), a0 + a1, (g1, g2))
    for p, q in zip(first, second):
        assert torch.equal(p, q)


def test_half_and_non_contiguous_maps(dev):
    from nerf_qa_amd.autograd import FeatsSimilarities
    f0, f1 = _ragged(dev, 2, 7), _ragged(dev, 2, 8)
    gen = torch.Generator().manual_seed(4)
    s_shape = (2, sum(CHNS))
    g1, g2 = torch.randn(s_shape, generator=gen).to(dev), torch.randn(s_shape, generator=gen).to(dev)

    def grads(maps):
        s1, s2 = FeatsSimilarities.apply(*maps)
        return torch.autograd.grad((s1, s2), maps, (g1, g2))

    # half maps: the gradient comes back in half, equal to the float gradient of the same values rounded once
    h = [f.half().requires_grad_() for f in f0 + f1]
    want = grads([f.detach().float().requires_grad_() for f in h])
    for g, w, f in zip(grads(h), want, h):
        assert g.dtype == torch.float16 and g.shape == f.shape
        assert torch.equal(g, w.half())
    # channels_last and sliced maps: gradients in the maps' shapes, equal to those of contiguous copies
    base = [f.detach().clone().requires_grad_() for f in f0 + f1]
    want = grads(base)
    cl = [f.detach().to(memory_format=torch.channels_last).requires_grad_() for f in f0 + f1]
    for g, w in zip(grads(cl), want):
        assert g.shape == w.shape and torch.equal(g.contiguous(), w)
    big = [F.pad(f.detach(), (1, 2, 2, 1)).requires_grad_() for f in f0 + f1]
    sl = [b[:, :, 2:-1, 1:-2] for b in big]
    assert not any(s.is_contiguous() for s in sl[1:6])
    s1, s2 = FeatsSimilarities.apply(*sl)
    torch.autograd.backward((s1, s2), (g1, g2))
    for b, w in zip(big, want):
        assert torch.equal(b.grad[:, :, 2:-1, 1:-2], w)
        inner = torch.zeros_like(b.grad)
        inner[:, :, 2:-1, 1:-2] = b.grad[:, :, 2:-1, 1:-2]
        assert torch.equal(b.grad, inner)  # nothing outside the slice


def test_forward_and_backward_capture_into_a_graph(dev):
    from nerf_qa_amd.DISTS_pytorch import DISTS
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = DISTS(precision="f32s").to(dev)
    m.alpha.requires_grad_(False)
    m.beta.requires_grad_(False)
    f0, f1 = _ragged(dev, 2, 10), _ragged(dev, 2, 11)
    f1 = [(a + 0.5 * b) for a, b in zip(f0, f1)]
    a0, a1 = _leaves(f0, ALL), _leaves(f1, (0, 1, 1, 1, 1, 1))

    def step():
        loss = m.forward_from_feats(a0, a1, batch_average=True)
        loss.backward()
        return loss

    eager = step().detach().clone()
    eager_g = [t.grad.clone() for t in a0 + a1 if t.requires_grad]
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):  # warm-up outside capture, per the torch docs
        for _ in range(2):
            for t in a0 + a1:
                t.grad = None
            step()
    torch.cuda.current_stream(dev).wait_stream(side)
    for t in a0 + a1:
        t.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_loss = step()
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize(dev)
        assert torch.equal(static_loss, eager)
        for g, w in zip([t.grad for t in a0 + a1 if t.requires_grad], eager_g):
            assert torch.equal(g, w)
    assert a1[0].grad is None
