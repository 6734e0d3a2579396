"""ADISTS(window_size=n) for n other than 21, at the module's surface, against oracle.adists_oracle run here on the CPU
with the same stand-in weights: scores, as_loss and as_map in f32 and f32s within the 1e-4 bar tests/test_gpu_adists.py
holds every A-DISTS mode to; NaN where the oracle gives NaN (a stage whose map is exactly one window has no unbiased
standard deviation); forward_group against the per-pair call; pair.score_pair's A-DISTS half; window_size=21 against the
default module; the refusals; and one loss step with the gradient on y, which must take the torch head.

Measured on an MI355X, f32 / f32s alike (window 21 lands at 1e-7 .. 3e-7 of the oracle):
  frame, n       score    loss     map
  40x56,  7      1.2e-7   6.0e-8   3.6e-7
  66x49, 12      1.2e-7   6.0e-8   3.0e-7
  40x56, 33      1.2e-7   6.0e-8   7.2e-7
  72x80, 63      3.0e-7   0        1.1e-6
  24x31,  4      2.4e-7   6.0e-8   3.0e-7
The loss step (40x56, n = 7, gradient on y): max err / max 2.5e-5, rms err / rms 2.5e-5 of the float64 gradient."""
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-4  # tests/test_gpu_adists.py SCORE_TOL["f32"] / ["f32s"], and its map bound
CASES = [(40, 56, 7), (66, 49, 12), (40, 56, 33), (72, 80, 63), (24, 31, 4)]
SEEDS = [3, 4, 5]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _module(dev, **kw):
    from nerf_qa_amd.ADISTS import ADISTS
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return ADISTS(**kw).to(dev).eval()


@pytest.fixture(scope="module")
def oracle(oracle_convs):
    """(h, w, n) -> (x, y, scores (B,), loss, map (B,B,h,w)) of the CPU oracle, computed once per case."""
    from nerf_qa_amd import synth
    from oracle import adists_oracle as ao
    from oracle import dists_oracle as do
    memo = {}

    def get(h, w, n):
        if (h, w, n) not in memo:
            xn, yn = synth.frame_batch(SEEDS, h, w)
            x, y = torch.from_numpy(xn), torch.from_numpy(yn)
            with torch.no_grad():
                fx, fy = do.vgg_pyramid(x, oracle_convs), do.vgg_pyramid(y, oracle_convs)
                memo[(h, w, n)] = (x, y, ao.adists_from_feats(fx, fy, n), ao.adists_from_feats(fx, fy, n, as_loss=True),
                                   ao.adists_from_feats(fx, fy, n, as_map=True))
        return memo[(h, w, n)]
    return get


@pytest.mark.parametrize("prec", ["f32", "f32s"])
@pytest.mark.parametrize("h,w,n", CASES, ids=["%dx%d-n%d" % c for c in CASES])
def test_scores_loss_and_map_against_the_oracle(h, w, n, prec, dev, oracle):
    x, y, score, loss, amap = oracle(h, w, n)
    assert torch.isfinite(score).all() and torch.isfinite(amap).all()
    m = _module(dev, window_size=n, precision=prec)
    xd, yd = x.to(dev), y.to(dev)
    got = m(xd, yd, as_loss=False)
    gl = m(xd, yd)
    gm = m(xd, yd, as_map=True)
    es = (got.cpu() - score).abs().max().item()
    el = abs(gl.item() - loss.item())
    em = (gm.cpu() - amap).abs().max().item()
    print(f"\n{h}x{w} n={n} [{prec}]: score {es:.2e}  loss {el:.2e}  map {em:.2e}")
    assert got.shape == (3,) and gl.dim() == 0 and gm.shape == amap.shape == (3, 3, h, w)
    assert es <= TOL and el <= TOL and em <= TOL
    with torch.no_grad():
        assert torch.equal(m(xd, yd, as_loss=False), got)  # repeatable


@pytest.mark.parametrize("h,w,n", [(40, 40, 5), (63, 63, 63)], ids=["40x40-n5", "63x63-n63"])
def test_nan_where_a_map_is_exactly_one_window(h, w, n, dev, oracle):
    x, y, score, loss, amap = oracle(h, w, n)
    assert torch.isnan(score).all() and torch.isnan(loss) and torch.isnan(amap).all()  # the CPU oracle, here
    m = _module(dev, window_size=n, precision="f32")
    xd, yd = x.to(dev), y.to(dev)
    assert torch.isnan(m(xd, yd, as_loss=False)).all() and torch.isnan(m(xd, yd)) and torch.isnan(m(xd, yd, as_map=True)).all()


def test_forward_group_against_the_per_pair_call(dev):
    """The figure INTEGRATION.md states for window 21: <= 6e-8, one float step."""
    from nerf_qa_amd import synth
    m = _module(dev, window_size=7, precision="f32")
    xn, _ = synth.frame_batch([3, 4], 40, 56)
    ref = torch.from_numpy(xn).to(dev)
    renders = torch.stack([torch.from_numpy(synth.frame_batch([3, 4], 40, 56, [k, k])[1]) for k in ("noise10", "blur", "noise02")],
                          dim=1).to(dev)
    got = m.forward_group(ref, renders)
    assert got.shape == (2, 3)
    for r in range(2):
        for k in range(3):
            one = m(ref[r:r + 1], renders[r, k:k + 1], as_loss=False)
            assert abs(got[r, k].item() - one.item()) <= 6e-8, (r, k, got[r, k].item(), one.item())
    assert abs(m.forward_group(ref, renders, as_loss=True).item() - got.mean().item()) <= 1e-6


def test_score_pair_and_score_group_carry_the_window(dev):
    from nerf_qa_amd import pair, synth
    from nerf_qa_amd.DISTS_pytorch import DISTS
    m = _module(dev, window_size=12, precision="f32")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        dm = DISTS().to(dev).eval()
    xn, yn = synth.frame_batch(SEEDS, 66, 49)
    x, y = torch.from_numpy(xn).to(dev), torch.from_numpy(yn).to(dev)
    for kw in ({}, {"as_loss": True}, {"as_map": True}):
        _, a = pair.score_pair(dm, m, x, y, **kw)
        assert torch.equal(a, m(x, y, **({"as_loss": False} | kw)))
    renders = torch.stack([y, x], dim=1)
    _, ag = pair.score_group(dm, m, x, renders)
    assert torch.equal(ag, m.forward_group(x, renders))
    d21 = _module(dev, precision="f32")(x, y, as_loss=False)
    assert not torch.equal(d21, m(x, y, as_loss=False))  # (the window does change the score)


def test_window_21_is_the_default_module_and_pickles(dev):
    import pickle
    from nerf_qa_amd import synth
    xn, yn = synth.frame_batch(SEEDS, 40, 56)
    x, y = torch.from_numpy(xn).to(dev), torch.from_numpy(yn).to(dev)
    a, b = _module(dev, precision="f32"), _module(dev, window_size=21, precision="f32")
    assert torch.equal(a(x, y, as_loss=False), b(x, y, as_loss=False)) and torch.equal(a(x, y, as_map=True), b(x, y, as_map=True))
    m7 = _module(dev, window_size=7, precision="f32")
    assert m7.window_size == 7 and tuple(m7.windows[1].shape) == (64, 1, 7, 7)
    back = pickle.loads(pickle.dumps(m7)).to(dev)
    assert back.window_size == 7 and torch.equal(back(x, y, as_loss=False), m7(x, y, as_loss=False))


def test_refused_window_sizes():
    from nerf_qa_amd.ADISTS import ADISTS
    for bad in (2, 64, 21.5, "21"):
        with pytest.raises(ValueError, match=r"3\.\.63"):
            ADISTS(window_size=bad)


def test_loss_step_takes_the_torch_head_and_matches_float64_autograd(dev, oracle_convs):
    """40 x 56, n = 7, gradient on y alone: with loss_head="auto" a 21-tap module takes the one-sided HIP backward; any
    other window takes the torch head.  y.grad against FLOAT64 autograd over the oracle's pyramid + head, within the
    end-to-end gradient bounds of tests/test_gpu_backward.py (rms <= 3e-3, max <= 2e-2 of the gradient's scale)."""
    from nerf_qa_amd import synth
    from oracle import adists_oracle as ao
    from oracle import dists_oracle as do
    h, w, n = 40, 56, 7
    xn, yn = synth.frame_batch([21, 22], h, w, ["noise10", "blur"])
    c64 = [(a.double(), b.double()) for a, b in oracle_convs]
    xc, yc = torch.from_numpy(xn).double(), torch.from_numpy(yn).double().requires_grad_()
    ref = ao.adists_from_feats(do.vgg_pyramid(xc, c64), do.vgg_pyramid(yc, c64), n, as_loss=True)
    ref.backward()
    m = _module(dev, window_size=n)
    assert m.loss_head == "auto"
    xd, yd = torch.from_numpy(xn).to(dev), torch.from_numpy(yn).to(dev).requires_grad_()
    got = m(xd, yd)
    assert got.requires_grad and "AdistsLossY" not in type(got.grad_fn).__name__
    y21 = torch.from_numpy(yn).to(dev).requires_grad_()
    assert "AdistsLossY" in type(_module(dev)(xd, y21).grad_fn).__name__  # (what the check above tells apart)
    assert abs(got.item() - ref.item()) <= TOL
    with torch.no_grad():
        assert abs(got.item() - m(xd, yd.detach()).item()) <= 1e-7  # the value IS the scoring path's
    got.backward()
    gd, gc = yd.grad.cpu().double(), yc.grad
    scale = gc.abs().max().item()
    err = (gd - gc).abs().max().item() / scale
    rms = (gd - gc).pow(2).mean().sqrt().item() / gc.pow(2).mean().sqrt().item()
    print(f"\nA-DISTS n={n} {h}x{w} d/dy: max|grad| {scale:.3e}  max err / max {err:.2e}  rms err / rms {rms:.2e}")
    assert torch.isfinite(gd).all() and xd.grad is None and err <= 2e-2 and rms <= 3e-3
    # a prepared target: the value works for every window, a gradient is refused with the way out
    t = m.prepare_target(xd)
    with torch.no_grad():
        v = m.forward_target(t, yd.detach())
    assert abs(v.item() - ref.item()) <= TOL
    assert m.forward_target(t, yd.detach(), as_loss=False).shape == (2,)
    with pytest.raises(ValueError, match=r"adists\(x, y\)"):
        m.forward_target(t, yd)
    from nerf_qa_amd import pair
    from nerf_qa_amd.DISTS_pytorch import DISTS
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        dm = DISTS().to(dev).eval()
    with pytest.raises(ValueError, match=r"adists\(x, y\)"):
        pair.forward_target(dm, m, t, yd)
    _, a = pair.forward_target(dm, m, t, yd.detach())
    assert abs(a.item() - v.item()) <= 1e-7
