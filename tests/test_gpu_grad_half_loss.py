"""grad_precision="f16" on the public surface: every loss step that ends in autograd.pyramid_backward_device, run once
with an f16 module and once with the default (f32s) module on the same weights, at 40x56 and 63x85 (ragged), B = 2.

What is held:
  * values: bit-equal to the default module's (the forward is untouched); alpha / beta gradients bit-equal (they do not
    pass the chain);
  * y.grad against the default module's y.grad: e_max and e_rms within grad_half_refs.HIP_FACTOR = 2 times the CPU
    emulation's figures for that shape (tests/grad_half_refs.py on the float64 oracle forward of the same pairs with
    DISTS' own tap gradients), and 1 - cosine <= 1e-5 (the cosine bar of test_gpu_backward._compare_grads; the emulation
    has <= 5e-7);
  * y.grad against float64 autograd over the CPU oracle: the existing end-to-end bounds unchanged (max <= 2e-2 of the
    largest gradient, rms <= 3e-3, cosine >= 0.99999; for the pair loss the triangle-inequality form of
    test_gpu_pair_target_loss), on pairs where the f32s path itself uses less than half of each bound -- checked here,
    its figures printed;
  * a whole step enqueues without a device -> host read; the two-sided DISTS step and the A-DISTS step with the gradient
    on x (torch head over PyramidTaps) run and meet the oracle bounds;
  * the keyword, the environment variable, pickling, and the pair rule.

Weights synth:1234; the pairs of tests/test_gpu_pair_target_loss.py."""
import functools
import pickle

import pytest
import torch

import grad_half_refs as ghr

pytestmark = pytest.mark.gpu

SPEC = "synth:1234"
DEV = "cuda:0"
PAIR_SEED = {"noise10": 51, "blur": 52, "indep": 53}
SHAPES = {(40, 56): ("noise10", "blur"), (63, 85): ("indep", "noise10")}
# the steps with a gradient towards x: at 40x56 the blur pair's d/dx has a ReLU of x's own forward on the other side in
# float32 (the f32s path alone stands at rms 5.3e-3 / max 1.0e-2 against the float64 oracle there, the f16 chain at the
# same figures): a badly chosen pair for that side, replaced by an independent one
SHAPES_X = {(40, 56): ("noise10", "indep"), (63, 85): ("indep", "noise10")}
SHAPE_IDS = ["40x56", "63x85_ragged"]


@functools.lru_cache(maxsize=None)
def _models(gp):
    from nerf_qa_amd.ADISTS import ADISTS
    from nerf_qa_amd.DISTS_pytorch import DISTS
    kw = {} if gp is None else {"grad_precision": gp}
    return (DISTS(vgg16_path=SPEC, precision="f32s", **kw).to(DEV).eval(),
            ADISTS(vgg16_path=SPEC, loss_head="auto", **kw).to(DEV).eval())


def _pairs_np(h, w, kinds=None):
    from nerf_qa_amd import synth
    kinds = kinds or SHAPES[(h, w)]
    return synth.frame_batch([PAIR_SEED[k] for k in kinds], h, w, list(kinds))


def _pairs(h, w, kinds=None):
    xn, yn = _pairs_np(h, w, kinds)
    return torch.from_numpy(xn).to(DEV), torch.from_numpy(yn).to(DEV)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@functools.lru_cache(maxsize=None)
def _oracle(h, w, kinds=None):
    """d(mean DISTS score)/d(x, y) and d(1 - mean D)/d(x, y) by float64 autograd on the CPU, once per shape and pairs."""
    from nerf_qa_amd.vgg_weights import load_vgg16_convs
    from oracle import adists_oracle as ao
    from oracle import dists_oracle as do
    convs, _ = load_vgg16_convs(SPEC)
    c64 = [(wt.double(), bs.double()) for wt, bs in convs]
    xn, yn = _pairs_np(h, w, kinds)
    xc, yc = torch.from_numpy(xn).double().requires_grad_(), torch.from_numpy(yn).double().requires_grad_()
    fx, fy = do.vgg_pyramid(xc, c64), do.vgg_pyramid(yc, c64)
    s1, s2 = do.dists_stats(fx, fy)
    m = _models(None)[0]
    d64 = do.dists_score(s1, s2, m.alpha.detach().cpu().double(), m.beta.detach().cpu().double()).mean()
    a64 = ao.adists_from_feats(fx, fy, as_loss=True)
    gdx, gdy = torch.autograd.grad(d64, (xc, yc), retain_graph=True)
    gax, gay = torch.autograd.grad(a64, (xc, yc))
    return {"dx": gdx, "dy": gdy, "ax": gax, "ay": gay}


def _emulation(h, w):
    kinds = SHAPES[(h, w)]
    return ghr.emulation_figures(h, w, kinds, tuple(PAIR_SEED[k] for k in kinds))


def _rms(t):
    return t.pow(2).mean().sqrt().item()


def _against(got, parts):
    """(e_max, e_rms, 1 - cosine) of got against sum(w * g) over parts = [(w, g64)], as fractions of the triangle-inequality
    scales sum(w max|g|), sum(w rms g) (one part: the plain per-metric figures)."""
    got = got.detach().cpu().double()
    ref = sum(wt * g for wt, g in parts)
    err = got - ref
    return (err.abs().max().item() / sum(wt * g.abs().max().item() for wt, g in parts),
            _rms(err) / sum(wt * _rms(g) for wt, g in parts), ghr.cosine_gap(got, ref))


def _check(tag, h, w, g16, g32, parts, cosine_bound=True):
    """The three statements about one gradient: f16 against f32s within twice the emulation; f32s against the oracle
    within HALF the end-to-end bounds (the pair is well chosen); f16 against the oracle within the bounds."""
    y_max, y_rms, y_cos = _emulation(h, w)
    assert torch.isfinite(g16).all() and g32.abs().max().item() > 0
    d = (g16 - g32).cpu().double()
    e_max, e_rms = d.abs().max().item() / g32.abs().max().item(), _rms(d) / _rms(g32.cpu().double())
    cgap = ghr.cosine_gap(g16, g32)
    s = _against(g32, parts)
    f = _against(g16, parts)
    print(f"\n[half loss] {tag} {h}x{w}: f16 vs f32s e_max {e_max:.2e} e_rms {e_rms:.2e} 1-cos {cgap:.2e}   (emulation "
          f"{y_max:.2e} / {y_rms:.2e} / {y_cos:.2e}; bound {ghr.HIP_FACTOR:g}x)\n"
          f"    vs float64 oracle: f32s max {s[0]:.2e} rms {s[1]:.2e} 1-cos {s[2]:.2e}   f16 max {f[0]:.2e} rms {f[1]:.2e} "
          f"1-cos {f[2]:.2e}   (bounds 2e-2 / 3e-3 / 1e-5)")
    assert s[0] <= 1e-2 and s[1] <= 1.5e-3 and (not cosine_bound or s[2] <= 0.5e-5), ("badly chosen pair", s)
    assert e_max <= ghr.HIP_FACTOR * y_max and e_rms <= ghr.HIP_FACTOR * y_rms and cgap <= 1e-5, (e_max, e_rms, cgap)
    assert f[0] <= 2e-2 and f[1] <= 3e-3 and (not cosine_bound or f[2] <= 1e-5), f


def _step(fn, y):
    """(value, y.grad) of fn(yd) summed."""
    yd = y.detach().clone().requires_grad_()
    v = fn(yd)
    v.sum().backward()
    return v.detach(), yd.grad


@pytest.mark.parametrize("path", ["dists_forward", "dists_target", "adists_forward", "adists_target"])
@pytest.mark.parametrize("h,w", list(SHAPES), ids=SHAPE_IDS)
def test_one_metric_steps(h, w, path):
    x, y = _pairs(h, w)
    out = {}
    for gp in (None, "f16"):
        dm, am = _models(gp)
        if path == "dists_forward":
            fn = lambda yd: dm.forward(x, yd, require_grad=True, batch_average=True)
        elif path == "dists_target":
            t = dm.prepare_target(x)
            fn = lambda yd: dm.forward_target(t, yd, require_grad=True, batch_average=True)
        elif path == "adists_forward":
            fn = lambda yd: am.forward(x, yd)
        else:
            t = am.prepare_target(x)
            fn = lambda yd: am.forward_target(t, yd)
        out[gp] = _step(fn, y)
    assert _same_bits(out["f16"][0], out[None][0])  # the value
    assert not _same_bits(out["f16"][1], out[None][1])  # (the f16 chain did run)
    g64 = _oracle(h, w)["dy" if path.startswith("dists") else "ay"]
    _check(path, h, w, out["f16"][1], out[None][1], [(1.0, g64)])


@pytest.mark.parametrize("wd,wa", [(1.0, 1.0), (0.25, 2.0)])
@pytest.mark.parametrize("h,w", list(SHAPES), ids=SHAPE_IDS)
def test_pair_target_step(h, w, wd, wa):
    from nerf_qa_amd import pair
    x, y = _pairs(h, w)
    out = {}
    for gp in (None, "f16"):
        dm, am = _models(gp)
        t = dm.prepare_target(x)
        yd = y.clone().requires_grad_()
        d, a = pair.forward_target(dm, am, t, yd, batch_average=True)
        (wd * d + wa * a).backward()
        out[gp] = (d.detach(), a.detach(), yd.grad)
    assert _same_bits(out["f16"][0], out[None][0]) and _same_bits(out["f16"][1], out[None][1])
    o = _oracle(h, w)
    _check(f"pair wd={wd} wa={wa}", h, w, out["f16"][2], out[None][2], [(wd, o["dy"]), (wa, o["ay"])], cosine_bound=False)


def test_alpha_and_beta_gradients_are_bit_equal():
    from nerf_qa_amd import pair
    from nerf_qa_amd.DISTS_pytorch import DISTS
    x, y = _pairs(40, 56)
    grads = {}
    for gp in (None, "f16"):
        kw = {} if gp is None else {"grad_precision": gp}
        m = DISTS(vgg16_path=SPEC, precision="f32s", **kw).to(DEV).eval()
        m.alpha.requires_grad_(True)
        m.beta.requires_grad_(True)
        am = _models(gp)[1]
        t = m.prepare_target(x)
        res = []
        for call in (lambda yd: m.forward(x, yd, require_grad=True, batch_average=True),
                     lambda yd: m.forward_target(t, yd, require_grad=True, batch_average=True),
                     lambda yd: sum(pair.forward_target(m, am, t, yd, batch_average=True))):
            m.alpha.grad = m.beta.grad = None
            yd = y.clone().requires_grad_()
            call(yd).backward()
            assert m.alpha.grad.abs().max().item() > 0 and m.beta.grad.abs().max().item() > 0
            res.append((m.alpha.grad.clone(), m.beta.grad.clone()))
        grads[gp] = res
    for (a16, b16), (a32, b32) in zip(grads["f16"], grads[None]):
        assert _same_bits(a16, a32) and _same_bits(b16, b32)


@pytest.mark.parametrize("h,w", list(SHAPES_X), ids=SHAPE_IDS)
def test_two_sided_dists_step_and_adists_step_towards_x(h, w):
    """x and y both requiring grad through DISTS, and x alone through A-DISTS (the torch head over PyramidTaps, whose
    backward is the chain): the oracle bounds, on pairs where the default module uses less than half of each."""
    kinds = SHAPES_X[(h, w)]
    x, y = _pairs(h, w, kinds)
    o = _oracle(h, w, kinds)
    got = {}
    for gp in (None, "f16"):
        dm, am = _models(gp)
        xd, yd = x.clone().requires_grad_(), y.clone().requires_grad_()
        dm.forward(xd, yd, require_grad=True, batch_average=True).backward()
        xa = x.clone().requires_grad_()
        am.forward(xa, y).backward()
        got[gp] = {"dx": xd.grad, "dy": yd.grad, "ax": xa.grad}
    for key, name in (("dx", "dists d/dx"), ("dy", "dists d/dy"), ("ax", "adists d/dx")):
        s, f = _against(got[None][key], [(1.0, o[key])]), _against(got["f16"][key], [(1.0, o[key])])
        print(f"\n[half loss] two-sided {name} {h}x{w}: vs float64 oracle f32s max {s[0]:.2e} rms {s[1]:.2e} 1-cos {s[2]:.2e}   "
              f"f16 max {f[0]:.2e} rms {f[1]:.2e} 1-cos {f[2]:.2e}")
        assert s[0] <= 1e-2 and s[1] <= 1.5e-3 and s[2] <= 0.5e-5, ("badly chosen pair", name, s)
        assert torch.isfinite(got["f16"][key]).all() and f[0] <= 2e-2 and f[1] <= 3e-3 and f[2] <= 1e-5, (name, f)


def test_a_whole_step_enqueues_without_a_host_read():
    from nerf_qa_amd import pair
    dm, am = _models("f16")
    x, y = _pairs(40, 56)
    td, ta = dm.prepare_target(x), am.prepare_target(x)

    def step():
        res = []
        for fn in (lambda yd: dm.forward_target(td, yd, require_grad=True, batch_average=True),
                   lambda yd: am.forward_target(ta, yd),
                   lambda yd: sum(pair.forward_target(dm, am, td, yd, batch_average=True))):
            res.append(_step(fn, y)[1])
        return res
    warm = step()  # packing, workspace, the half blobs, the weights comparison
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = step()
    finally:
        torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
    assert all(torch.isfinite(g).all() and _same_bits(g, wg) for g, wg in zip(got, warm))


def test_keyword_environment_pickle_and_pair_rule(monkeypatch):
    from nerf_qa_amd import pair
    from nerf_qa_amd.ADISTS import ADISTS
    from nerf_qa_amd.DISTS_pytorch import DISTS
    from nerf_qa_amd.DISTS_pytorch.DISTS_pt_original import DISTS as DISTS_original
    from nerf_qa_amd.DISTS_pytorch.DISTS_pt_softmax import DISTS as DISTS_softmax
    for cls in (DISTS, ADISTS, DISTS_original, DISTS_softmax):
        with pytest.raises(ValueError):
            cls(vgg16_path=SPEC, grad_precision="bf16")
        assert cls(vgg16_path=SPEC).grad_precision == "f32s"
        assert cls(vgg16_path=SPEC, grad_precision="f16").grad_precision == "f16"
    monkeypatch.setenv("NQA_GRAD_PRECISION", "f16")
    assert DISTS(vgg16_path=SPEC).grad_precision == "f16" and ADISTS(vgg16_path=SPEC).grad_precision == "f16"
    assert DISTS(vgg16_path=SPEC, grad_precision="f32s").grad_precision == "f32s"  # the argument wins
    monkeypatch.setenv("NQA_GRAD_PRECISION", "half")
    with pytest.raises(ValueError):
        DISTS(vgg16_path=SPEC)
    monkeypatch.delenv("NQA_GRAD_PRECISION")
    for m in _models("f16"):
        back = pickle.loads(pickle.dumps(m))
        assert back.grad_precision == "f16" and back.precision == m.precision
        state = m.__getstate__()
        state.pop("grad_precision")  # a module pickled before the keyword existed
        old = type(m).__new__(type(m))
        old.__setstate__(state)
        assert old.grad_precision == "f32s"
    dm16, am16 = _models("f16")
    dm32, am32 = _models(None)
    x, y = _pairs(40, 56)
    yd = y.clone().requires_grad_()
    for d, a in ((dm16, am32), (dm32, am16)):
        with pytest.raises(ValueError, match="grad_precision"):
            pair.forward_target(d, a, d.prepare_target(x), yd)
    # the env variable is honoured on the device too: a module constructed without the keyword runs the f16 chain
    monkeypatch.setenv("NQA_GRAD_PRECISION", "f16")
    env_model = DISTS(vgg16_path=SPEC, precision="f32s").to(DEV).eval()
    monkeypatch.delenv("NQA_GRAD_PRECISION")
    fn = lambda m: _step(lambda q: m.forward_target(m.prepare_target(x), q, require_grad=True, batch_average=True), y)[1]
    assert _same_bits(fn(env_model), fn(dm16)) and not _same_bits(fn(env_model), fn(dm32))
