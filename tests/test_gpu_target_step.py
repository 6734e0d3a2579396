"""The DISTS prepared-target loss step as TWO library calls (include/nqa.h, "the prepared-target loss step":
nqa_dists_target_step_forward / _backward on one caller-owned state block, csrc/nqa_loss_step.hip; DISTS(target_step="c"),
autograd.DistsTargetStep) and nqa_dists_score_backward.

What is held here:
  * through ctypes on torch buffers alone, S1, S2 and dL/dy of the two calls equal autograd.dists_target_forward /
    dists_target_backward bit for bit, on both rungs of the gradient chain;
  * DISTS(target_step="c") against the default module: loss, y.grad, alpha.grad and beta.grad bit for bit; a second backward
    (retain_graph=True) gives the first one's bits;
  * the state: the same bits whether it held 0x00 or 0xFF before the forward, and two 4 KiB guard bands around it intact
    after the forward and after the backward;
  * a whole step enqueues without one device -> host read;
  * the launches: 13 conv launches forward, the chain's alone backward, the statistics launches of the Python step;
  * a pair's gradient alone equals its gradient beside a neighbour;
  * the values against the float64 CPU oracle (score 1e-4, S1 / S2 5e-4: tests/test_gpu_dists.py's f32s constants), so that
    the file does not rest on HIP against HIP alone;
  * nqa_dists_score_backward against the float64 formula to a relative 2^-22: three float roundings of at most 2^-24
    each (w, the quotient, the product);
  * the errors of the interface.

Weights synth:1234; pairs from nerf_qa_amd/synth.py with the seeds and kinds of tests/test_gpu_target_loss.py; B = 2 with
two different kinds.  Shapes: 33x47 (every level odd: 33 17 9 5 3), 40x56 (the last tap is 3x4) and 1x1.  The Python
path's results are computed once per (shape, rung) and shared."""
import ctypes as C

import pytest
import torch

import poison

pytestmark = pytest.mark.gpu

SPEC = "synth:1234"
SCORE_TOL = 1e-4  # tests/test_gpu_dists.py SCORE_TOL["f32s"]
S_TOL = 5e-4      # tests/test_gpu_dists.py test_dists_vs_golden, s_tol of "f32s"
PAIR_SEED = {"noise10": 51, "blur": 52, "indep": 53, "nerf_white": 54, "nerf_float": 55}
CASES = [(33, 47, ("nerf_white", "indep")), (40, 56, ("noise10", "blur")), (1, 1, ("noise10", "indep"))]
RUNGS = ("f32s", "f16")
RUNG_ID = {"f32s": 3, "f16": 2}  # NQA_PREC_F32S, NQA_PREC_F16
GUARD = 4096
SHAPE_RUNG = [pytest.param(h, w, kinds, rung, id=f"{h}x{w}-{rung}") for h, w, kinds in CASES for rung in RUNGS]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def models(dev):
    """{(rung, target_step): module}, alpha and beta asking for gradients."""
    from nerf_qa_amd.DISTS_pytorch import DISTS
    out = {}
    for rung in RUNGS:
        for step in ("python", "c"):
            m = DISTS(vgg16_path=SPEC, precision="f32s", grad_precision=rung, target_step=step).to(dev).eval()
            m.alpha.requires_grad_(True)
            m.beta.requires_grad_(True)
            out[rung, step] = m
    return out


def _pairs(h, w, kinds, dev):
    from nerf_qa_amd import synth
    xn, yn = synth.frame_batch([PAIR_SEED[k] for k in kinds], h, w, list(kinds))
    return torch.from_numpy(xn).to(dev), torch.from_numpy(yn).to(dev)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _upstream(model, b, dev):
    """dL/dS1, dL/dS2 (b, 1475) of a loss that weighs pair i's score with 2^-i / b: what _weighted's backward hands down."""
    a, bt = model._score_weights()
    wgt = torch.tensor([0.5 ** i / b for i in range(b)], device=dev).reshape(b, 1)
    return (-(a.to(dev)).reshape(1, -1) * wgt).contiguous(), (-(bt.to(dev)).reshape(1, -1) * wgt).contiguous()


@pytest.fixture(scope="module")
def reference(models, dev):
    """(h, w, rung) -> (x, y, target, g1, g2, s1, s2, gy) of the Python path, computed once and left unchanged."""
    from nerf_qa_amd import autograd
    memo = {}

    def get(h, w, kinds, rung):
        if (h, w, rung) not in memo:
            m = models[rung, "python"]
            x, y = _pairs(h, w, kinds, dev)
            target = m.prepare_target(x)
            g1, g2 = _upstream(m, x.shape[0], dev)
            s1, s2, state = autograd.dists_target_forward(m, target, y)
            gy = autograd.dists_target_backward(m, target, state, g1, g2)
            assert torch.isfinite(gy).all() and gy.abs().max().item() > 0
            memo[h, w, rung] = (x, y, target, g1, g2, s1, s2, gy)
        return memo[h, w, rung]
    return get


class RawStep:
    """The two entry points through ctypes on torch buffers: a state of exactly nqa_dists_target_step_bytes between two
    guard bands of a fixed pattern, pre-filled with `fill`."""

    def __init__(self, model, rung, target, y, fill=None):
        from nerf_qa_amd import _lib, autograd
        self.lib, self.rung, self.target, self.y = _lib.lib(), RUNG_ID[rung], target, y
        dev = y.device
        self.b, _, self.h, self.w = (int(v) for v in y.shape)
        self.nbytes = int(self.lib.nqa_dists_target_step_bytes(self.b, self.h, self.w, self.rung))
        assert self.nbytes > 0
        self.buf = torch.empty(self.nbytes + 2 * GUARD, dtype=torch.uint8, device=dev)
        self.pattern = (torch.arange(GUARD, device=dev) * 37 % 251).to(torch.uint8)
        self.buf[:GUARD] = self.pattern
        self.buf[-GUARD:] = self.pattern
        self.state = self.buf[GUARD:GUARD + self.nbytes]
        if fill is not None:
            poison.fill_bytes(self.state, fill)
        self.packed = model._packed_weights(dev, "f32s")
        self.blobs, self.w0 = autograd._backward_blobs(model, dev, rung)
        self.taps = (C.c_void_p * 5)(*[t.data_ptr() for t in target.taps])
        self.layers = (C.c_void_p * 12)(*[self.blobs[l].data_ptr() for l in range(1, 13)])
        self.stream = torch.cuda.current_stream(dev).cuda_stream

    def guards_intact(self):
        return torch.equal(self.buf[:GUARD], self.pattern) and torch.equal(self.buf[-GUARD:], self.pattern)

    def forward(self):
        s1 = torch.full((self.b, 1475), float("nan"), device=self.y.device)
        s2 = torch.full_like(s1, float("nan"))
        rc = self.lib.nqa_dists_target_step_forward(self.target.x.data_ptr(), self.taps, self.y.data_ptr(), self.b, self.h,
                                                    self.w, self.packed.data_ptr(), self.rung, self.state.data_ptr(),
                                                    self.nbytes, s1.data_ptr(), s2.data_ptr(), self.stream)
        assert rc == 0, self.lib.nqa_last_error()
        return s1, s2

    def backward(self, g1, g2):
        gy = torch.full_like(self.y, float("nan"))
        rc = self.lib.nqa_dists_target_step_backward(self.target.x.data_ptr(), self.taps, self.y.data_ptr(), self.b, self.h,
                                                     self.w, g1.data_ptr(), g2.data_ptr(), self.layers, self.w0.data_ptr(),
                                                     self.rung, self.state.data_ptr(), self.nbytes, gy.data_ptr(), self.stream)
        assert rc == 0, self.lib.nqa_last_error()
        return gy


# ---- 1. the raw ABI, and what the state may hold ------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,kinds,rung", SHAPE_RUNG)
def test_raw_abi_is_the_python_step_bit_for_bit_whatever_the_state_held(h, w, kinds, rung, models, reference, dev):
    x, y, target, g1, g2, s1, s2, gy = reference(h, w, kinds, rung)
    for fill in (0x00, 0xFF):
        raw = RawStep(models[rung, "python"], rung, target, y, fill)
        r1, r2 = raw.forward()
        assert raw.guards_intact()
        assert _same_bits(r1, s1) and _same_bits(r2, s2), fill
        rg = raw.backward(g1, g2)
        assert raw.guards_intact()
        assert _same_bits(rg, gy), fill
        # the kept part is only read: a second backward on the same state, and one with another upstream gradient between
        raw.backward(g2, g1)
        assert _same_bits(raw.backward(g1, g2), rg) and raw.guards_intact()


# ---- 2. the module ------------------------------------------------------------------------------------------------------
def _module_step(m, target, y, retain=False):
    m.alpha.grad = m.beta.grad = None
    yd = y.detach().clone().requires_grad_()
    loss = m.forward_target(target, yd, require_grad=True, batch_average=True)
    loss.backward(retain_graph=retain)
    return loss, yd, m.alpha.grad.clone(), m.beta.grad.clone()


@pytest.mark.parametrize("h,w,kinds,rung", SHAPE_RUNG)
def test_module_in_c_mode_is_the_default_module_bit_for_bit(h, w, kinds, rung, models, reference, dev):
    from nerf_qa_amd import autograd
    x, y = reference(h, w, kinds, rung)[:2]
    mp, mc = models[rung, "python"], models[rung, "c"]
    assert mp.target_step == "python" and mc.target_step == "c"
    lp, yp, ap, bp = _module_step(mp, mp.prepare_target(x), y)
    tc = mc.prepare_target(x)
    lc, yc, ac, bc = _module_step(mc, tc, y, retain=True)
    assert torch.isfinite(yc.grad).all() and yc.grad.abs().max().item() > 0
    assert _same_bits(lc.detach(), lp.detach()) and _same_bits(yc.grad, yp.grad)
    assert _same_bits(ac, ap) and _same_bits(bc, bp) and ac.abs().max().item() > 0
    # a second backward through the kept graph: the first one's bits again
    first = yc.grad.clone()
    yc.grad = None
    lc.backward()
    assert _same_bits(yc.grad, first)
    # per-pair scores with per-pair upstream gradients, and the Function that ran
    yd = y.clone().requires_grad_()
    score = mc.forward_target(tc, yd, require_grad=True)
    assert score.shape == (2,) and score.requires_grad
    (score * torch.tensor([1.0, 0.5], device=dev)).sum().backward()
    yw = y.clone().requires_grad_()
    (mp.forward_target(mp.prepare_target(x), yw, require_grad=True) * torch.tensor([1.0, 0.5], device=dev)).sum().backward()
    assert _same_bits(yd.grad, yw.grad)
    s1, _ = autograd.DistsTargetStep.apply(y.clone().requires_grad_(), tc, mc)
    assert isinstance(s1.grad_fn, autograd.DistsTargetStep._backward_cls)
    # without a gradient to form the c module runs what the default module runs
    with torch.no_grad():
        assert _same_bits(mc.forward_target(tc, y), mp.forward_target(mp.prepare_target(x), y))


# ---- 3. no host read ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rung", RUNGS)
def test_c_step_enqueues_without_a_host_read(rung, models, dev):
    m = models[rung, "c"]
    x, y = _pairs(64, 80, ("noise10", "nerf_white"), dev)
    target = m.prepare_target(x)

    def step():
        yd = y.detach().clone().requires_grad_()
        loss = m.forward_target(target, yd, require_grad=True, batch_average=True)
        loss.backward()
        return loss.detach(), yd.grad

    warm = step()  # packing, the backward's weight blobs
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


# ---- 4. the launches ----------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("rung", RUNGS)
def test_c_step_runs_the_python_steps_launches(rung, models, reference, dev):
    """The launch counters are per thread and autograd runs a backward on a thread of its own, so both halves are called
    here directly, as the two Functions call them."""
    from nerf_qa_amd import autograd, ops
    x, y, target, g1, g2, s1, s2, gy = reference(40, 56, ("noise10", "blur"), rung)
    m = models[rung, "python"]
    (_, _, state), n_fwd_py, st_fwd_py = _counted(lambda: autograd.dists_target_forward(m, target, y))
    _, n_bwd_py, st_bwd_py = _counted(lambda: autograd.dists_target_backward(m, target, state, g1, g2))
    pyr = state.pyramid
    g_taps = [torch.ones_like(t) for t in pyr.taps]
    _, n_chain, _ = _counted(lambda: autograd.pyramid_backward_device(m, pyr.acts, pyr.taps, pyr.pooled, g_taps))
    blobs, w0 = autograd._backward_blobs(m, dev, rung)
    buf = autograd.dists_target_step_state(m, target)
    packed = m._packed_weights(dev, "f32s")
    (c1, c2), n_fwd, st_fwd = _counted(lambda: ops.dists_target_step_forward(target.x, target.taps, y, packed, rung, buf))
    cg, n_bwd, st_bwd = _counted(lambda: ops.dists_target_step_backward(target.x, target.taps, y, g1, g2, blobs, w0, rung, buf))
    assert n_fwd == 13 == n_fwd_py  # conv1_1 + twelve layers: ONE kept pyramid
    assert n_bwd == n_chain == n_bwd_py and n_chain > 0  # the chain's data-gradient convolutions, nothing else
    assert st_fwd == st_fwd_py and st_bwd == st_bwd_py and st_fwd > 0 and st_bwd > 0
    assert _same_bits(c1, s1) and _same_bits(c2, s2) and _same_bits(cg, gy)


# ---- 5. batch handling --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rung", RUNGS)
def test_a_pairs_gradient_does_not_depend_on_its_batch_neighbour(rung, models, dev):
    """Pair 0 alone against pair 0 next to a pair whose upstream gradient is 2^12 times larger."""
    m = models[rung, "c"]
    x, y = _pairs(33, 47, ("noise10", "nerf_float"), dev)
    target = m.prepare_target(x)
    ya = y[:1].clone().requires_grad_()
    m.forward_target(target[0:1], ya, require_grad=True).sum().backward()
    yb = y.clone().requires_grad_()
    (m.forward_target(target, yb, require_grad=True) * torch.tensor([1.0, 4096.0], device=dev)).sum().backward()
    assert ya.grad.abs().max().item() > 0 and yb.grad[1].abs().max().item() > 64 * yb.grad[0].abs().max().item()
    assert _same_bits(ya.grad[0], yb.grad[0])


# ---- 6. values ----------------------------------------------------------------------------------------------------------
def test_c_step_values_against_the_cpu_oracle(models, dev):
    from nerf_qa_amd import autograd, ops, synth
    from nerf_qa_amd.vgg_weights import load_vgg16_convs
    from oracle import dists_oracle as do
    h, w, kinds = 40, 56, ("noise10", "blur")
    xn, yn = synth.frame_batch([PAIR_SEED[k] for k in kinds], h, w, list(kinds))
    x, y = torch.from_numpy(xn).to(dev), torch.from_numpy(yn).to(dev)
    m = models["f32s", "c"]
    c64 = [(cw.double(), cb.double()) for cw, cb in load_vgg16_convs(SPEC)[0]]
    with torch.no_grad():
        w1, w2 = do.dists_stats(do.vgg_pyramid(torch.from_numpy(xn).double(), c64),
                                do.vgg_pyramid(torch.from_numpy(yn).double(), c64))
        want = do.dists_score(w1, w2, m.alpha.detach().cpu().double(), m.beta.detach().cpu().double())
    target = m.prepare_target(x)
    score = m.forward_target(target, y.clone().requires_grad_(), require_grad=True)
    assert score.requires_grad
    s1, s2 = ops.dists_target_step_forward(target.x, target.taps, y, m._packed_weights(dev, "f32s"), "f32s",
                                           autograd.dists_target_step_state(m, target))
    d = (score.detach().cpu().double() - want).abs().max().item()
    e1, e2 = (s1.cpu().double() - w1).abs().max().item(), (s2.cpu().double() - w2).abs().max().item()
    print(f"\n[c step values] DISTS {h}x{w} {'+'.join(kinds)}: |dscore| {d:.2e}  max|dS1| {e1:.2e}  max|dS2| {e2:.2e}")
    assert d <= SCORE_TOL and e1 <= S_TOL and e2 <= S_TOL, (d, e1, e2)


# ---- 7. the score's backward --------------------------------------------------------------------------------------------
def test_score_backward_against_the_float64_formula(dev):
    from nerf_qa_amd import ops
    from nerf_qa_amd.DISTS_pytorch import DISTS
    m = DISTS(vgg16_path=SPEC, precision="f32s").to(dev).eval()  # load_weights=True: the published alpha / beta
    alpha, beta = m.alpha.detach().reshape(-1), m.beta.detach().reshape(-1)
    g = torch.tensor([1.0 / 3.0, -0.7, 2.5e-3], device=dev)  # B = 3
    g1, g2 = ops.dists_score_backward(alpha, beta, g)
    assert g1.shape == g2.shape == (3, 1475)
    a64, b64, g64 = alpha.double(), beta.double(), g.double()
    w64 = a64.sum() + b64.sum()
    want1, want2 = -g64[:, None] * a64[None, :] / w64, -g64[:, None] * b64[None, :] / w64
    assert want1.abs().max().item() > 0 and want2.abs().max().item() > 0
    rel = 2.0 ** -22
    e1 = ((g1.double() - want1).abs() - rel * want1.abs()).max().item()
    e2 = ((g2.double() - want2).abs() - rel * want2.abs()).max().item()
    r1 = ((g1.double() - want1).abs() / want1.abs().clamp_min(1e-300)).max().item()
    r2 = ((g2.double() - want2).abs() / want2.abs().clamp_min(1e-300)).max().item()
    print(f"\n[score backward] max relative error: g_s1 {r1:.2e}  g_s2 {r2:.2e}  (bound {rel:.2e})")
    assert e1 <= 0 and e2 <= 0, (r1, r2)


# ---- 8. errors and the keyword ------------------------------------------------------------------------------------------
def test_errors_of_the_interface(models, dev, monkeypatch):
    import pickle
    from nerf_qa_amd import autograd
    from nerf_qa_amd._lib import NqaError
    from nerf_qa_amd.DISTS_pytorch import DISTS
    from nerf_qa_amd.DISTS_pytorch.DISTS_pt_original import DISTS as DISTS_original
    from nerf_qa_amd.DISTS_pytorch.DISTS_pt_softmax import DISTS as DISTS_softmax
    monkeypatch.delenv("NQA_TARGET_STEP", raising=False)
    for cls in (DISTS, DISTS_original, DISTS_softmax):
        with pytest.raises(ValueError, match="target_step"):
            cls(vgg16_path=SPEC, target_step="hip")
        assert cls(vgg16_path=SPEC).target_step == "python"  # the default does not move
        assert cls(vgg16_path=SPEC, target_step="c").target_step == "c"
    monkeypatch.setenv("NQA_TARGET_STEP", "c")
    assert DISTS(vgg16_path=SPEC).target_step == "c" and DISTS(vgg16_path=SPEC, target_step="python").target_step == "python"
    monkeypatch.setenv("NQA_TARGET_STEP", "graph")
    with pytest.raises(ValueError, match="target_step"):
        DISTS(vgg16_path=SPEC)
    monkeypatch.delenv("NQA_TARGET_STEP")
    mc = models["f32s", "c"]
    assert pickle.loads(pickle.dumps(mc)).target_step == "c"
    state = mc.__getstate__()
    state.pop("target_step")  # a module pickled before the keyword existed
    old = DISTS.__new__(DISTS)
    old.__setstate__(state)
    assert old.target_step == "python"
    # a state beyond the budget: the target is used whole, the error names the slices
    x, y = _pairs(40, 56, ("noise10", "blur"), dev)
    target = mc.prepare_target(x)
    need = autograd.dists_target_step_state(mc, target).numel()
    monkeypatch.setenv("NQA_MAX_WORKSPACE_GB", repr((need - 1) / 2 ** 30))
    with pytest.raises(NqaError, match=r"target\[i:j\]"):
        mc.forward_target(target, y.clone().requires_grad_(), require_grad=True)
    with torch.no_grad():  # no gradient: no state, no refusal
        assert torch.isfinite(mc.forward_target(target, y.clone().requires_grad_(), require_grad=True)).all()
    mp = models["f32s", "python"]
    assert torch.isfinite(mp.forward_target(mp.prepare_target(x), y.clone().requires_grad_(), require_grad=True)).all()
    monkeypatch.setenv("NQA_MAX_WORKSPACE_GB", repr(need / 2 ** 30))
    assert torch.isfinite(mc.forward_target(target, y.clone().requires_grad_(), require_grad=True)).all()
