"""The A-DISTS stage backward (ops.adists_ts_backward, nqa_adists_ts_backward_n; csrc/nqa_adists_backward.hip) held to
float64 STEP BY STEP, past one block of every launch.

tests/test_gpu_adists_loss_y.py and tests/test_gpu_adists_ts_backward_n.py hold the final gradient by global norms
(max|d| / max|ref|, rms(d) / rms(ref)), because an elementwise comparison of the final gy with float64 math on the float
inputs is ill-conditioned.  A wrong value among small entries (border pixels, nearly dead channels, anything near
x == y) passes such a bar, and their cases never leave the first block of any launch.  Here every call leaves its
intermediates in a 0xFF-filled workspace that the test keeps, and each kernel is compared with a float64 replay
(tests/ts_backward_refs.py) of its own step from the DEVICE's inputs to that step, so every bound is one rounding:

  a. no 0xFF pattern is left in part, sdot, pm, mom or the fenced output;
  b. mom[0] and mom[2] are ops.window_moments' maps bit for bit (same variant bits);
  c. g1, g3, g4 (mom[1], mom[3], mom[4]) against float32(coef_replay(ops.window_moments(...))): bit-equal or the adjacent
     float, the adjacent ones at most 1e-3 of the elements;
  d. pm is ops.window_moments_backward(x, y, [None, g1, None, g3, g4], need=(False, True)) bit for bit, on the device's
     g1, g3, g4; at 72x60 and 520x508 pm and the five forward means are also held elementwise to
     window_moments_n_refs.bound_backward / bound_forward against the float64 replay.  On the plane of y filled with 1e-20,
     E[y^2] = 1e-40 is a denormal float, where a rounding errs by up to 2^-150 absolutely and not by 2^-24 relatively:
     the forward bound gets (2 n + 3) * 2^-149 added, one such term per rounding the bound's own count allows;
  e. every dot partial against the float64 block sum of pm * y: |d| <= 4096 * 2^-53 * sum |pm_i y_i|;
  f. sdot against a_y^2 * sum_k part: |d| <= (nblk + 2) * 2^-53 * a_y^2 sum |part|, exactly 0.0 on the clamped planes;
  g. gy against float32(pm - y * sdot): bit-equal or adjacent, adjacent at most 1e-3; exactly zero under the mask; the NHWC
     output is the planar one permuted; two launches are bit-equal (the whole workspace too).
The global branch is held elementwise to global_replay with the bound of ts_backward_refs.check_global.

Inputs: ReLU-like maps, one plane of y all zero and one filled with 1e-20 (clamped norm, values not zero) wherever a case
has three channels or more (the two large-plane cases have two planes and one: both stay ordinary), distinct u_b, and q /
wgt inside the head's 1475 columns at column 3 in three cases.  Each case asserts the launch geometry it is there for.

The last test turns the method round: every deliberately wrong replay of ts_backward_refs.WRONG, used as the reference
for the DEVICE's outputs, fails its step's check on every case it applies to -- these tests could have failed.

On an MI355X every check passes with no kernel changed (DESIGN.md 4.22 has the table):
  * c: 0 adjacent floats and 0 further apart among all 3 x 1 037 189 coefficients of the seven windowed cases; g: 0 among
    their 1 238 785 gradient elements.  The device's fp64 arithmetic and the replay's round to the same float everywhere;
  * e: the worst dot partial sits at 2.7e-4 of its bound (2x32x40x44), 1.6e-4 and 1.4e-4 at the two 65-partial cases;
  * f: every sdot equals the replay's double exactly, the 65-partial folds included;
  * d: pm is the window-moments backward's bits in every case; against float64 the forward means sit at 0.040 / 0.040 /
    0.051 and pm at 0.038 / 0.038 / 0.049 of window_moments_n_refs' bounds (72x60 tuned, 72x60 generic, 520x508);
  * global: 0.497 (HW = 800) and 0.499 (HW = 3844) of the bound, i.e. the one float rounding and nothing else;
  * the ten tests of the file take 4.5 s together, the slowest case (520x508) 1.3 s."""
import functools
import types

import pytest
import torch

import ts_backward_refs as T
import window_moments_n_refs as R

pytestmark = pytest.mark.gpu

FORWARD_AND_PM_HELD = ("n21-1x32x72x60", "n21-1x32x72x60_generic", "n7-1x2x520x508")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _region(raw, off, count, dtype):
    nbytes = count * torch.empty((), dtype=dtype).element_size()
    return raw[off:off + nbytes].clone().view(dtype)


def _launch(c, lay, args, dev, nhwc):
    """One call into a fenced NaN-filled output with a 0xFF-filled workspace: (gy on the CPU, the workspace's bytes)."""
    import poison
    from nerf_qa_amd import ops
    x, y, q, wgt, ps, u, coff, mask = args
    out = R.Fenced((c.B, c.H, c.W, c.C) if nhwc else (c.B, c.C, c.H, c.W), dev)
    ws = poison.PoisonWorkspace(0xFF)
    got = ops.adists_ts_backward(x, y, q, wgt, ps, u, mask, coff=coff, nhwc=nhwc, ws=ws, out=out.view, window=c.n)
    assert got.data_ptr() == out.view.data_ptr() and ws.gets == 1
    gy = out.check(f"{c.name} nhwc={nhwc}").cpu()
    (buf,) = ws.bufs.values()
    assert buf.numel() >= lay.bytes
    return gy, buf[:lay.bytes].clone()


@functools.lru_cache(maxsize=None)
def device_run(name):
    """Everything the device computes for a case, fetched once: the planar gy and the workspace regions of the first
    launch, whether the second launch, the NHWC launch and its repeat gave the same bits, ops.window_moments' five maps
    and ops.window_moments_backward's gy on the workspace's g1, g3, g4."""
    from nerf_qa_amd import ops
    c = next(c for c in T.CASES if c.name == name)
    dev = torch.device("cuda:0")
    lay = T.layout(c.B, c.C, c.H, c.W, c.n)
    assert lay.bytes == ops.lib().nqa_adists_ts_backward_bytes_n(c.B, c.C, c.H, c.W, c.n)
    k = T.make_case(c)
    args = tuple(t.to(dev).contiguous() for t in (k.x, k.y, k.q, k.wgt, k.ps, k.u)) + (k.coff, k.mask)
    r = types.SimpleNamespace(c=c, k=k, lay=lay, nhwc=c.C % 32 == 0)
    try:
        if c.generic:
            ops.set_conv_variant(ops.DEFAULT_CONV_VARIANT | ops.CONV_MOMENTS_GENERIC)
        r.gy, raw = _launch(c, lay, args, dev, False)
        gy2, raw2 = _launch(c, lay, args, dev, False)
        r.repeat = torch.equal(r.gy.view(torch.int32), gy2.view(torch.int32)) and torch.equal(raw, raw2)
        if r.nhwc:
            g3, raw3 = _launch(c, lay, args, dev, True)
            g4, _ = _launch(c, lay, args, dev, True)
            r.nhwc_equal = torch.equal(g3.permute(0, 3, 1, 2).contiguous().view(torch.int32), r.gy.view(torch.int32))
            r.nhwc_repeat = torch.equal(g3.view(torch.int32), g4.view(torch.int32))
            # (everything before the apply kernel does not know the output's layout)
            r.nhwc_ws_equal = torch.equal(raw3, raw)
        if lay.windowed:
            P, HW, hw = lay.P, lay.HW, lay.hw
            mshape = (c.B, c.C, c.H - c.n + 1, c.W - c.n + 1)
            mom_dev = _region(raw, lay.mom, 5 * P * hw, torch.float32).view(5, *mshape)
            wm = ops.window_moments(args[0], args[1], c.n)
            gs = [None, mom_dev[1].clone(), None, mom_dev[3].clone(), mom_dev[4].clone()]
            pm_again = ops.window_moments_backward(args[0], args[1], gs, need=(False, True), window=c.n)[1]
            r.wm = [m.cpu() for m in wm]
            r.pm_again = pm_again.cpu().view(P, HW)
            raw = raw.cpu()
            r.part = _region(raw, lay.part, P * lay.nblk_dot, torch.float64).view(P, lay.nblk_dot)
            r.sdot = _region(raw, lay.sdot, P, torch.float64)
            r.pm = _region(raw, lay.pm, P * HW, torch.float32).view(P, HW)
            r.mom = mom_dev.cpu()
    finally:
        ops.set_conv_variant(ops.DEFAULT_CONV_VARIANT)
    return r


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _poisoned(t):
    """Whether any element still holds the 0xFF fill (every bit set)."""
    return bool((t.view(torch.int64 if t.dtype == torch.float64 else torch.int32) == -1).any())


def _step_args(r, step):
    """(the device's output of `step`, the device's inputs to it), as ts_backward_refs.CHECKS takes them."""
    k, lay = r.k, r.lay
    if step == "global":
        return r.gy, (k.x, k.y, k.q, k.wgt, k.ps, k.u, k.coff, k.mask)
    if step == "coef":
        return (r.mom[1], r.mom[3], r.mom[4]), (r.wm, k.q, k.wgt, k.ps, k.u, k.coff)
    y = k.y.view(lay.P, lay.HW)
    if step == "dot":
        return r.part, (r.pm, y)
    if step == "fold":
        return r.sdot, (r.part, k.ay)
    assert step == "apply"
    return r.gy.view(lay.P, lay.HW), (r.pm, y, r.sdot, k.mask)


def _assert_regime(c, lay):
    """The launch geometry the case is there for, from the layout the library's byte count has confirmed."""
    vec, vec_m = c.W % 4 == 0, c.W % 4 == 0 and lay.hw % 4 == 0
    want = {
        "n7-2x32x40x44": lambda: (lay.hw, lay.nblk_coef, vec_m, lay.HW, lay.nblk_apply, lay.HW % 64) == (1292, 2, True, 1760, 2, 32),
        "n7-2x3x41x45_nomask": lambda: (lay.hw, lay.nblk_coef, vec, (lay.hw - 1024) % 4, c.mask) == (1365, 2, False, 1, False),
        "n4-1x32x36x40": lambda: (lay.hw, lay.nblk_coef, vec, vec_m) == (1221, 2, True, False),
        "n21-1x32x72x60": lambda: (lay.HW, lay.nblk_dot, lay.HW - 4096, lay.hw, lay.nblk_coef) == (4320, 2, 224, 2080, 3),
        "n7-1x2x520x508": lambda: (lay.HW, lay.nblk_dot, lay.nblk_coef, lay.P, vec) == (264160, 65, 252, 2, True),
        "n7-1x1x513x515": lambda: (lay.nblk_dot, vec, lay.HW % 4) == (65, False, 3),
        "n21-2x32x20x40_global": lambda: (lay.windowed, lay.HW, T.cdiv(lay.HW, 256), lay.HW % 256) == (False, 800, 4, 32),
        "n63-1x32x62x62_global": lambda: (lay.windowed, lay.HW) == (False, 3844),
    }[c.name.replace("_generic", "")]
    assert want(), (c.name, vars(lay))
    print(f"\n{c.name}: P {lay.P}, HW {lay.HW}, hw {lay.hw}; blocks per plane: coef {lay.nblk_coef}, dot {lay.nblk_dot}, "
          f"apply {lay.nblk_apply}; 16-byte rows {vec}, 16-byte moment planes {vec_m}; workspace {lay.bytes} bytes"
          + ("; generic kernels" if c.generic else ""))


def _layouts_and_repeats(r, bad):
    if not r.repeat:
        bad.append("two launches differ")
    if r.nhwc and not (r.nhwc_equal and r.nhwc_repeat and r.nhwc_ws_equal):
        bad.append(f"NHWC: equal to planar {r.nhwc_equal}, repeatable {r.nhwc_repeat}, same workspace {r.nhwc_ws_equal}")


@pytest.mark.parametrize("c", [c for c in T.CASES if c.H >= c.n and c.W >= c.n], ids=lambda c: c.name)
def test_windowed_stage_step_by_step(c, dev):
    lay = T.layout(c.B, c.C, c.H, c.W, c.n)
    _assert_regime(c, lay)
    r = device_run(c.name)
    k, bad = r.k, []
    # a. every region was written
    for name in ("part", "sdot", "pm", "mom"):
        t = getattr(r, name)
        if _poisoned(t) or not torch.isfinite(t).all():
            bad.append(f"a: {name} holds the fill or a non-finite number")
    # b. moments 0 and 2 are the window-moments call's
    if not (_bits_equal(r.mom[0], r.wm[0]) and _bits_equal(r.mom[2], r.wm[2])):
        bad.append("b: mom[0] / mom[2] are not ops.window_moments' bits")
    # c .. g, each on the device's inputs to the step
    for step in ("coef", "dot", "fold", "apply"):
        got, args = _step_args(r, step)
        res = T.CHECKS[step](got, *args)
        print(f"  {step}: {res.text}")
        if not res.ok:
            bad.append(f"{step}: {res.text}")
        if step == "coef":
            # d. P is the window-moments backward of the device's g1, g3, g4
            same = _bits_equal(r.pm, r.pm_again)
            print(f"  pm: {'bit-equal to' if same else 'NOT'} ops.window_moments_backward on the workspace's g1, g3, g4")
            if not same:
                bad.append("d: pm is not ops.window_moments_backward's bits")
    if c.C >= 3:  # the all-zero plane and the 1e-20 plane: a clamped norm
        z, tiny = 1, (c.B - 1) * c.C + 2
        assert (k.y.view(lay.P, -1)[z] == 0).all() and (k.y.view(lay.P, -1)[tiny] == 1e-20).all()
        assert T.clamped(k.ay)[[z, tiny]].all() and int(T.clamped(k.ay).sum()) == 2
        if not (r.sdot[z] == 0 and r.sdot[tiny] == 0):
            bad.append(f"f: sdot of the clamped planes {r.sdot[z].item()}, {r.sdot[tiny].item()}")
        if k.mask and not (r.gy.view(lay.P, -1)[z].view(torch.int32) == 0).all():
            bad.append("g: the dead plane is not exactly zero under the mask")
        if not _bits_equal(r.gy.view(lay.P, -1)[tiny], r.pm[tiny]):
            bad.append("g: the clamped 1e-20 plane is not P alone")
    _layouts_and_repeats(r, bad)
    if c.name in FORWARD_AND_PM_HELD:
        under = (2 * c.n + 3) * 2.0 ** -149
        f64, fb = R.replay_forward(k.x, k.y, c.n), R.bound_forward(k.x, k.y, c.n)
        rf = max(R.ratio(a, b, bd + under) for a, b, bd in zip(r.wm, f64, fb))
        gs = [None, r.mom[1], None, r.mom[3], r.mom[4]]
        rb = R.ratio(r.pm.view(k.y.shape), R.replay_backward(k.x, k.y, gs, c.n)[1], R.bound_backward(k.x, k.y, gs, c.n)[1])
        print(f"  window moments against float64: forward at {rf:.3f}, pm at {rb:.3f} of window_moments_n_refs' bounds")
        if not (rf <= 1 and rb <= 1):
            bad.append(f"d: forward means at {rf:.3f}, pm at {rb:.3f} of the bound")
    assert not bad, bad


@pytest.mark.parametrize("c", [c for c in T.CASES if not (c.H >= c.n and c.W >= c.n)], ids=lambda c: c.name)
def test_global_stage_elementwise(c, dev):
    lay = T.layout(c.B, c.C, c.H, c.W, c.n)
    _assert_regime(c, lay)
    r = device_run(c.name)
    k, bad = r.k, []
    got, args = _step_args(r, "global")
    res = T.check_global(got, *args)
    print(f"  {res.text}")
    if not res.ok:
        bad.append(res.text)
    z, tiny = r.gy[0, 1], r.gy[c.B - 1, 2]
    if not (z.view(torch.int32) == 0).all():
        bad.append("the dead plane is not exactly zero under the mask")
    if not (tiny != 0).any():
        bad.append("the clamped 1e-20 plane has no gradient at all")
    _layouts_and_repeats(r, bad)
    assert r.nhwc and not bad, bad


def test_every_wrong_replay_fails_on_the_device_s_outputs(dev):
    """ts_backward_refs.WRONG as the reference for what the device computed: each entry fails its step's check on every
    case it applies to (and on at least one), so a kernel that made that mistake could not pass the tests above."""
    missed = []
    for name, (step, applies, make) in T.WRONG.items():
        seen = []
        for c in T.CASES:
            lay = T.layout(c.B, c.C, c.H, c.W, c.n)
            if not applies(lay):
                continue
            got, args = _step_args(device_run(c.name), step)
            res = T.CHECKS[step](got, *args, replay=make(lay))
            seen.append(not res.ok)
            print(f"\n{name} on {c.name}: {'fails' if not res.ok else 'PASSES'} -- {res.text}")
        if not seen or not all(seen):
            missed.append((name, seen))
    assert not missed, missed
