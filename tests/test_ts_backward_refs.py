"""tests/ts_backward_refs.py on the CPU: what tests/test_gpu_adists_ts_backward_steps.py relies on is checked here before
anything runs on a device.

  * `layout` is ts_plan: its byte count is nqa_adists_ts_backward_bytes_n's (a host-side query) over a grid of shapes and
    window sizes, every case of the GPU file among them;
  * the restated contract IS the reference's gradient: coef_replay -> float64 W^T -> dot -> fold -> apply, and
    global_replay, equal float64 autograd of the stage's D term (stage_d of tests/test_gpu_adists_ts_backward_n.py) to
    1e-10 of the largest entry, with and without the mask, with a dead plane of y among the planes;
  * the coefficient and apply replays round to the same floats when evaluated in 80-bit numpy.longdouble;
  * every deliberately wrong replay of `WRONG` fails its step's check on the reference alone (the device's output replaced
    by the right replay, rounded as the device rounds), while the right replay passes it at 0."""
import functools

import pytest
import torch

import ts_backward_refs as T
import window_moments_n_refs as R


@pytest.fixture(scope="module")
def lib():
    from nerf_qa_amd import build, _lib
    build.build()
    return _lib.lib()


def test_layout_is_the_library_s_byte_count(lib):
    shapes = [(c.B, c.C, c.H, c.W, c.n) for c in T.CASES]
    for n in (3, 4, 7, 12, 21, 33, 63):
        shapes += [(2, 3, n + 5, n + 8, n), (1, 64, n + 6, n + 9, n), (3, 5, n, n, n), (1, 1, n + 70, n + 61, n),
                   (2, 32, n - 1, n + 20, n), (1, 3, n + 2, n - 1, n)]  # odd and even W, one window, two global shapes
    for (b, c, h, w, n) in shapes:
        t = T.layout(b, c, h, w, n)
        assert t.bytes == lib.nqa_adists_ts_backward_bytes_n(b, c, h, w, n), (b, c, h, w, n)
        assert t.windowed == (h >= n and w >= n)
        if t.windowed:
            assert 0 == t.part < t.sdot < t.pm < t.mom < t.bytes and all(o % 16 == 0 for o in (t.sdot, t.pm, t.mom, t.bytes))
            assert t.sdot >= 8 * t.P * t.nblk_dot and t.pm - t.sdot >= 8 * t.P and t.mom - t.pm >= 4 * t.P * t.HW
    # 21 through the entry point without a window argument
    assert T.layout(1, 32, 72, 60, 21).bytes == lib.nqa_adists_ts_backward_bytes(1, 32, 72, 60)


def test_the_cases_reach_the_regimes_they_name():
    lay = {c.name: T.layout(c.B, c.C, c.H, c.W, c.n) for c in T.CASES}
    t = lay["n7-2x32x40x44"]
    assert (t.hw, t.nblk_coef, t.hw % 4, t.hw - 1024, t.HW, t.nblk_apply, t.HW % 64) == (1292, 2, 0, 268, 1760, 2, 32)
    t = lay["n7-2x3x41x45_nomask"]
    assert (t.hw, t.nblk_coef, (t.hw - 1024) % 4) == (1365, 2, 1)
    t = lay["n4-1x32x36x40"]
    assert (t.hw, t.hw % 2, t.nblk_coef) == (1221, 1, 2)
    t = lay["n21-1x32x72x60"]
    assert (t.HW, t.nblk_dot, t.HW - 4096, t.hw, t.nblk_coef) == (4320, 2, 224, 2080, 3)
    t = lay["n7-1x2x520x508"]
    assert (t.HW, t.nblk_dot, t.nblk_coef, t.P) == (264160, 65, 252, 2)
    t = lay["n7-1x1x513x515"]
    assert t.nblk_dot == 65 and 515 % 4 != 0 and t.HW % 4 != 0
    t = lay["n21-2x32x20x40_global"]
    assert not t.windowed and (t.HW, T.cdiv(t.HW, 256), t.HW % 256) == (800, 4, 32)
    t = lay["n63-1x32x62x62_global"]
    assert not t.windowed and t.HW == 3844


def _stage_q64(X, Y):
    """stage_q without its rounding to float: the float64 run of the reference normalises in float64."""
    xd, yd = X.double(), Y.double()
    q = torch.zeros(8, X.shape[0], X.shape[1], dtype=torch.float64)
    q[0] = 1 / xd.flatten(2).norm(dim=2).clamp_min(1e-12)
    q[1] = 1 / yd.flatten(2).norm(dim=2).clamp_min(1e-12)
    mx, my = xd.mean(dim=(2, 3)), yd.mean(dim=(2, 3))
    q[3], q[4] = mx, my
    q[5] = (xd * xd).mean(dim=(2, 3)) - mx * mx
    q[6] = (yd * yd).mean(dim=(2, 3)) - my * my
    q[7] = (xd * yd).mean(dim=(2, 3)) - mx * my
    return q


@pytest.mark.parametrize("mask", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("n,b,c,h,w", [(5, 2, 4, 9, 12), (4, 2, 3, 8, 7), (12, 2, 4, 11, 20)],
                         ids=["n5-windowed", "n4-windowed-even", "n12-global"])
def test_the_restated_contract_is_the_reference_s_gradient(n, b, c, h, w, mask):
    from test_gpu_adists_ts_backward_n import relu_maps, stage_grad
    gen = torch.Generator().manual_seed(17 * n + h)
    X, Y = relu_maps((b, c, h, w), gen), relu_maps((b, c, h, w), gen)
    Y[0, 1] = 0
    windowed = h >= n and w >= n
    ps = torch.rand((b, h - n + 1, w - n + 1) if windowed else (b, 1, 1), generator=gen)
    wgt = (torch.rand((b, c), generator=gen) + 0.5) / 1475
    u = torch.tensor([-0.7, 0.4])
    q = _stage_q64(X, Y)
    ref = stage_grad(X, Y, wgt, ps, u, mask, n, torch.float64)
    if windowed:
        win = R.window(n, c, torch.float64, R.taps_1d(n))  # the outer product in float64 of the head's float taps
        g1, g3, g4 = T.coef_replay(R.replay_forward(X, Y, n, torch.float64, win), q, wgt, ps, u, 0)
        pm = R.wt(g1, n, win) + 2 * Y.double() * R.wt(g3, n, win) + X.double() * R.wt(g4, n, win)
        pm, yf = pm.reshape(b * c, h * w), Y.reshape(b * c, h * w)
        part, _ = T.dot_replay(pm, yf)
        sdot, _ = T.fold_replay(part, q[1].reshape(-1))
        assert sdot[1] == 0 and (sdot[[0, 2]] != 0).all()
        got = T.apply_replay(pm, yf, sdot, mask, rounded=False).view(b, c, h, w)
    else:
        got, _, _ = T.global_replay(X, Y, q, wgt, ps, u, 0, mask)
    err = (got - ref).abs().max().item() / ref.abs().max().item()
    print(f"\nn={n} {b}x{c}x{h}x{w} mask={mask}: replay against float64 autograd {err:.3e} of the largest entry")
    assert got.dtype == torch.float64 and err <= 1e-10
    if mask:
        assert (got[~(Y > 0)] == 0).all()


def test_one_ulp_apart():
    a = torch.tensor([1.0, 1.0, 1.0, 0.0, -2.0, 2.0 ** -126, 3.0, float("nan")])
    b = a.clone()
    b[1] = 1.0 + 2.0 ** -23      # the next float up
    b[2] = 1.0 + 2.0 ** -22      # two floats up
    b[3] = -2.0 ** -149          # the denormal next to zero, on the other side
    b[4] = -2.0 - 2.0 ** -22     # the next float down of a negative number
    b[5] = 2.0 ** -126 - 2.0 ** -149
    b[6] = -3.0
    equal, adj = T.one_ulp_apart(a, b)
    assert equal.tolist() == [True, False, False, False, False, False, False, True]
    assert adj.tolist() == [False, True, False, True, True, True, False, False]
    c = T.check_ulp(a[:2], b[:2], "x")
    assert not c.ok and c.worst == 0.5   # an adjacent float is allowed, half of the elements are not


def test_the_float64_replays_round_as_an_80_bit_evaluation_does():
    """The reference alone sits at 0: the coefficient and apply replays in numpy.longdouble (64 bits of mantissa on x86)
    round to the same floats as the float64 ones on the 2x3x41x45 case, the clamped planes included, so an adjacent
    float on the device is the device's arithmetic and not the replay's."""
    import numpy as np
    c = next(c for c in T.CASES if c.name == "n7-2x3x41x45_nomask")
    (mom5, q, wgt, ps, u, coff), right = _step_inputs("coef", c.name)
    L = lambda t: t.numpy().astype(np.longdouble)
    m_x, m_y, m_xx, m_yy, m_xy = (L(m) for m in mom5)
    ax, ay, w = (L(t[:, coff:coff + c.C])[:, :, None, None] for t in (q[0], q[1], wgt))
    ub, p = L(u)[:, None, None, None], L(ps)[:, None]
    N = np.longdouble(m_x.shape[2] * m_x.shape[3])
    xm, ym = ax * m_x, ay * m_y
    wide = T._upstreams(xm, ym, ax * ax * m_xx - xm * xm, ay * ay * m_yy - ym * ym, ax * ay * m_xy - xm * ym, ax, ay,
                        ub * w * (1 - p) / N, ub * w * p / N)
    print(f"\nnumpy.longdouble carries {np.finfo(np.longdouble).nmant} mantissa bits here (52: the comparison is trivial)")
    for g64, g80 in zip(right, wide):
        assert np.array_equal(g64.numpy().view(np.int32), g80.astype(np.float32).view(np.int32))
    (pm, y, sdot, mask), gy = _step_inputs("apply", c.name)
    gy80 = (L(pm) - L(y) * L(sdot)[:, None]).astype(np.float32)
    assert np.array_equal(gy.numpy().view(np.int32), np.where(y.numpy() > 0, gy80, np.float32(0)).view(np.int32) if mask
                          else gy80.view(np.int32))


# ---- every wrong replay fails its step's check on the reference alone ----------------------------------------------
@functools.lru_cache(maxsize=None)
def _step_inputs(step, name):
    """The inputs of `step` for the case `name`, and the right replay's output in the device's number format."""
    c = next(c for c in T.CASES if c.name == name)
    t = T.layout(c.B, c.C, c.H, c.W, c.n)
    gen = torch.Generator().manual_seed(len(name) + 100 * c.H)
    if step in ("coef", "global"):
        k = T.make_case(c)
        if step == "global":
            args = (k.x, k.y, k.q, k.wgt, k.ps, k.u, k.coff, k.mask)
            return args, T.global_replay(*args)[0].float()
        mom5 = tuple(m.float() for m in R.replay_forward(k.x, k.y, c.n))
        args = (mom5, k.q, k.wgt, k.ps, k.u, k.coff)
        return args, tuple(g.float() for g in T.coef_replay(*args))
    pm = torch.randn((t.P, t.HW), generator=gen)
    y = torch.rand((t.P, t.HW), generator=gen).sub_(0.3).clamp_(min=0)
    y[:, -1] = 0.25  # (the last element of a plane is what a dropped tail drops)
    if step == "dot":
        return (pm, y), T.dot_replay(pm, y)[0]
    if step == "fold":
        part = torch.randn((t.P, t.nblk_dot), generator=gen, dtype=torch.float64)
        ay = torch.rand((t.P,), generator=gen) + 0.5
        return (part, ay), T.fold_replay(part, ay)[0]
    assert step == "apply"
    sdot = torch.randn((t.P,), generator=gen, dtype=torch.float64)
    return (pm, y, sdot, c.mask), T.apply_replay(pm, y, sdot, c.mask)


def _cases_of(applies, step):
    for c in T.CASES:
        t = T.layout(c.B, c.C, c.H, c.W, c.n)
        # (the moments of the generic case are those of its twin, and the two 21-tap replays take a second each: one
        # case with three coefficient blocks is enough here; the device's outputs go through all of them)
        if applies(t) and not c.generic and not (step == "coef" and c.n == 21):
            yield c, t


@pytest.mark.parametrize("name", list(T.WRONG), ids=[k.replace(" ", "_") for k in T.WRONG])
def test_a_wrong_replay_fails_its_check_on_the_reference_alone(name):
    step, applies, make = T.WRONG[name]
    failed, seen = [], 0
    for c, t in _cases_of(applies, step):
        args, right = _step_inputs(step, c.name)
        ok = T.CHECKS[step](right, *args)
        # the right replay against itself: at 0, or (the global bound, whose first term is two half-ulps of a float, on
        # the replay rounded to float) at a half
        assert ok.ok and ok.worst <= (0.5 if step == "global" else 0), (c.name, ok)
        res = T.CHECKS[step](right, *args, replay=make(t))
        print(f"\n{name} on {c.name}: {'FAILS its check' if not res.ok else 'passes'} -- {res.text}")
        seen += 1
        if not res.ok:
            failed.append(c.name)
    assert seen and failed, f"{name}: no case it applies to notices it"
    assert len(failed) == seen, (name, failed)  # in fact every case it applies to does
