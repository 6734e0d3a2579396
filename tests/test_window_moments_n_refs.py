"""tests/window_moments_n_refs.py on the CPU: the references and the bound the GPU tests of the generic-n windowed
moments (tests/test_gpu_window_moments_n.py) rely on are checked here before anything runs on a device.

  * at n = 21 the replay is what tests/test_gpu_window_moments.py uses (F.conv2d with the oracle's window in float64,
    and the full correlation with the flipped window for the transposed pass), to float64 rounding;
  * the float32 replay stays under a THIRD of the bound c(n) * 2^-24 * W[|terms|], c(n) = 128 * max(1, n / 21), on every
    case, forward and backward -- the bound leaves room for a float32 evaluation in another order;
  * every deliberately wrong replay exceeds the bound on every case it applies to; the smallest ratio of a wrong replay to
    the bound is printed (DESIGN.md 4.20 records it)."""
import pytest
import torch
import torch.nn.functional as F

import window_moments_n_refs as R


def test_replay_at_21_is_the_21_tap_tests_reference():
    from oracle import adists_oracle as ao
    n, h, w = 21, 40, 56
    x, y = R.maps(n, h, w)
    gs = R.upstream(n, h, w)
    xd, yd = x.double().requires_grad_(), y.double().requires_grad_()
    win = ao.window_2d(R.PLANES).double()
    means = [F.conv2d(p, win, groups=R.PLANES) for p in (xd, yd, xd * xd, yd * yd, xd * yd)]
    rx, ry = torch.autograd.grad(sum((m * g.double()).sum() for m, g in zip(means, gs)), (xd, yd))
    for a, b in zip(R.replay_forward(x, y, n), means):
        assert torch.equal(a, b.detach())
    gx, gy = R.replay_backward(x, y, gs, n)
    assert torch.equal(gx, rx) and torch.equal(gy, ry)
    # the transposed pass written out (what the bound is built from) is that gradient
    a = [F.conv2d(g.double(), win.flip(2, 3), padding=20, groups=R.PLANES) for g in gs]
    wx = a[0] + 2 * x.double() * a[2] + y.double() * a[4]
    assert (wx - rx).abs().max().item() <= 1e-13 * rx.abs().max().item()
    assert torch.equal(R.wt(gs[0].double(), n), a[0])


def test_taps_are_the_head_s_and_an_even_window_is_not_symmetric():
    from nerf_qa_amd.ADISTS import head
    for n in R.WINDOWS:
        t = R.taps_1d(n)
        assert torch.equal(t, head.gauss_1d(n, torch.zeros(1)))
        assert torch.equal(t, t.flip(0)) == (n % 2 == 1)
        assert int(t.argmax()) == n // 2


@pytest.mark.parametrize("n,h,w", R.CASES, ids=R.CASE_IDS)
def test_float32_replay_stays_under_a_third_of_the_bound(n, h, w):
    x, y, gs, f64, (gx64, gy64), fb, (bx, by) = R.case(n, h, w)
    f32 = R.replay_forward(x, y, n, torch.float32)
    worst = max(R.ratio(a, b, c) for a, b, c in zip(f32, f64, fb))
    gx32, gy32 = R.replay_backward(x, y, gs, n, torch.float32)
    worst_b = max(R.ratio(gx32, gx64, bx), R.ratio(gy32, gy64, by))
    print(f"\nn={n} {h}x{w}: float32 replay at {worst:.3f} (forward) and {worst_b:.3f} (backward) of the bound")
    assert worst <= 1 / 3 and worst_b <= 1 / 3


def test_every_wrong_replay_exceeds_the_bound_on_every_case():
    smallest, weak = {}, []
    for (n, h, w) in R.CASES:
        x, y, gs, _, (gx64, gy64), _, (bx, by) = R.case(n, h, w)
        for name, (applies, fn) in R.WRONG.items():
            if not applies(n, h, w):
                continue
            wx, wy = fn(x, y, gs, n)
            r = max(R.ratio(wx, gx64, bx), R.ratio(wy, gy64, by))
            if r < smallest.get(name, (float("inf"),))[0]:
                smallest[name] = (r, (n, h, w))
            if r <= 1:
                weak.append((name, n, h, w, r))
    print()
    for name, (r, c) in smallest.items():
        print(f"{name}: smallest ratio to the bound {r:.3e} at n={c[0]} {c[1]}x{c[2]}")
    print(f"smallest ratio of any wrong replay to the bound: {min(r for r, _ in smallest.values()):.3e}")
    assert set(smallest) == set(R.WRONG)
    assert not weak, weak


def test_wrong_forward_taps_and_shift_exceed_the_forward_bound():
    """The forward's own mistakes: the taps of n +- 1 and a window shifted by one, on every case."""
    low = float("inf")
    for (n, h, w) in R.CASES:
        x, y, _, f64, _, fb, _ = R.case(n, h, w)
        for m in (n - 1, n + 1):
            t = R.taps_1d(m).double()
            t = t[:n] if m > n else torch.cat([t, torch.zeros(n - m, dtype=torch.float64)])
            wrong = R.replay_forward(x, y, n, win=R.window(n, R.PLANES, torch.float64, t))
            r = max(R.ratio(a, b, c) for a, b, c in zip(wrong, f64, fb))
            low = min(low, r)
            assert r > 1, (n, h, w, m, r)
        wrong = R.replay_forward(torch.roll(x, 1, dims=-1), torch.roll(y, 1, dims=-1), n)
        r = max(R.ratio(a, b, c) for a, b, c in zip(wrong, f64, fb))
        low = min(low, r)
        assert r > 1, (n, h, w, "shift", r)
    print(f"\nsmallest ratio of a wrong forward replay to the bound: {low:.3e}")


def test_fenced_buffer_notices_what_it_should():
    f = R.Fenced((2, 3), torch.device("cpu"))
    with pytest.raises(AssertionError, match="not written"):
        f.check("nothing written")
    f.view.zero_()
    assert f.check().shape == (2, 3)
    f.buf[f.lead + f.numel] = 0.0
    with pytest.raises(AssertionError, match="past"):
        f.check("overrun")
    g = R.Fenced((5,), torch.device("cpu"), odd=True)
    assert g.lead == R.FENCE + 1
