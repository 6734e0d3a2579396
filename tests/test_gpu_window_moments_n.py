"""The generic-n HIP windowed moments (csrc/nqa_window_moments_n.hip; nqa_window_moments_forward_n / _backward_n,
ops.window_moments(window=n) / window_moments_backward(window=n)) against the float64 replay of
tests/window_moments_n_refs.py.

Bound, elementwise, in the form of tests/test_gpu_window_moments.py: c(n) * 2^-24 times the window mean of the absolute
terms, c(n) = 128 * max(1, n / 21) -- the worst-case rounding of two n-tap FMA passes plus the tap and product roundings
is about (2 n + 3) * 2^-24, 128 is 2.8 times that at n = 21 and the factor is kept as n grows;
tests/test_window_moments_n_refs.py holds the float32 CPU replay under a third of it and every wrong replay above it.

Cases (window_moments_n_refs.CASES): n in {3, 4, 12, 33, 63} and 21 forced onto the generic kernels (set_conv_variant bit
4096); P = 3 planes of different content; n x n (one output), (n + 1) x (n + 2), one output tile plus a row and a column,
and a two-tile-wide shape with W % 4 == 0.  The kernels are called at the C ABI on outputs that sit NaN-filled between
guard fences; ops' own wrappers are held bit-equal to that under a NaN fill of torch.empty (tests/poison.py)."""
import pytest
import torch

import window_moments_n_refs as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture()
def generic21():
    """n = 21 runs the generic kernels for the test's duration."""
    from nerf_qa_amd import ops
    ops.set_conv_variant(ops.DEFAULT_CONV_VARIANT | ops.CONV_MOMENTS_GENERIC)
    yield
    ops.set_conv_variant(ops.DEFAULT_CONV_VARIANT)


def _forward(x, y, n, odd=False):
    """nqa_window_moments_forward_n into a fenced, NaN-filled output: the (2 | 5, 1, P, h, w) maps."""
    from nerf_qa_amd import ops
    _, p, h, w = x.shape
    out = R.Fenced((2 if y is None else 5, 1, p, h - n + 1, w - n + 1), x.device, odd)
    ops._call(x.device, ops.lib().nqa_window_moments_forward_n, ops.ptr(x), None if y is None else ops.ptr(y), p, h, w, n,
              ops.ptr(out.view), ops.stream_ptr(x.device))
    return out.check(f"forward n={n} {h}x{w}")


def _backward(x, y, gs, n, need=(True, True), odd=False):
    from nerf_qa_amd import ops
    _, p, h, w = x.shape
    fx = R.Fenced(x.shape, x.device, odd) if need[0] else None
    fy = R.Fenced(x.shape, x.device, odd) if need[1] else None
    ops._call(x.device, ops.lib().nqa_window_moments_backward_n, ops.ptr(x), None if y is None else ops.ptr(y), p, h, w, n,
              *[None if g is None else ops.ptr(g) for g in gs], None if fx is None else ops.ptr(fx.view),
              None if fy is None else ops.ptr(fy.view), ops.stream_ptr(x.device))
    return tuple(None if f is None else f.check(f"backward n={n} {h}x{w}") for f in (fx, fy))


def _run_case(n, h, w, dev, tag=""):
    x, y, gs, f64, (gx64, gy64), fb, (bx, by) = R.case(n, h, w)
    xd, yd, gd = x.to(dev), y.to(dev), [g.to(dev) for g in gs]
    got = _forward(xd, yd, n)
    rf = max(R.ratio(got[i], f64[i], fb[i]) for i in range(5))
    one = _forward(xd, None, n)
    assert torch.equal(one[0], got[0]) and torch.equal(one[1], got[2])  # the x-only form is the pair's E[x], E[x^2]
    again = _forward(xd, yd, n)
    assert torch.equal(again, got)
    gx, gy = _backward(xd, yd, gd, n)
    rb = max(R.ratio(gx, gx64, bx), R.ratio(gy, gy64, by))
    gx1, _ = _backward(xd, yd, gd, n, need=(True, False))
    _, gy1 = _backward(xd, yd, gd, n, need=(False, True))
    assert torch.equal(gx1, gx) and torch.equal(gy1, gy)  # a null side leaves the other bit-identical
    gx2, gy2 = _backward(xd, yd, gd, n)
    assert torch.equal(gx2, gx) and torch.equal(gy2, gy)  # two runs
    # y null: the x-only backward of (g0, g2)
    gxo, _ = _backward(xd, None, [gd[0], None, gd[2], None, None], n, need=(True, False))
    rx64, _ = R.replay_backward(x, y, [gs[0], None, gs[2], None, None], n)
    bxo, _ = R.bound_backward(x, y, [gs[0], None, gs[2], None, None], n)
    ro = R.ratio(gxo, rx64, bxo)
    print(f"\nn={n}{tag} {h}x{w}: forward {rf:.3f}, backward {rb:.3f}, x-only backward {ro:.3f} of the bound "
          f"(c = {R.c_of(n):.0f} units of 2^-24)")
    assert rf <= 1 and rb <= 1 and ro <= 1, (n, h, w, rf, rb, ro)
    return got, gx, gy


GENERIC_CASES = [c for c in R.CASES if c[0] != 21]
CASES_21 = [c for c in R.CASES if c[0] == 21]


@pytest.mark.parametrize("n,h,w", GENERIC_CASES, ids=["n%d-%dx%d" % c for c in GENERIC_CASES])
def test_generic_kernels_match_the_float64_replay(n, h, w, dev):
    _run_case(n, h, w, dev)


@pytest.mark.parametrize("n,h,w", CASES_21, ids=["n%d-%dx%d" % c for c in CASES_21])
def test_21_on_the_generic_and_on_the_specialised_kernels(n, h, w, dev, generic21):
    """Both inside the bound against the same float64; the figures of both are printed."""
    from nerf_qa_amd import ops
    _run_case(n, h, w, dev, " (generic, bit 4096)")
    ops.set_conv_variant(ops.DEFAULT_CONV_VARIANT)
    _run_case(n, h, w, dev, " (21-tap kernels)")
    x, y, gs = (R.case(n, h, w)[i] for i in range(3))
    # without the bit the _n entry points ARE the 21-tap ones
    xd, yd, gd = x.to(dev), y.to(dev), [g.to(dev) for g in gs]
    assert all(torch.equal(a, b) for a, b in zip(_forward(xd, yd, n).unbind(0), ops.window_moments(xd, yd)))
    old = R.Fenced((5, 1, R.PLANES, h - 20, w - 20), dev)
    ops._call(dev, ops.lib().nqa_window_moments_forward, ops.ptr(xd), ops.ptr(yd), R.PLANES, h, w, ops.ptr(old.view),
              ops.stream_ptr(dev))
    assert torch.equal(old.check("21-tap entry point"), _forward(xd, yd, n))


def test_the_old_entry_points_ignore_bit_4096(dev, generic21):
    """nqa_window_moments_forward / _backward keep their kernels whatever the bit says: equal bits with and without."""
    from nerf_qa_amd import ops
    n, h, w = 21, 45, 85
    x, y, gs = (R.case(n, h, w)[i] for i in range(3))
    xd, yd, gd = x.to(dev), y.to(dev), [g.to(dev) for g in gs]

    def old():
        out = R.Fenced((5, 1, R.PLANES, h - 20, w - 20), dev)
        ops._call(dev, ops.lib().nqa_window_moments_forward, ops.ptr(xd), ops.ptr(yd), R.PLANES, h, w, ops.ptr(out.view),
                  ops.stream_ptr(dev))
        gx = R.Fenced(x.shape, dev)
        ops._call(dev, ops.lib().nqa_window_moments_backward, ops.ptr(xd), ops.ptr(yd), R.PLANES, h, w,
                  *[ops.ptr(g) for g in gd], ops.ptr(gx.view), None, ops.stream_ptr(dev))
        return out.check("old forward"), gx.check("old backward")
    with_bit = old()
    ops.set_conv_variant(ops.DEFAULT_CONV_VARIANT)
    without = old()
    assert torch.equal(with_bit[0], without[0]) and torch.equal(with_bit[1], without[1])


@pytest.mark.parametrize("n", [4, 12, 33, 63])
def test_dead_windows_do_not_leak(n, dev):
    """Plane 1 is zero outside a block and the upstream of E[x^2] holds 1e12 on every window that lies wholly in the zero
    region.  Live pixels, which no such window contains, must match the reference computed with those upstream entries
    set to ZERO, to the same bound -- in which no 1e12 term appears."""
    h, w = R.tile_rows(n) + 2 * n, 64 + n
    x, y = R.maps(n, h, w, seed=3)
    r0, r1, c0, c1 = n, n + 9, n + 2, n + 17  # the live block of plane 1
    keep = torch.zeros((h, w), dtype=torch.bool)
    keep[r0:r1, c0:c1] = True
    x[:, 1], y[:, 1] = (x[:, 1].abs() + 0.1) * keep, (y[:, 1].abs() + 0.1) * keep
    gs = R.upstream(n, h, w, seed=3)
    ho, wo = h - n + 1, w - n + 1
    i = torch.arange(ho).view(-1, 1).expand(ho, wo)
    j = torch.arange(wo).view(1, -1).expand(ho, wo)
    dead = (i + n - 1 < r0) | (i >= r1) | (j + n - 1 < c0) | (j >= c1)
    assert dead.any() and (~dead).any()
    clean = [g.clone() for g in gs]
    clean[2][:, 1] = torch.where(dead, torch.zeros(()), gs[2][:, 1])
    gs[2][:, 1] = torch.where(dead, torch.full((), 1e12), gs[2][:, 1])
    gx64, gy64 = R.replay_backward(x, y, clean, n)
    bx, by = R.bound_backward(x, y, clean, n)
    assert bx[:, 1, r0:r1, c0:c1].max().item() < 1.0
    gx, gy = _backward(x.to(dev), y.to(dev), [g.to(dev) for g in gs], n)
    live = (slice(None), 1, slice(r0, r1), slice(c0, c1))
    rx = R.ratio(gx.cpu()[live], gx64[live], bx[live])
    ry = R.ratio(gy.cpu()[live], gy64[live], by[live])
    # planes 0 and 2 hold no 1e12 at all and are held everywhere
    others = max(R.ratio(gx.cpu()[:, k], gx64[:, k], bx[:, k]) for k in (0, 2))
    print(f"\nn={n} dead windows: live pixels gx {rx:.3f} gy {ry:.3f}, other planes {others:.3f} of the bound")
    assert rx <= 1 and ry <= 1 and others <= 1
    assert torch.isfinite(gx).all() and torch.isfinite(gy).all()


@pytest.mark.parametrize("n,h,w", [(4, 7, 9), (12, 15, 21), (33, 35, 37)])
def test_contiguous_batch_slice_at_odd_plane_size(n, h, w, dev):
    """A contiguous batch slice at odd H * W starts off a 16-byte boundary: the scalar path takes it, with the bits of an
    aligned copy."""
    from nerf_qa_amd import ops
    g = torch.Generator().manual_seed(n)
    xs, ys = (torch.randn((3, R.PLANES, h, w), generator=g).to(dev) for _ in range(2))
    x, y = xs[1:2], ys[1:2]
    assert x.is_contiguous() and x.data_ptr() % 16 != 0 and (h * w) % 2 == 1
    xc, yc = x.clone(), y.clone()
    got, want = ops.window_moments(x, y, n), ops.window_moments(xc, yc, n)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    gs = [torch.randn_like(t) for t in want]
    gx, gy = ops.window_moments_backward(x, y, gs, window=n)
    wx, wy = ops.window_moments_backward(xc, yc, gs, window=n)
    assert torch.equal(gx, wx) and torch.equal(gy, wy)
    # and outputs that start off a 16-byte boundary themselves
    assert torch.equal(_forward(xc, yc, n, odd=True), torch.stack(want))
    ox, oy = _backward(xc, yc, gs, n, odd=True)
    assert torch.equal(ox, wx) and torch.equal(oy, wy)


@pytest.mark.parametrize("n", [4, 33])
def test_ops_and_autograd_are_the_entry_points_under_a_nan_fill(n, dev):
    import poison
    from nerf_qa_amd import _lib, ops
    from nerf_qa_amd.autograd import WindowMoments
    h, w = R.shapes_of(n)[2]
    x, y, gs = (R.case(n, h, w)[i] for i in range(3))
    xd, yd, gd = x.to(dev), y.to(dev), [g.to(dev) for g in gs]
    want, (wx, wy) = _forward(xd, yd, n), _backward(xd, yd, gd, n)
    with poison.poisoned_empty(0xFF) as hook:
        got = ops.window_moments(xd, yd, window=n)
        gx, gy = ops.window_moments_backward(xd, yd, gd, window=n)
        xa, ya = xd.clone().requires_grad_(), yd.clone().requires_grad_()
        sum((m * g).sum() for m, g in zip(WindowMoments.apply(xa, ya, n), gd)).backward()
    assert hook.filled >= 3
    assert all(torch.equal(a, b) for a, b in zip(got, want.unbind(0)))
    assert torch.equal(gx, wx) and torch.equal(gy, wy) and torch.equal(xa.grad, wx) and torch.equal(ya.grad, wy)
    with pytest.raises(_lib.NqaError):
        ops.window_moments(xd[..., : n - 1, :].contiguous(), window=n)  # no window fits: refused, never launched
    with pytest.raises(ValueError):
        ops.window_moments(xd, window=64)
