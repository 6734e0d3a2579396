"""References for the generic-n windowed moments (csrc/nqa_window_moments_n.hip; ops.window_moments(window=n) and
ops.window_moments_backward(window=n)): a helper module, not a test file.

  * `replay_forward` / `replay_backward`: the window means of (x, y) and the gradient of <means, upstream> in float64 or
    float32 on the CPU.  The forward is F.conv2d with the oracle's window_2d(n) cast to the dtype (valid depthwise
    correlation), the backward is its autograd gradient; at n = 21 that is what tests/test_gpu_window_moments.py uses.
  * `bound_forward` / `bound_backward`: the elementwise bound, c(n) * 2^-24 times the window mean of the ABSOLUTE terms
    (forward) or W^T|g0| + 2|x| W^T|g2| + |y| W^T|g4| and its mirror (backward), c(n) = 128 * max(1, n / 21).  Two n-tap
    FMA passes plus the tap and product roundings are at most about (2 n + 3) * 2^-24 of that; 128 is 2.8 times this
    at n = 21, and the factor is kept as n grows.
  * `WRONG`: deliberately wrong float64 backward / forward replays.  Each must EXCEED the bound on every case it applies
    to (tests/test_window_moments_n_refs.py), so a kernel that made that mistake could not pass.
  * `CASES`: (n, H, W) -- per n the shapes n x n (one output), (n + 1) x (n + 2), one output tile of the kernels plus one
    row and one column (TH + n, 64 + n; TH = 24 up to n = 21, 16 above), and a shape two column tiles wide whose W is a
    multiple of 4.  P = 3 planes of different content.
  * `fenced`: an output buffer between guard fences, NaN-filled, for the GPU tests."""
import functools

import torch
import torch.nn.functional as F

WINDOWS = (3, 4, 12, 21, 33, 63)
PLANES = 3
FENCE = 64              # floats on either side of a fenced payload (a multiple of 4: the payload keeps 16-byte alignment)
FENCE_VALUE = -7.0e30


def c_of(n: int) -> float:
    return 128.0 * max(1.0, n / 21.0)


def unit(n: int) -> float:
    return c_of(n) * 2.0 ** -24


def tile_rows(n: int) -> int:
    """Rows of the kernels' tile of outputs (csrc/nqa_window_moments_n.hip, tile_rows_n)."""
    return 24 if n <= 21 else 16


def shapes_of(n: int):
    r4 = lambda v: (v + 3) // 4 * 4
    return [(n, n), (n + 1, n + 2), (tile_rows(n) + n, 64 + n), (n + 3, r4(64 + n + 4))]


CASES = [(n, h, w) for n in WINDOWS for (h, w) in shapes_of(n)]
CASE_IDS = ["n%d-%dx%d" % c for c in CASES]


def maps(n, h, w, seed=0):
    """(x, y) float32 (1, PLANES, h, w): plane 0 signed noise, the others ReLU-like with a zero band each."""
    g = torch.Generator().manual_seed(1000 * n + 7 * h + w + seed)
    x, y = torch.randn((1, PLANES, h, w), generator=g), torch.randn((1, PLANES, h, w), generator=g)
    x[:, 1:], y[:, 1:] = x[:, 1:].clamp_min(0), (0.7 * x[:, 1:] + 0.5 * y[:, 1:]).clamp_min(0)
    if h > n + 2:
        x[:, 2, : h // 4] = 0
    if w > n + 2:
        y[:, 1, :, 3 * w // 4:] = 0
    return x.contiguous(), y.contiguous()


def upstream(n, h, w, seed=0):
    """Five float32 upstream maps (1, PLANES, h-n+1, w-n+1), different per plane and per map."""
    g = torch.Generator().manual_seed(5000 * n + 11 * h + w + seed)
    return [torch.randn((1, PLANES, h - n + 1, w - n + 1), generator=g) for _ in range(5)]


def window(n, c, dtype, taps=None):
    """(c, 1, n, n): the oracle's window_2d(n) in `dtype`, or the outer product of the 1-D `taps` given."""
    if taps is None:
        from oracle import adists_oracle as ao
        return ao.window_2d(c, n).to(dtype)
    t = taps.to(dtype).unsqueeze(1)
    return t.mm(t.t()).unsqueeze(0).unsqueeze(0).expand(c, 1, n, n).contiguous()


def taps_1d(n):
    from oracle import adists_oracle as ao
    return ao.gaussian_1d(n, n / 3)


def wmean(t, n, win=None):
    return F.conv2d(t, window(n, t.shape[1], t.dtype) if win is None else win, groups=t.shape[1])


def wt(g, n, win=None):
    """W^T g: the transposed correlation, as the full correlation with the flipped window."""
    win = window(n, g.shape[1], g.dtype) if win is None else win
    return F.conv2d(g, win.flip(2, 3), padding=n - 1, groups=g.shape[1])


def terms(x, y):
    return [x, y, x * x, y * y, x * y]


def replay_forward(x, y, n, dtype=torch.float64, win=None):
    """The five window means of (x, y) in `dtype` on the CPU."""
    xd, yd = x.detach().cpu().to(dtype), y.detach().cpu().to(dtype)
    return [wmean(t, n, win) for t in terms(xd, yd)]


def replay_backward(x, y, gs, n, dtype=torch.float64, win=None):
    """(gx, gy) of sum_q <mean_q, gs[q]> (None = zero map) by autograd in `dtype` on the CPU."""
    xd = x.detach().cpu().to(dtype).requires_grad_()
    yd = y.detach().cpu().to(dtype).requires_grad_()
    means = [wmean(t, n, win) for t in terms(xd, yd)]
    loss = sum((m * g.detach().cpu().to(dtype)).sum() for m, g in zip(means, gs) if g is not None)
    gx, gy = torch.autograd.grad(loss, (xd, yd), allow_unused=True)
    z = torch.zeros_like(xd)
    return (z if gx is None else gx), (z if gy is None else gy)


def bound_forward(x, y, n):
    xd, yd = x.detach().cpu().double(), y.detach().cpu().double()
    return [unit(n) * wmean(t.abs(), n) for t in terms(xd, yd)]


def bound_backward(x, y, gs, n):
    xd, yd = x.detach().cpu().double().abs(), y.detach().cpu().double().abs()
    so = (x.shape[0], x.shape[1], x.shape[2] - n + 1, x.shape[3] - n + 1)
    a = [wt(torch.zeros(so, dtype=torch.float64) if g is None else g.detach().cpu().double().abs(), n) for g in gs]
    u = unit(n)
    return u * (a[0] + 2 * xd * a[2] + yd * a[4]), u * (a[1] + 2 * yd * a[3] + xd * a[4])


def ratio(got, ref, bound):
    """max over elements of |got - ref| / bound (0 / 0 = 0): <= 1 passes."""
    d = (got.detach().cpu().double() - ref).abs()
    r = torch.where(d > 0, d / bound.clamp_min(1e-300), torch.zeros_like(d))
    return r.max().item()


@functools.lru_cache(maxsize=None)
def case(n, h, w):
    """(x, y, gs, forward float64, backward float64 (gx, gy), forward bounds, backward bounds) of a case, computed once."""
    x, y = maps(n, h, w)
    gs = upstream(n, h, w)
    return (x, y, gs, replay_forward(x, y, n), replay_backward(x, y, gs, n), bound_forward(x, y, n),
            bound_backward(x, y, gs, n))


# ---- deliberately wrong replays: name -> (applies(n, h, w), fn(x, y, gs, n) -> (gx, gy) float64) -------------------
def _unmirrored(x, y, gs, n):
    """The transposed pass as the forward passes on the zero-padded upstream with the taps NOT mirrored (what the 21-tap
    kernel does, rightly, for its symmetric window)."""
    xd, yd = x.double(), y.double()
    w = window(n, x.shape[1], torch.float64)
    a = [F.conv2d(g.double(), w, padding=n - 1, groups=g.shape[1]) for g in gs]
    return a[0] + 2 * xd * a[2] + yd * a[4], a[1] + 2 * yd * a[3] + xd * a[4]


def _other_taps(m):
    def fn(x, y, gs, n):
        t = taps_1d(m).double()
        t = t[:n] if m > n else torch.cat([t, torch.zeros(n - m, dtype=torch.float64)])
        return replay_backward(x, y, gs, n, win=window(n, x.shape[1], torch.float64, t))
    return fn


def _shifted(x, y, gs, n):
    gx, gy = replay_backward(x, y, gs, n)
    return torch.roll(gx, 1, dims=-1), torch.roll(gy, 1, dims=-1)


def _exchanged(x, y, gs, n):
    gx, gy = replay_backward(x, y, gs, n)
    return gy, gx


def _plane0(x, y, gs, n):
    return replay_backward(x, y, [g[:, :1].expand_as(g).contiguous() for g in gs], n)


WRONG = {
    "unmirrored taps in the transposed pass": (lambda n, h, w: n % 2 == 0, _unmirrored),
    "taps of n + 1": (lambda n, h, w: True, lambda x, y, gs, n: _other_taps(n + 1)(x, y, gs, n)),
    "taps of n - 1": (lambda n, h, w: True, lambda x, y, gs, n: _other_taps(n - 1)(x, y, gs, n)),
    "window shifted by one": (lambda n, h, w: True, _shifted),
    "gx and gy exchanged": (lambda n, h, w: True, _exchanged),
    "plane 0's upstream for every plane": (lambda n, h, w: True, _plane0),
}


# ---- fenced device buffers -----------------------------------------------------------------------------------------
class Fenced:
    """A float32 device payload of `shape`, NaN-filled, between two fences of FENCE floats holding FENCE_VALUE; with
    odd=True the payload starts 4 bytes past a 16-byte boundary (for the scalar path only).  check() asserts that both
    fences are intact and that the payload holds no NaN any more."""

    def __init__(self, shape, dev, odd=False):
        numel = 1
        for s in shape:
            numel *= int(s)
        lead = FENCE + (1 if odd else 0)
        self.buf = torch.full((lead + numel + FENCE,), FENCE_VALUE, dtype=torch.float32, device=dev)
        self.view = self.buf[lead:lead + numel].view(*shape)
        self.view.fill_(float("nan"))
        self.lead, self.numel = lead, numel

    def check(self, name=""):
        assert (self.buf[:self.lead] == FENCE_VALUE).all(), f"{name}: wrote before the output"
        assert (self.buf[self.lead + self.numel:] == FENCE_VALUE).all(), f"{name}: wrote past the output"
        assert torch.isfinite(self.view).all(), f"{name}: an element of the output was not written"
        return self.view
