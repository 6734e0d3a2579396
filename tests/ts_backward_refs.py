"""Step-by-step float64 replays of the A-DISTS stage backward (csrc/nqa_adists_backward.hip, nqa_adists_ts_backward_n):
a helper module, not a test file.  include/nqa.h states the stage's arithmetic step by step, and every intermediate is
still in the caller's workspace when the call returns, so each kernel can be held on its own against float64 math on
the DEVICE's inputs to that step; every bound is then one rounding, however ill-conditioned the stage is as a whole.

  * `layout`: the byte offsets of the workspace regions, restated from ts_plan (part, sdot, pm, mom, in that order, each
    rounded up to 16 bytes; the global branch keeps nothing in its 16 bytes), and the blocks per plane of each launch.
  * `coef_replay`, `dot_replay`, `fold_replay`, `apply_replay`, `global_replay`: one step each in float64, every float
    input widened first, written as the header writes them.
  * `one_ulp_apart`, `check_ulp`: "equal bits" and "adjacent floats".  A float64 evaluation in another association or
    with other contractions can move a result across a float rounding boundary, and no further.
  * `check_coef` .. `check_global`: the check of each step, with the replay as an argument, so that the deliberately wrong
    replays of `WRONG` go through the very same code (tests/test_ts_backward_refs.py on the reference alone,
    tests/test_gpu_adists_ts_backward_steps.py on the device's outputs).
  * `make_case`: the inputs of a case, shared by the CPU and the GPU tests."""
import collections
import types

import torch

EPS = 1e-6
CLAMP = 1e12            # a_y = 1 / max(||y||, 1e-12) sits at float(1e12) where F.normalize clamps
COEF_PER_BLOCK = 1024   # map positions per block of the coefficient and planar apply kernels
DOT_PER_BLOCK = 4096    # plane elements per dot partial
U53 = 2.0 ** -53
ADJACENT_CAP = 1e-3     # share of the elements of a case that may be the adjacent float instead of the equal one


def cdiv(a, b):
    return (a + b - 1) // b


def _up16(v):
    return (v + 15) // 16 * 16


def layout(B, C, H, W, n):
    """The workspace of nqa_adists_ts_backward_n(B, C, H, W, n): byte offsets `part`, `sdot`, `pm`, `mom`, the total
    `bytes`, and P, HW, hw, nblk_dot, nblk_coef, nblk_apply (0 on the global branch, whose 16 bytes keep nothing)."""
    t = types.SimpleNamespace(windowed=H >= n and W >= n, P=B * C, HW=H * W, hw=0, nblk_dot=0, nblk_coef=0, nblk_apply=0,
                              part=0, sdot=0, pm=0, mom=0, bytes=16)
    if not t.windowed:
        return t
    t.hw = (H - n + 1) * (W - n + 1)
    t.nblk_dot, t.nblk_coef, t.nblk_apply = cdiv(t.HW, DOT_PER_BLOCK), cdiv(t.hw, COEF_PER_BLOCK), cdiv(t.HW, COEF_PER_BLOCK)
    t.sdot = t.part + _up16(8 * t.P * t.nblk_dot)
    t.pm = t.sdot + _up16(8 * t.P)
    t.mom = t.pm + _up16(4 * t.P * t.HW)
    t.bytes = t.mom + _up16(4 * 5 * t.P * t.hw)
    return t


# ---- the replays ---------------------------------------------------------------------------------------------------
def _plane_scalars(q, wgt, u, coff, C):
    """a_x, a_y, w_c (B, C) and u_b (B, 1) in float64 from q (8, B, ctot), wgt (B, ctot), u (B,)."""
    qd = q.double()
    return qd[0][:, coff:coff + C], qd[1][:, coff:coff + C], wgt.double()[:, coff:coff + C], u.double()[:, None]


def _upstreams(xm, ym, xv, yv, cov, ax, ay, A, Bc, square=True):
    """g1, g3, g4 of include/nqa.h from the normalised moments, line by line."""
    T = (2 * xm * ym + EPS) / (xm * xm + ym * ym + EPS)
    S = (2 * cov + EPS) / (xv + yv + EPS)
    dT_dym = (2 * xm - 2 * ym * T) / (xm * xm + ym * ym + EPS)
    dS_dcov = 2 / (xv + yv + EPS)
    dS_dyv = -S / (xv + yv + EPS)
    G_ym = A * dT_dym - Bc * (xm * dS_dcov + 2 * ym * dS_dyv)
    G_yy = Bc * dS_dyv
    G_xy = Bc * dS_dcov
    return ay * G_ym, (ay * ay if square else ay) * G_yy, ax * ay * G_xy


def coef_replay(mom5, q, wgt, ps, u, coff, N=None, square=True):
    """g1, g3, g4 (B, C, h, w) float64 from the five window means (B, C, h, w), q (8, B, ctot), wgt (B, ctot), ps (B, h, w)
    and u (B,).  N, square: for the wrong replays only."""
    m_x, m_y, m_xx, m_yy, m_xy = (m.double() for m in mom5)
    C = m_x.shape[1]
    ax, ay, w, ub = (t[:, :, None, None] for t in _plane_scalars(q, wgt, u, coff, C))
    N = m_x.shape[2] * m_x.shape[3] if N is None else N
    p = ps.double()[:, None]
    xm, ym = ax * m_x, ay * m_y
    xv, yv = ax * ax * m_xx - xm * xm, ay * ay * m_yy - ym * ym
    cov = ax * ay * m_xy - xm * ym
    A, Bc = ub * w * (1 - p) / N, ub * w * p / N
    return _upstreams(xm, ym, xv, yv, cov, ax, ay, A, Bc, square)


def dot_replay(pm, y, upto=None):
    """(part, mag) float64 (P, nblk): the sum of pm * y, and of |pm * y|, over elements 4096 k .. 4096 k + 4095 of each
    plane; the last block sums the tail only.  pm, y: (P, HW) float32.  upto: for the wrong replay only."""
    P, HW = pm.shape
    prod = pm.double() * y.double()  # (exact: the product of two floats fits a double)
    if upto is not None:
        prod[:, upto:] = 0
    nblk = cdiv(HW, DOT_PER_BLOCK)
    pad = torch.zeros((P, nblk * DOT_PER_BLOCK), dtype=torch.float64)
    pad[:, :HW] = prod
    pad = pad.view(P, nblk, DOT_PER_BLOCK)
    return pad.sum(dim=2), pad.abs().sum(dim=2)


def clamped(ay):
    """Where F.normalize clamps: the float a_y is at least float(1e12)."""
    return ay.float() >= torch.tensor(CLAMP, dtype=torch.float32)


def fold_replay(part, ay, upto=None, shift=0):
    """(sdot, mag) float64 (P,): a_y^2 * sum_k part[p, k], exactly 0 where the norm is clamped, and a_y^2 * sum_k |part|.
    part (P, nblk) float64, ay (P,) float32.  upto, shift: for the wrong replays only."""
    part = part.roll(shift, 0) if shift else part
    part = part[:, :upto] if upto is not None else part
    a2 = ay.double() ** 2
    live = ~clamped(ay)
    z = torch.zeros_like(a2)
    return torch.where(live, a2 * part.sum(dim=1), z), torch.where(live, a2 * part.abs().sum(dim=1), z)


def apply_replay(pm, y, sdot, mask, shift=0, rounded=True):
    """float32(float64(pm) - float64(y) * sdot[plane]) (P, HW), and exactly 0 where mask and not (y > 0).  rounded=False
    keeps the float64 (for the comparison with autograd); shift: for the wrong replay only."""
    s = sdot.roll(shift, 0) if shift else sdot
    r = pm.double() - y.double() * s[:, None]
    r = r.float() if rounded else r
    return torch.where(y > 0, r, torch.zeros_like(r)) if mask else r


def global_replay(x, y, q, wgt, ps, u, coff, mask, npix=None, two_in_sum=True):
    """The global branch from q rows 0, 1, 3..7: (gy, mag_p, mag_s) float64 (B, C, H, W), gy before its one rounding to
    float, mag_p = (|g1| + 2 |y| |g3| + |x| |g4|) / HW, mag_s = |y| a_y^2 sum_r |P(r) y(r)| (0 where the norm is clamped:
    the device multiplies nothing there).  ps (B, 1, 1).  npix, two_in_sum: for the wrong replays only."""
    B, C, H, W = x.shape
    HW = H * W
    qd = q.double()
    ax, ay, w, ub = _plane_scalars(q, wgt, u, coff, C)
    row = lambda k: qd[k][:, coff:coff + C]
    xm, ym = ax * row(3), ay * row(4)
    xv, yv, cov = ax * ax * row(5), ay * ay * row(6), ax * ay * row(7)
    p = ps.double().reshape(B, 1)
    g1, g3, g4 = (g[:, :, None, None] for g in _upstreams(xm, ym, xv, yv, cov, ax, ay, ub * w * (1 - p), ub * w * p))
    xd, yd = x.double(), y.double()
    P = (g1 + 2 * yd * g3 + xd * g4) / HW
    Ps = P if two_in_sum else (g1 + yd * g3 + xd * g4) / HW
    py = (Ps * yd).flatten(2)
    if npix is not None:
        py = py[:, :, :npix]
    live = ~clamped(q[1][:, coff:coff + C])
    a2 = torch.where(live, ay * ay, torch.zeros_like(ay))[:, :, None, None]
    sd = a2 * py.sum(dim=2)[:, :, None, None]
    gy = P - yd * sd
    if mask:
        gy = torch.where(y > 0, gy, torch.zeros_like(gy))
    mag_p = (g1.abs() + 2 * yd.abs() * g3.abs() + xd.abs() * g4.abs()) / HW
    mag_s = yd.abs() * a2 * py.abs().sum(dim=2)[:, :, None, None]
    return gy, mag_p, mag_s


# ---- the checks ----------------------------------------------------------------------------------------------------
def _key(t):
    """float32 -> int64 that orders the floats: adjacent floats differ by 1, +0 and -0 share 0."""
    b = t.contiguous().view(torch.int32).long()
    return torch.where(b < 0, -(b & 0x7FFFFFFF), b)


def one_ulp_apart(got, ref):
    """(equal, adjacent): the elementwise masks "the same bits" and "neighbouring floats" of two float32 tensors."""
    assert got.dtype == torch.float32 and ref.dtype == torch.float32 and got.shape == ref.shape
    equal = got.contiguous().view(torch.int32) == ref.contiguous().view(torch.int32)
    finite = torch.isfinite(got) & torch.isfinite(ref)
    return equal, finite & ~equal & ((_key(got) - _key(ref)).abs() == 1)


Check = collections.namedtuple("Check", "ok worst text")
# ok: the step holds; worst: the worst ratio to its bound, or the share of adjacent floats; text: one line for the log


def check_ulp(got, ref, what):
    """Every element bit-equal or the adjacent float, the adjacent ones at most ADJACENT_CAP of the elements."""
    equal, adj = one_ulp_apart(got, ref)
    far = int((~equal & ~adj).sum())
    share = int(adj.sum()) / max(got.numel(), 1)
    return Check(far == 0 and share <= ADJACENT_CAP, share,
                 f"{what}: {int(adj.sum())} adjacent of {got.numel()} ({share:.2e}), {far} further apart")


def _ratio(got, ref, bound):
    """max |got - ref| / bound, 0 / 0 = 0 and anything over a zero bound infinite; a non-finite `got` is infinite too."""
    d = (got.double() - ref).abs()
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, float("inf")))
    r = torch.where(d > 0, d / bound.clamp_min(1e-300), torch.zeros_like(d))
    return r.max().item() if r.numel() else 0.0


def check_coef(got3, mom5, q, wgt, ps, u, coff, replay=coef_replay):
    """got3: the device's g1, g3, g4 (B, C, h, w) float32; mom5: the five float32 window means they were made from."""
    res = [check_ulp(g.reshape(r.shape), r.float(), name)
           for g, r, name in zip(got3, replay(mom5, q, wgt, ps, u, coff), ("g1", "g3", "g4"))]
    return Check(all(c.ok for c in res), max(c.worst for c in res), "; ".join(c.text for c in res))


def check_dot(part, pm, y, replay=dot_replay):
    """part (P, nblk) float64 of the device against the float64 block sums of its own pm (P, HW) and y:
    |d| <= 4096 * 2^-53 * sum |pm_i y_i| over the block (the products are exact; only the additions round)."""
    ref, mag = replay(pm, y)
    assert part.shape == ref.shape, (part.shape, ref.shape)
    r = _ratio(part, ref, DOT_PER_BLOCK * U53 * mag)
    return Check(r <= 1, r, f"dot partials at {r:.3e} of 4096 * 2^-53 * sum |pm y|")


def check_fold(sdot, part, ay, replay=fold_replay):
    """sdot (P,) float64 of the device against a_y^2 * sum_k of its own partials: |d| <= (nblk + 2) * 2^-53 * a_y^2 *
    sum_k |part|, and exactly 0.0 where the norm is clamped."""
    ref, mag = replay(part, ay)
    r = _ratio(sdot, ref, (part.shape[1] + 2) * U53 * mag)
    zero = bool((sdot[clamped(ay)] == 0).all())
    return Check(r <= 1 and zero, r, f"fold at {r:.3e} of (nblk + 2) * 2^-53 * a_y^2 sum |part|; clamped planes "
                 f"{'exactly 0' if zero else 'NOT 0'}")


def check_apply(gy, pm, y, sdot, mask, replay=apply_replay):
    """gy (P, HW) float32 of the device against float32(pm - y * sdot) from its own pm and sdot."""
    c = check_ulp(gy, replay(pm, y, sdot, mask), "gy")
    zero = (not mask) or bool((gy[~(y > 0)].view(torch.int32) == 0).all())
    return Check(c.ok and zero, c.worst, c.text + ("" if zero else "; NOT +0 under the mask"))


def check_global(gy, x, y, q, wgt, ps, u, coff, mask, replay=global_replay):
    """gy (B, C, H, W) float32 of the device against the float64 replay: |d| <= 2^-23 |ref| + (HW + 8) * 2^-53 * (mag_p +
    mag_s) -- one float rounding with an ulp of slack for the boundary, the fp64 roundings of the per-pixel expression,
    and those of the HW-term sum inside sd."""
    ref, mag_p, mag_s = replay(x, y, q, wgt, ps, u, coff, mask)
    HW = x.shape[2] * x.shape[3]
    r = _ratio(gy, ref, 2.0 ** -23 * ref.abs() + (HW + 8) * U53 * (mag_p + mag_s))
    zero = (not mask) or bool((gy[~(y > 0)].view(torch.int32) == 0).all())
    return Check(r <= 1 and zero, r, f"global gy at {r:.3e} of its bound" + ("" if zero else "; NOT +0 under the mask"))


CHECKS = {"coef": check_coef, "dot": check_dot, "fold": check_fold, "apply": check_apply, "global": check_global}


# ---- deliberately wrong replays: name -> (step, applies(lay), make(lay) -> replay of that step's signature) ----------
def _repeat_block(g):
    """Positions >= 1024 of every plane repeat positions - 1024: what a coefficient kernel without its block index
    would leave there."""
    f = g.flatten(2).clone()
    f[:, :, COEF_PER_BLOCK:] = g.flatten(2)[:, :, :-COEF_PER_BLOCK]
    return f.view(g.shape)


WRONG = {
    "coef: block index dropped": (
        "coef", lambda t: t.windowed and t.nblk_coef > 1,
        lambda t: lambda *a: tuple(_repeat_block(g) for g in coef_replay(*a))),
    "coef: N = HW instead of hw": (
        "coef", lambda t: t.windowed and t.HW != t.hw, lambda t: lambda *a: coef_replay(*a, N=t.HW)),
    "coef: g3 without the square of a_y": (
        "coef", lambda t: t.windowed, lambda t: lambda *a: coef_replay(*a, square=False)),
    "fold: only partials 0..63": (
        "fold", lambda t: t.windowed and t.nblk_dot > 64, lambda t: lambda part, ay: fold_replay(part, ay, upto=64)),
    "fold: the neighbouring plane's partials": (
        "fold", lambda t: t.windowed and t.P > 1, lambda t: lambda part, ay: fold_replay(part, ay, shift=1)),
    "dot: scalar tail dropped": (
        "dot", lambda t: t.windowed and t.HW % 4 != 0, lambda t: lambda pm, y: dot_replay(pm, y, upto=t.HW // 4 * 4)),
    "apply: sdot of plane p - 1": (
        "apply", lambda t: t.windowed and t.P > 1, lambda t: lambda pm, y, s, mask: apply_replay(pm, y, s, mask, shift=1)),
    "global: only pixels 0..255 in the sum": (
        "global", lambda t: not t.windowed and t.HW > 256, lambda t: lambda *a: global_replay(*a, npix=256)),
    "global: 2 g3 in the result but not in the sum": (
        "global", lambda t: not t.windowed, lambda t: lambda *a: global_replay(*a, two_in_sum=False)),
}


# ---- the cases -----------------------------------------------------------------------------------------------------
CTOT, COFF = 1475, 3   # a stage's channels inside the head's 1475-wide q / wgt

Case = collections.namedtuple("Case", "name n B C H W mask wide generic")
CASES = [
    # two coefficient blocks on the 16-byte path (hw = 1292, a tail block of 268), two apply blocks, NHWC with HW % 64 = 32
    Case("n7-2x32x40x44", 7, 2, 32, 40, 44, True, True, False),
    # hw = 1365 = 1024 + 341, 341 % 4 = 1: the scalar path, a thread with one live position in the second block
    Case("n7-2x3x41x45_nomask", 7, 2, 3, 41, 45, False, False, False),
    # W % 4 == 0 but hw = 1221 odd: 16-byte rows, scalar moment planes, two blocks
    Case("n4-1x32x36x40", 4, 1, 32, 36, 40, True, False, False),
    # the 21-tap kernels; HW = 4320: two dot partials with a tail of 224; hw = 2080: three coefficient blocks
    Case("n21-1x32x72x60", 21, 1, 32, 72, 60, True, True, False),
    Case("n21-1x32x72x60_generic", 21, 1, 32, 72, 60, True, True, True),
    # HW = 264160: 65 dot partials, the second trip of the fold's lane loop; 252 coefficient blocks; idle fold waves
    Case("n7-1x2x520x508", 7, 1, 2, 520, 508, True, False, False),
    # the same on the scalar dot path (W % 4 != 0)
    Case("n7-1x1x513x515", 7, 1, 1, 513, 515, True, False, False),
    # global, HW = 800: four trips of the 256-stride loops, a ragged last one
    Case("n21-2x32x20x40_global", 21, 2, 32, 20, 40, True, True, False),
    # global, HW = 3844
    Case("n63-1x32x62x62_global", 63, 1, 32, 62, 62, True, False, False),
]


def make_case(c):
    """The inputs of a case on the CPU: ReLU-like maps X, Y (B, C, H, W) with -- where there are three channels or more --
    plane (0, 1) of Y all zero and plane (B - 1, 2) of Y filled with 1e-20 (a norm under F.normalize's clamp with values
    that are not zero); q from the float64 statistics of the maps, wgt = (rand + 0.5) / 1475, ps = rand, distinct u_b;
    with c.wide inside a 1475-wide q / wgt of other numbers at column 3.  Returns a namespace with coff set."""
    from test_gpu_adists_ts_backward_n import relu_maps, stage_q
    gen = torch.Generator().manual_seed(4000 + 31 * c.n + 7 * c.C + c.H)
    shape = (c.B, c.C, c.H, c.W)
    X, Y = relu_maps(shape, gen), relu_maps(shape, gen)
    if c.C >= 3:
        Y[0, 1] = 0
        Y[c.B - 1, 2] = 1e-20
    windowed = c.H >= c.n and c.W >= c.n
    ps = torch.rand((c.B, c.H - c.n + 1, c.W - c.n + 1) if windowed else (c.B, 1, 1), generator=gen)
    wgt = (torch.rand((c.B, c.C), generator=gen) + 0.5) / CTOT
    u = -(0.5 + 0.25 * torch.arange(c.B, dtype=torch.float32))
    q, coff = stage_q(X, Y), 0
    if c.wide:
        qw, ww = torch.rand((8, c.B, CTOT), generator=gen), torch.rand((c.B, CTOT), generator=gen) / CTOT
        qw[:, :, COFF:COFF + c.C], ww[:, COFF:COFF + c.C] = q, wgt
        q, wgt, coff = qw, ww, COFF
    return types.SimpleNamespace(x=X, y=Y, q=q, wgt=wgt, ps=ps, u=u, coff=coff, mask=c.mask,
                                 ay=q[1][:, coff:coff + c.C].reshape(-1).clone())
