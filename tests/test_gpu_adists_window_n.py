"""The generic A-DISTS window pass -- adists_window_n_lanes_kernel, adists_window_n_planar_kernel and their group forms
(csrc/nqa_window_n.h), through ops.adists_window_stage(window=n) / ops.adists_window_stage_group(window=n), which launch
one stage exactly as the forwards do -- held to a float64 replay of the same stage for a general window size
(tests/window_n_refs.py): n in {3, 4, 12, 21 forced onto the generic kernels, 33, 63}; planes, 64 and 128 channels;
float, f16 and bf16 taps; B = 2 with different q / wgt per image; groups of K = 3; one-row, one-column and one-element
maps (H = n, W = n); one output row and one column more than a block covers; forced strips with 64-row groups over two
channel blocks; and H = n - 1 or W = n - 1, which must take the global branch.

Bound, per map (gamma, tw, sw; all images of the case): max|hip - r64| / max|r64| <= max(8 x e32, 16 x 2^-24), e32 being
the float32 replay's own distance from r64 for that map (window_refs.YARD, FLOOR).  Every call also runs with NaN-filled
outputs between guard regions (every element written, nothing else touched) and twice (bit-identical).  At n = 21 the
specialised kernels run on the same inputs and must sit inside the same bound against the same r64.

Measured on an MI355X (all 43 cases pass):
  kernel family                     largest error (of the map's maximum): gamma  tw  sw     largest error / bound
  lanes, float taps (15 cases)      2.9e-7  1.3e-7  2.1e-7                                   0.16
  lanes, f16 / bf16 taps (6)        2.6e-7  1.1e-7  2.0e-7                                   0.16
  planes, C = 3 (9)                 1.1e-6  2.8e-7  1.2e-6                                   0.15
  group forms, K = 3 (7)            1.2e-6  2.2e-7  1.2e-6                                   0.14
  global branch (5)                 2.7e-8  7.7e-8  3.7e-8                                   0.08
  n = 21, generic / specialised     1.8e-7 / 1.3e-7 (C = 128)   6.9e-7 / 7.2e-7 (planes)     0.14 / 0.15
No case is above a sixth of its bound; the generic kernels sit about as far from float64 as the float32 replay itself
and as the specialised 21-tap kernels on the same inputs.
tests/test_window_n_refs.py recomputes e32 without a GPU and shows that every wrong replay (taps of n - 1 / n + 1,
sigma 7, rotated vertical taps, a shifted window, y from x, image 0's scalars, a mirrored even window) sits at least 61
times above the largest bound of any case (2.5e-5) on every case it applies to."""
import pytest
import torch

import window_n_refs as N
import window_refs as R21

pytestmark = pytest.mark.gpu

GUARD = 1 << 14  # floats on every side of every output map
FENCE = -1234.5


@pytest.fixture(scope="module")
def refs():
    return {N.case_id(c): N.references(c) for c in N.CASES}


def _device_taps(case, x, y, dev):
    if case.C == 3:
        return x.to(dev).contiguous(), y.to(dev).contiguous()
    return x.permute(0, 2, 3, 1).contiguous().to(dev), y.permute(0, 2, 3, 1).contiguous().to(dev)


def _call(case, fx, fy, q, wgt, window, maps=None):
    from nerf_qa_amd import ops
    if maps is None:
        if case.K:
            return ops.adists_window_stage_group(fx, fy, q, wgt, case.prec, case.strip, window=window)
        return ops.adists_window_stage(fx, fy, q, wgt, case.prec, case.strip, window=window)
    if case.K:
        ops.adists_window_stage_group(fx, fy, q, wgt, case.prec, case.strip, window=window, out=tuple(maps))
    else:
        ops.adists_window_stage_into(fx, fy, q, wgt, case.prec, case.strip, *maps, window=window)


def _run(case, fx, fy, q, wgt, shapes, window):
    """One call into NaN-filled maps fenced on every side: (maps, whether the fences survived)."""
    ns = [s[0] * s[1] * s[2] for s in shapes]
    buf = torch.full((4 * GUARD + sum(ns),), FENCE, dtype=torch.float32, device=fx.device)
    maps, inside, off = [], torch.zeros_like(buf, dtype=torch.bool), GUARD
    for s, n in zip(shapes, ns):
        m = buf[off:off + n].view(s)
        m.fill_(float("nan"))
        inside[off:off + n] = True
        maps.append(m)
        off += n + GUARD
    _call(case, fx, fy, q, wgt, window, maps)
    torch.cuda.synchronize()
    return [m.clone() for m in maps], bool((buf[~inside] == FENCE).all())


@pytest.mark.parametrize("case", N.CASES, ids=N.case_id)
def test_stage_against_float64_replay(case, refs):
    from nerf_qa_amd import ops
    dev = torch.device("cuda:0")
    (x, y, q, wgt), r64, e32 = refs[N.case_id(case)]
    fx, fy = _device_taps(case, x, y, dev)
    q, wgt = q.to(dev), wgt.to(dev)
    shapes = [tuple(r.shape) for r in r64]
    windowed = case.H >= case.n and case.W >= case.n
    assert (case.kind == "global") == (not windowed)
    try:
        if case.generic:
            ops.set_conv_variant(ops.DEFAULT_CONV_VARIANT | ops.CONV_WINDOW_GENERIC)
            assert ops.adists_window_grid(case.B, case.H, case.W, case.C, case.prec, 0) == (0, 0, 0)  # no LDS kernel
        first, intact = _run(case, fx, fy, q, wgt, shapes, case.n)
        second, _ = _run(case, fx, fy, q, wgt, shapes, case.n)
        plain = _call(case, fx, fy, q, wgt, case.n)
    finally:
        ops.set_conv_variant(ops.DEFAULT_CONV_VARIANT)
    figs, ok = R21.check(first, r64, e32)
    print("%s: " % N.case_id(case) + "  ".join("%s %.2e / %.2e (%.2f)" % (n, e, b, e / b if b else float("inf"))
                                               for n, (e, b) in zip(("gamma", "tw", "sw"), figs)))
    assert intact, "a kernel wrote outside its maps"
    assert not any(torch.isnan(m).any() for m in first), "an output element was not written"
    assert ok, figs
    for a, b, c in zip(first, second, plain):
        assert torch.equal(a, b) and torch.equal(a, c)
    if case.generic and not case.strip:
        # the specialised 21-tap kernels on the same inputs: inside the same bound against the same r64
        tuned = _call(case, fx, fy, q, wgt, 21)
        tfigs, tok = R21.check(tuned, r64, e32)
        print("%s (specialised): " % N.case_id(case) + "  ".join("%.2e / %.2e" % f for f in tfigs))
        assert tok, tfigs
        old = (ops.adists_window_stage_group if case.K else ops.adists_window_stage)(fx, fy, q, wgt, case.prec, case.strip)
        for a, b in zip(tuned, old):
            assert torch.equal(a, b)  # window=21 is the old call


def test_wrapper_refuses_what_the_kernels_cannot_take():
    from nerf_qa_amd import ops
    dev = torch.device("cuda:0")
    x = torch.rand(2, 24, 25, 64, device=dev)
    q, w = torch.rand(8, 2, 64, device=dev), torch.rand(2, 64, device=dev)
    g, t, s = ops.adists_window_stage(x, x, q, w, "f32", window=7)
    assert g.shape == t.shape == s.shape == (2, 18, 19)
    assert ops.adists_window_stage(x, x, q, w, "f32", window=25)[0].shape == (2, 1, 1)  # H = 24 < 25: the global branch
    for kw in ({"window": 2}, {"window": 64}, {"window": 7.0}, {"window": 7, "strip": 19}, {"window": 7, "strip": -1}):
        with pytest.raises(ValueError):
            ops.adists_window_stage(x, x, q, w, "f32", **kw)
    out = [torch.empty(2, 18, 19, device=dev) for _ in range(3)]
    ops.adists_window_stage_into(x, x, q, w, "f32", 0, *out, window=7)
    with pytest.raises(ValueError):
        ops.adists_window_stage_into(x, x, q, w, "f32", 0, *out, window=8)
