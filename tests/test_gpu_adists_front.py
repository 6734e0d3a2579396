"""The front part of the A-DISTS forward -- stats_nchw_kernel, pool_stats_kernel, stats_nhwc_kernel, adists_prep_kernel,
nchw3_to_nhwc4_kernel, entropy_nhwc_kernel, adists_entropy_fold_kernel and adists_weights_kernel, through ops.adists_front,
which launches them as adists_forward does -- held to a float64 replay of the same operation (tests/front_refs.py) at the
kernels' own edges: pool tiles that are whole, ragged to the right, ragged at the bottom with the window's lower row
outside the image, or shorter than TR; maps of 1 x 1, 1 x 13, 13 x 1 and 2 x 2 where every window is a border window; every
channel count and storage type of the pool pass; grids of 12 and of 8 blocks under the workgroup-id remap; 1, 2 and 67
blocks of the tap-5 statistics and of the entropy pass, the last holding one pixel; one full entropy block and one pixel
more; images of one block, of 4096 pixels and of 4160; all four modes; B = 1, 2, 3.  Every case asserts the edge it was
written for through ops.adists_front_grid.

Bounds (each case prints what it measures; front_refs.check):
    q rows 3, 4 (means)                      |d| <= 1e-6 (|mean| + 1e-3)
    q rows 5..7 (variances, covariance)      |d| <= 2e-5 max(var_x + var_y, 1e-12) + 1e-12
    q rows 0, 1 (inv)                        |d| <= 1e-6 |inv|
    hsum (q row 2), wgt, per stage           max|d| / max|r64| <= max(8 e32, 16 x 2^-24), e32 the float32 replay's own
    a dead channel                           inv == float32(1e12), mean, variance, covariance and hsum == 0 exactly;
                                             its wgt on the clamp's lower bound to the stage's bound on wgt
    every image's wgt                        |sum - 1| <= 1475 x 2^-24
Every call writes into prefilled outputs between guard regions (every element written, nothing else touched), and a second
call with another fill is bit-identical.

A 1 x 1 tap's entropies are taken as the reference's float32 run has them, exactly 0 (front_refs.ONE_PIXEL): the kernels
must give that 0 too, and the stage's weights sit on the clamp's lower bound.

Measured on an MI355X (all 41 cases pass), largest error / bound over the cases of a family (A  B  C):
  means                    0.21  0.14  0.16        (largest |d| / |mean|: 2.1e-7)
  variances, covariance    0.02  0.02  0.02
  inv                      0.28  0.20  0.19
  hsum                     0.15  0.12  0.10        (largest error 1.7e-7 of the stage's maximum; e32 1.8e-7 to 3.5e-7)
  wgt                      0.14  0.14  0.10        (largest error 2.5e-7 of the stage's maximum; e32 2.4e-7 to 4.8e-7)
  a dead channel's wgt     0.08  -     0.08        (family A: channels of a 1 x 1 tap whose one pixel is 0)
  |sum wgt - 1|            6.7e-8 at most (bound 8.8e-5)
No class of any case is above 0.3 of its bound, and the hand-chained forward is bit-equal in all four of its cases.
tests/test_front_refs.py recomputes e32 without a GPU and shows every named wrong replay at least 110 times above a
bound in some case.
"""
import pytest
import torch

import front_refs as R

pytestmark = pytest.mark.gpu

GUARD = 1 << 12  # floats on every side of every output
FENCE = -1234.5


@pytest.fixture(scope="module")
def refs():
    return {R.case_id(c): R.references(c) for c in R.CASES}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _run(x, y, taps, prec, fill):
    """One call into outputs prefilled with `fill` and fenced on every side: (q, wgt, fences intact)."""
    from nerf_qa_amd import ops
    B, dev = x.shape[0], x.device
    shapes = [(8, B, R.CTOT), (B, R.CTOT)]
    sizes = [int(torch.Size(s).numel()) for s in shapes]
    buf = torch.full((GUARD * 3 + sum(sizes),), FENCE, dtype=torch.float32, device=dev)
    fence = torch.ones_like(buf, dtype=torch.bool)
    outs, at = [], GUARD
    for s, n in zip(shapes, sizes):
        o = buf[at:at + n].view(s)
        o.fill_(fill)
        fence[at:at + n] = False
        outs.append(o)
        at += n + GUARD
    ops.adists_front_into(x, y, taps, prec, outs[0], outs[1])
    torch.cuda.synchronize()
    intact = bool((buf[fence] == FENCE).all())
    return outs[0].clone(), outs[1].clone(), intact


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_front_against_float64_replay(case, refs, dev):
    from nerf_qa_amd import ops
    (x, y, taps), r64, e32, dead = refs[R.case_id(case)]
    grid = ops.adists_front_grid(case.B, case.dims, case.prec)
    for k, want in case.expect.items():  # the case reaches the edge it was written for
        assert all(w is None or w == g for w, g in zip(want, grid[k])), (k, want, grid[k])
    x, y, taps = x.to(dev), y.to(dev), [t.to(dev) for t in taps]
    q, wgt, intact = _run(x, y, taps, case.prec, float("nan"))
    q2, wgt2, intact2 = _run(x, y, taps, case.prec, -777.25)
    figs, ok = R.check({"q": q, "wgt": wgt}, r64, e32, dead)
    print("%s: e32 hsum %.2e wgt %.2e | %s" % (R.case_id(case), max(e32["hsum"]), max(e32["wgt"]), R.show(figs)))
    assert intact and intact2, "a kernel wrote outside its outputs"
    assert not bool((q2 == -777.25).any()) and not bool((wgt2 == -777.25).any()), "an output element was not written"
    assert _same_bits(q, q2) and _same_bits(wgt, wgt2), "two calls differ"
    assert bool(torch.isfinite(q).all()) and bool(torch.isfinite(wgt).all())
    assert ok, figs
    q3, wgt3 = ops.adists_front(x, y, taps, case.prec)
    assert _same_bits(q, q3) and _same_bits(wgt, wgt3)


@pytest.fixture(scope="module")
def packed(np_convs, dev):
    from nerf_qa_amd import ops
    return {p: ops.pack_vgg_weights(np_convs, p).to(dev) for p in ("f32s", "f16")}


@pytest.mark.parametrize("prec", ["f32s", "f16"])
@pytest.mark.parametrize("h,w", [(45, 70), (9, 13)], ids=["45x70", "9x13"])
def test_forward_is_a_chain_of_its_three_parts(prec, h, w, packed, dev):
    """The A-DISTS twin of test_pyramid_is_a_chain_of_single_operators: real taps from ops.vgg_pyramid, then
    ops.adists_front, ops.adists_window_stage per stage on that stage's slice of q and wgt, and ops.adists_chain give
    ops.adists_forward's D and map bit for bit.  45 x 70: stages 0..2 windowed, the rest global; 9 x 13: all global."""
    from nerf_qa_amd import ops, synth
    B = 2
    x, y = (torch.from_numpy(a).to(dev) for a in synth.frame_batch([3, 5], h, w))
    taps = ops.vgg_pyramid(torch.cat([x, y]), packed[prec], prec)
    q, wgt = ops.adists_front(x, y, taps, prec)
    dims, nwin = ops.adists_chain_dims(h, w)
    assert nwin == (3 if h == 45 else 0)
    gamma, tw, sw = [], [], []
    for k, s in enumerate(R.stage_slices()):
        fx, fy = (x, y) if k == 0 else (taps[k - 1][:B], taps[k - 1][B:])
        g, t, s_ = ops.adists_window_stage(fx, fy, q[:, :, s].contiguous(), wgt[:, s].contiguous(), prec)
        assert tuple(g.shape) == (B,) + dims[k]
        gamma.append(g.contiguous())
        tw.append(t.contiguous())
        sw.append(s_.contiguous())
    _, d, m = ops.adists_chain(gamma, tw, sw, h, w)
    d0, m0 = ops.adists_forward(x, y, packed[prec], prec, with_map=True)
    torch.cuda.synchronize()
    print("%s %dx%d: max|d - d0| = %.3e, max|map - map0| = %.3e" % (prec, h, w, float((d - d0).abs().max()),
                                                                 float((m - m0).abs().max())))
    assert _same_bits(d, d0), (d, d0)
    assert _same_bits(m, m0)
