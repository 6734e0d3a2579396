"""The back part of the A-DISTS forward -- chain_init_kernel, ones_kernel, chain_moments_kernel, chain_fold_kernel,
chain_psminmax_kernel, chain_ppminmax_kernel, chain_final_kernel, chain_global_kernel, adists_d_kernel and
adists_map_kernel, through ops.adists_chain, which launches them exactly as adists_forward does -- held to a float64
replay of the same operation (tests/chain_refs.py) at the kernels' own edges: all-global frames, windowed maps of 1, 2, 4
and 6 elements, exactly one block, a last block of 16 live threads, a 1 x 2 stage upsampled to 21 x 23, up to six windowed
stages, and 513 x 514 elements, where the grids stop at 1024 blocks and the stride loops run.

Bound, per output (each ps_prod map, D, the map; all images of the case):
    max|hip - r64| <= max(8 x e32, 16 x 2^-24 x max(1, max|r64|)),
e32 being the float32 replay's own distance from r64 for that output.  Every call writes into prefilled outputs between
guard regions (every element written, nothing else touched); a second call with another fill is bit-identical; image 0 on
its own gives row 0 of the batch call bit for bit; the 21 x 21 frame has NaN exactly where the float64 replay has.

Measured on an MI355X (all 39 cases pass; families of chain_refs.inputs: lognormal / smooth / two-level):
  output                      largest error                            largest error / bound
  ps_prod (six maps a case)   5.4e-6      9.0e-7      4.4e-6           0.21  0.21  0.22
  D                           3.8e-7      4.1e-7      3.7e-7           0.09  0.11  0.09
  map                         1.9e-5      1.8e-5      2.7e-5           0.14  0.15  0.13
No output of any case is above a quarter of its bound: the kernels sit closer to float64 than the float32 replay does
(fp64 moment and D sums); the largest errors are those of the 513 x 514 maps, where a float source coordinate of the
bilinear steps is worth 3e-5 of a pixel in both.
tests/test_chain_refs.py recomputes e32 without a GPU and shows every named wrong replay at least 1.4e4 times above the
bound in some case."""
import pytest
import torch

import chain_refs as R

pytestmark = pytest.mark.gpu

GUARD = 1 << 12  # floats on every side of every output
FENCE = -1234.5


@pytest.fixture(scope="module")
def refs():
    return {R.case_id(c): R.references(c) for c in R.CASES}


def _run(gamma, tw, sw, H, W, fill, with_map=True):
    """One call into outputs prefilled with `fill` and fenced on every side: ((ps_prod, d, map), fences intact)."""
    from nerf_qa_amd import ops
    B, dev = gamma[0].shape[0], gamma[0].device
    shapes = [tuple(g.shape) for g in gamma] + [(B,)] + ([(B, H, W)] if with_map else [])
    sizes = [int(torch.Size(s).numel()) for s in shapes]
    buf = torch.full((GUARD * (len(sizes) + 1) + sum(sizes),), FENCE, dtype=torch.float32, device=dev)
    fence = torch.ones_like(buf, dtype=torch.bool)
    outs, at = [], GUARD
    for s, n in zip(shapes, sizes):
        o = buf[at:at + n].view(s)
        o.fill_(fill)
        fence[at:at + n] = False
        outs.append(o)
        at += n + GUARD
    ops.adists_chain_into(gamma, tw, sw, H, W, outs[:6], outs[6], outs[7] if with_map else None)
    torch.cuda.synchronize()
    intact = bool((buf[fence] == FENCE).all())
    outs = [o.clone() for o in outs]
    return (outs[:6], outs[6], outs[7] if with_map else None), intact


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_chain_against_float64_replay(case, refs):
    dev = torch.device("cuda:0")
    (gamma, tw, sw), r64, e32, _ = refs[R.case_id(case)]
    gamma, tw, sw = ([t.to(dev) for t in ts] for ts in (gamma, tw, sw))
    first, intact = _run(gamma, tw, sw, case.H, case.W, float("nan"))
    second, intact2 = _run(gamma, tw, sw, case.H, case.W, -777.25)
    figs, ok = R.check(first, r64, e32)
    print("%s: " % R.case_id(case) + "  ".join("%s %.2e / %.2e (%.2f)" % (n, e, b, e / b) for n, e, b in figs))
    assert intact and intact2, "a kernel wrote outside its outputs"
    # written everywhere: no element keeps the finite fill, and the NaN-filled call has NaN only where r64 has (R.check)
    for a, b in zip(R.flat(first)[1], R.flat(second)[1]):
        assert not bool((b == -777.25).any()), "an output element was not written"
        assert _same_bits(a, b), "two calls differ"
    assert ok, figs
    if case.H == 21 and case.W == 21:
        ps, d, m = first
        assert all(torch.isnan(p).all() for p in ps[:2]) and torch.isnan(d).all() and torch.isnan(m).all()
        assert all(torch.isfinite(p).all() for p in ps[2:])
    if case.B > 1:
        alone, _ = _run(*([t[:1].contiguous() for t in ts] for ts in (gamma, tw, sw)), case.H, case.W, float("nan"))
        for a, b in zip(R.flat(first)[1], R.flat(alone)[1]):
            assert _same_bits(a[:1], b), "image 0 depends on the rest of the batch"


def test_without_the_map_d_and_ps_prod_are_the_same_bits(refs):
    from nerf_qa_amd import ops
    dev = torch.device("cuda:0")
    case = R.Case(97, 131, 3, "lognormal")
    gamma, tw, sw = ([t.to(dev) for t in ts] for ts in refs[R.case_id(case)][0])
    (ps, d, m), intact = _run(gamma, tw, sw, case.H, case.W, float("nan"))
    (ps0, d0, m0), intact0 = _run(gamma, tw, sw, case.H, case.W, float("nan"), with_map=False)
    assert intact and intact0 and m0 is None
    assert _same_bits(d, d0) and all(_same_bits(a, b) for a, b in zip(ps, ps0))
    ps1, d1, m1 = ops.adists_chain(gamma, tw, sw, case.H, case.W)
    assert _same_bits(d, d1) and _same_bits(m, m1) and all(_same_bits(a, b) for a, b in zip(ps, ps1))
    assert ops.adists_chain(gamma, tw, sw, case.H, case.W, with_map=False)[2] is None


def test_wrapper_refuses_what_the_kernels_cannot_take():
    """Shapes, dtypes, devices and contiguity are checked before the library is called: nothing short reaches a kernel."""
    from nerf_qa_amd import _lib, ops
    dev = torch.device("cuda:0")
    H, W, B = 45, 50, 2
    dims, nwin = ops.adists_chain_dims(H, W)
    assert (dims, nwin) == ([(25, 30), (25, 30), (3, 5), (1, 1), (1, 1), (1, 1)], 3)
    g = [0.05 + torch.rand((B,) + d, device=dev) for d in dims]
    t = [torch.rand((B,) + d, device=dev) for d in dims]
    ops.adists_chain(g, t, t, H, W)

    def swap(ts, k, new):
        return ts[:k] + [new] + ts[k + 1:]

    bad = [(g[:5], t, t, H, W), (g, t + t[:1], t, H, W), (g, t, tuple(t[:3]), H, W), (g, t, t, H, W + 1), (g, t, t, H + 2, W),
           (g, t, t, 0, W), (g, t, t, H, -1), (swap(g, 0, g[0][:1]), t, t, H, W), (g, swap(t, 2, t[2][:, :, :4]), t, H, W),
           (g, t, swap(t, 5, t[5][:, 0]), H, W), (swap(g, 1, g[1].double()), t, t, H, W), (g, swap(t, 1, t[1].half()), t, H, W),
           (swap(g, 0, g[0].transpose(1, 2).contiguous().transpose(1, 2)), t, t, H, W),
           (g, t, swap(t, 2, torch.rand(B, 3, 10, device=dev)[:, :, ::2]), H, W),
           ([x[:0] for x in g], [x[:0] for x in t], [x[:0] for x in t], H, W), (swap(g, 3, None), t, t, H, W)]
    for args in bad:
        with pytest.raises(ValueError):
            ops.adists_chain(*args)
    with pytest.raises(_lib.NqaError):
        ops.adists_chain(swap(g, 4, g[4].cpu()), t, t, H, W)
    ps = [torch.empty((B,) + d, device=dev) for d in dims]
    d, m = torch.empty(B, device=dev), torch.empty(B, H, W, device=dev)
    ops.adists_chain_into(g, t, t, H, W, ps, d, m)
    ops.adists_chain_into(g, t, t, H, W, ps, d)
    wrong = [(ps[:5], d, m), (swap(ps, 0, ps[0][:, :24]), d, m), (swap(ps, 2, ps[2].double()), d, m), (ps, d[:1], m),
             (ps, d.double(), m), (ps, d, m[:, :, :49]), (ps, d, torch.empty(B, W, H, device=dev).transpose(1, 2)),
             (ps, torch.empty(2 * B, device=dev)[::2], m), (swap(ps, 1, None), d, m)]
    for outs in wrong:
        with pytest.raises(ValueError):
            ops.adists_chain_into(g, t, t, H, W, *outs)
