"""The A-DISTS window pass -- adists_window_lds_kernel, adists_window_lanes_kernel, adists_window_planar_kernel and
adists_global_kernel, through ops.adists_window_stage, which launches one stage exactly as adists_forward does -- held to
a float64 replay of the same stage (tests/window_refs.py) at the kernels' own edges: strips and 64-row groups, channel
blocks, grids of 1 / 6 / 8 / 9 / 20 blocks under the workgroup-id remap, dead columns, both forms of the lanes pass, the
planar kernel's column blocks and the global branch.

Bound, per map (gamma, tw, sw; all images of the case): max|hip - r64| / max|r64| <= max(8 x e32, 16 x 2^-24), e32 being
the float32 replay's own distance from r64 for that map (family B: 8 x e32 alone).  Every call also runs with NaN-filled
outputs between guard regions (every element written, nothing else touched) and twice (bit-identical).

Measured on an MI355X (all 87 cases pass; families A / B / C of window_refs.inputs):
  kernel family               largest error (of the map's maximum)     largest error / bound
  LDS, launcher's strips      2.8e-7 (A)  1.7e-7 (B)  2.2e-7 (C)      0.16  0.18  0.12
  LDS, forced strips          2.3e-7 (A)  2.0e-7 (B)  1.7e-7 (C)      0.15  0.13  0.12
  first form, f16 taps        2.1e-7 (A)  2.0e-7 (B)  1.8e-7 (C)      0.15  0.11  0.11
  first form, bf16 taps       2.2e-7 (A)                              0.14
  first form, float taps      1.9e-7 (A)  1.5e-7 (B)  1.5e-7 (C)      0.16  0.10  0.11
  planar (C = 3)              1.0e-6 (A)  1.0e-6 (B)  6.7e-7 (C)      0.47  0.14  0.13
  global branch               1.1e-7 (A)  2.7e-8 (B)  4.1e-8 (C)      0.12  0.06  0.04
No case is above a half of its bound; the HIP maps sit about as far from float64 as the float32 replay itself.
tests/test_window_refs.py recomputes e32 without a GPU and shows the smallest wrong replay caught (a rotated vertical
window, 2.2e-3) sits 250 times above the largest bound of any case (8.5e-6)."""
import pytest
import torch

import window_refs as R

pytestmark = pytest.mark.gpu

GUARD = 1 << 14  # floats on every side of every output map
FENCE = -1234.5


@pytest.fixture(scope="module")
def refs():
    return {R.case_id(c): R.references(c) for c in R.CASES}


def _device_taps(case, x, y, dev):
    if case.C == 3:
        return x.to(dev).contiguous(), y.to(dev).contiguous()
    return x.permute(0, 2, 3, 1).contiguous().to(dev), y.permute(0, 2, 3, 1).contiguous().to(dev)


def _run(case, fx, fy, q, wgt, shape):
    """One call into NaN-filled maps fenced on every side: (maps, whether the fences survived)."""
    from nerf_qa_amd import ops
    n = shape[0] * shape[1] * shape[2]
    buf = torch.full((4 * GUARD + 3 * n,), FENCE, dtype=torch.float32, device=fx.device)
    maps = []
    for j in range(3):
        m = buf[GUARD + j * (GUARD + n):][:n].view(shape)
        m.fill_(float("nan"))
        maps.append(m)
    ops.adists_window_stage_into(fx, fy, q, wgt, case.prec, case.strip, *maps)
    torch.cuda.synchronize()
    fence = torch.ones_like(buf, dtype=torch.bool)
    for j in range(3):
        fence[GUARD + j * (GUARD + n):][:n] = False
    return [m.clone() for m in maps], bool((buf[fence] == FENCE).all())


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_stage_against_float64_replay(case, refs):
    from nerf_qa_amd import ops
    dev = torch.device("cuda:0")
    (x, y, q, wgt), r64, e32 = refs[R.case_id(case)]
    fx, fy = _device_taps(case, x, y, dev)
    q, wgt = q.to(dev), wgt.to(dev)
    try:
        if case.legacy:
            ops.set_conv_variant(ops.DEFAULT_CONV_VARIANT | 8)
        grid = ops.adists_window_grid(case.B, case.H, case.W, case.C, case.prec, case.strip)
        first, intact = _run(case, fx, fy, q, wgt, tuple(r64[0].shape))
        second, _ = _run(case, fx, fy, q, wgt, tuple(r64[0].shape))
        plain = ops.adists_window_stage(fx, fy, q, wgt, case.prec, case.strip)
    finally:
        ops.set_conv_variant(ops.DEFAULT_CONV_VARIANT)
    # the dispatch: the LDS kernel exactly where the case means it, on the grid the case means
    assert (grid != (0, 0, 0)) == (case.kind == "lds"), grid
    if case.grid:
        assert grid == case.grid
    figs, ok = R.check(first, r64, e32, case.family)
    print("%s: " % R.case_id(case) + "  ".join("%s %.2e / %.2e (%.2f)" % (n, e, b, e / b if b else float("inf"))
                                               for n, (e, b) in zip(("gamma", "tw", "sw"), figs)))
    assert intact, "a kernel wrote outside its maps"
    assert not any(torch.isnan(m).any() for m in first), "an output element was not written"
    assert ok, figs
    for a, b, c in zip(first, second, plain):
        assert torch.equal(a, b) and torch.equal(a, c)


def test_wrapper_refuses_what_the_kernels_cannot_take():
    """Shapes, dtypes, devices and contiguity are checked before the library is called: nothing short reaches a kernel."""
    from nerf_qa_amd import ops
    dev = torch.device("cuda:0")
    x = torch.rand(2, 24, 25, 64, device=dev)
    q, w = torch.rand(8, 2, 64, device=dev), torch.rand(2, 64, device=dev)
    ops.adists_window_stage(x, x, q, w, "f32")
    bad = [(x[:1], x, q, w, "f32", 0), (x, x[:, :, :, :32], q, w, "f32", 0), (x.half(), x.half(), q, w, "f32", 0),
           (x, x, q, w, "f16", 0), (x, x, q[:, :1], w, "f32", 0), (x, x, q[:7], w, "f32", 0), (x, x, q, w[:, :32], "f32", 0),
           (x, x, q.double(), w, "f32", 0), (x, x, q, w.half(), "f32", 0), (x, x, q, w, "f32m", 0), (x, x, q, w, "f32", 5),
           (x, x, q, w, "f32", -1), (x.permute(0, 2, 1, 3), x.permute(0, 2, 1, 3), q, w, "f32", 0),
           (x, x, q.permute(0, 2, 1).contiguous().permute(0, 2, 1), w, "f32", 0),
           (x.permute(0, 3, 1, 2).contiguous(), x.permute(0, 3, 1, 2).contiguous(), q, w, "f32", 0),
           (x[:, :, :, :3].contiguous(), x[:, :, :, :3].contiguous(), q[:, :, :3].contiguous(), w[:, :3].contiguous(), "f32", 0)]
    for args in bad:
        with pytest.raises(ValueError):
            ops.adists_window_stage(*args)
    out = [torch.empty(2, 4, 5, device=dev) for _ in range(3)]
    ops.adists_window_stage_into(x, x, q, w, "f32", 0, *out)
    for wrong in (torch.empty(2, 4, 6, device=dev), torch.empty(2, 4, 5, device=dev, dtype=torch.float64),
                  torch.empty(2, 5, 4, device=dev).transpose(1, 2)):
        with pytest.raises(ValueError):
            ops.adists_window_stage_into(x, x, q, w, "f32", 0, out[0], wrong, out[2])
