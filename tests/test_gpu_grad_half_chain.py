"""The half gradient chain, autograd.pyramid_backward_device(grad_precision="f16"), on device activations against the
float64 replay of the same linear map on the device's own ReLU masks (tests/grad_replay.py).

Yardstick: the CPU emulation of the chain's arithmetic (tests/grad_half_refs.py: half-rounded masked gradient, half
weights, float64 sums, half-rounded conv output, window [8, 16)) on the SAME operands.  The HIP chain gets
grad_half_refs.HIP_FACTOR = 2 times the emulation's e_max and e_rms: float32 instead of float64 accumulation and the
exponent choices that follow from it.  Fixed in advance, not fitted.  Per case the f32s chain is printed beside them.
    e_max = max|got - f64| / max|f64|        e_rms = rms(got - f64) / rms(f64)

Measured on an MI355X (HIP f16 / emulation / HIP f32s, e_max; e_rms is within 10 % of it; full table in DESIGN.md 4.17):
    1x1 n=2 random 2.5e-4 / 2.4e-4 / 7.4e-8      5x7 n=2 random 4.2e-4 / 5.1e-4 / 2.3e-7
    33x47 n=4 real 5.7e-4 / 5.9e-4 / 5.6e-7      96x112 n=2 gain 1.3 real 1.28e-3 / 1.31e-3 / 1.2e-6

Without a reference: exact scaling by 2^+-20, determinism, independence of an image from its neighbour's scale, dead
tap entries, finiteness, and the launch count of the conv class."""
import functools

import pytest
import torch

import grad_half_refs as ghr
import grad_replay
from grad_replay import errors

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _module(spec):
    from nerf_qa_amd.DISTS_pytorch import DISTS
    return DISTS(vgg16_path=spec).to(DEV).eval()


@functools.lru_cache(maxsize=None)
def _convs(spec):
    parts = spec.split(":")
    return ghr.convs64(int(parts[1]), float(parts[2]) if len(parts) > 2 else 1.0)


@functools.lru_cache(maxsize=None)
def _forward(spec, h, w, kinds, seed):
    """pyramid_keep of the pairs' images [x.., y..] on the device, and what the replay needs of it on the CPU."""
    from nerf_qa_amd import autograd, ops, synth
    m = _module(spec)
    b = len(kinds)
    xn, yn = synth.frame_batch([seed + i for i in range(b)], h, w, list(kinds))
    imgs = torch.cat([torch.from_numpy(xn), torch.from_numpy(yn)]).to(DEV).contiguous()
    acts, taps, pooled = autograd.pyramid_keep(m, imgs)
    torch.cuda.synchronize()
    acts_c = {l: ops.split16_decode(a).cpu() for l, a in acts.items() if l not in ops.TAP_LAYERS}
    return m, b, acts, taps, pooled, acts_c, [t.cpu() for t in taps]


def _real_g_taps(m, b, taps):
    """The tap gradients DISTS' own backward forms (the statistics' gradient of the module's weighted sum)."""
    from nerf_qa_amd import autograd
    a, bt = m.alpha.detach().reshape(1, -1).to(DEV), m.beta.detach().reshape(1, -1).to(DEV)
    wsum = a.sum() + bt.sum()
    g1, g2 = (-a / wsum).expand(b, -1).contiguous(), (-bt / wsum).expand(b, -1).contiguous()
    off, out = 3, []
    for t in taps:
        c = t.shape[-1]
        gx, gy = autograd._stats_grad(t[:b], t[b:], g1[:, off:off + c], g2[:, off:off + c], dims=(1, 2))
        out.append(torch.cat([gx, gy]).contiguous())
        off += c
    return out


def _random_g_taps(taps, seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(t.shape, generator=gen).to(DEV) for t in taps]


def _half_chain(m, acts, taps, pooled, g_taps, **kw):
    from nerf_qa_amd import autograd
    return autograd.pyramid_backward_device(m, acts, taps, pooled, g_taps, grad_precision="f16", **kw)


CASES = [  # (weights, h, w, kinds of the pairs (n = 2 * len), g kind)
    ("synth:1234", 1, 1, ("noise10",), "random"),
    ("synth:1234", 5, 7, ("noise10",), "random"),
    ("synth:1234", 33, 47, ("blur", "nerf_float"), "real"),
    ("synth:1234:1.3", 96, 112, ("noise02",), "real"),
]


@pytest.mark.parametrize("spec,h,w,kinds,gk", CASES, ids=[f"{h}x{w}-n{2 * len(k)}-{g}" for _, h, w, k, g in CASES])
def test_half_chain_matches_float64_replay_within_twice_the_emulation(spec, h, w, kinds, gk):
    from nerf_qa_amd import autograd
    m, b, acts, taps, pooled, acts_c, taps_c = _forward(spec, h, w, kinds, 31)
    g_taps = _real_g_taps(m, b, taps) if gk == "real" else _random_g_taps(taps, h * w)
    got = _half_chain(m, acts, taps, pooled, g_taps).cpu()
    f32s = autograd.pyramid_backward_device(m, acts, taps, pooled, g_taps, grad_precision="f32s").cpu()
    g_c = [g.cpu() for g in g_taps]
    convs = _convs(spec)
    r64 = grad_replay.replay(acts_c, taps_c, g_c, convs, torch.float64)
    emu = ghr.replay_half(acts_c, taps_c, g_c, convs)
    assert torch.isfinite(got).all() and torch.isfinite(r64).all() and r64.abs().max().item() > 0
    (y_max, y_rms), (e_max, e_rms), (s_max, s_rms) = errors(emu, r64), errors(got, r64), errors(f32s, r64)
    print(f"\n[half chain] {h}x{w} n={2 * b} {'+'.join(kinds)} {spec} {gk}: max|grad| {r64.abs().max().item():.2e}\n"
          f"    HIP f16   e_max {e_max:.2e}  e_rms {e_rms:.2e}  1-cos {ghr.cosine_gap(got, r64):.2e}\n"
          f"    emulation e_max {y_max:.2e}  e_rms {y_rms:.2e}  1-cos {ghr.cosine_gap(emu, r64):.2e}\n"
          f"    HIP f32s  e_max {s_max:.2e}  e_rms {s_rms:.2e}  1-cos {ghr.cosine_gap(f32s, r64):.2e}")
    assert e_max <= ghr.HIP_FACTOR * y_max and e_rms <= ghr.HIP_FACTOR * y_rms, (e_max, y_max, e_rms, y_rms)


def test_exact_scaling_determinism_and_finiteness():
    """chain(c g) == c chain(g) bit for bit for c = 2^-20, 2^20 (the exponents take out exact powers of two, so every
    kernel sees the same operands), on a real DISTS gradient at 96x112; two calls are bit-equal."""
    m, b, acts, taps, pooled, _, _ = _forward("synth:1234:1.3", 96, 112, ("noise02",), 31)
    g = _real_g_taps(m, b, taps)
    base = _half_chain(m, acts, taps, pooled, g)
    again = _half_chain(m, acts, taps, pooled, g)
    assert torch.isfinite(base).all() and base.abs().max().item() > 0 and torch.equal(base, again)
    for c in (2.0 ** -20, 2.0 ** 20):
        scaled = _half_chain(m, acts, taps, pooled, [x * c for x in g])
        assert torch.equal(scaled, base * c), c


def test_an_image_does_not_see_its_neighbours_scale():
    """Image 0 alone equals image 0 beside an image whose upstream is 2^12 times larger, bit for bit: the exponents are
    per image."""
    m, b, acts, taps, pooled, _, _ = _forward("synth:1234", 33, 47, ("blur", "nerf_float"), 31)
    g = _real_g_taps(m, b, taps)
    one = _half_chain(m, {l: a[:1].contiguous() for l, a in acts.items()}, [t[:1].contiguous() for t in taps], None,
                      [x[:1].contiguous() for x in g])
    scale = torch.ones((taps[0].shape[0], 1, 1, 1), device=DEV)
    scale[1:] = 2.0 ** 12
    both = _half_chain(m, acts, taps, pooled, [x * scale for x in g])
    assert torch.isfinite(both).all() and one.abs().max().item() > 0
    assert torch.equal(both[:1], one)


def test_huge_gradients_on_dead_tap_entries_change_nothing():
    """1e8-fold gradients on exactly dead tap entries (A-DISTS' F.normalize produces such) are discarded by the tap's ReLU
    BEFORE the first exponent is taken (masked=False): bit-equal to the same call with those entries zeroed."""
    m, b, acts, taps, pooled, _, _ = _forward("synth:1234", 40, 56, ("nerf_white",), 31)
    g = [x * 1e-3 for x in _random_g_taps(taps, 9)]
    dead = [t == 0 for t in taps]
    assert all(int(d.sum()) > 0 for d in dead)
    g_huge = [torch.where(d, x * 1e8, x) for x, d in zip(g, dead)]
    g_zero = [torch.where(d, torch.zeros_like(x), x) for x, d in zip(g, dead)]
    a = _half_chain(m, acts, taps, pooled, g_huge, masked=False)
    z = _half_chain(m, acts, taps, pooled, g_zero, masked=False)
    assert torch.isfinite(a).all() and a.abs().max().item() > 0 and torch.equal(a, z)


def test_the_half_chain_launches_as_many_convolutions():
    """Twelve data-gradient convolutions in either chain (the launch counters of the timing ring, class conv_igemm)."""
    from nerf_qa_amd import autograd, ops
    m, b, acts, taps, pooled, _, _ = _forward("synth:1234", 5, 7, ("noise10",), 31)
    g = _random_g_taps(taps, 35)
    counts = {}
    for gp in ("f32s", "f16"):
        autograd.pyramid_backward_device(m, acts, taps, pooled, g, grad_precision=gp)  # (packs the blobs)
        torch.cuda.synchronize()
        ops.timing_enable(True)
        try:
            autograd.pyramid_backward_device(m, acts, taps, pooled, g, grad_precision=gp)
            counts[gp] = ops.timing_collect()["conv_igemm"][0]
        finally:
            ops.timing_enable(False)
    assert counts["f32s"] == counts["f16"] == 12, counts


def test_only_the_set_that_is_asked_for_is_packed():
    from nerf_qa_amd import autograd
    from nerf_qa_amd.DISTS_pytorch import DISTS
    m = DISTS(vgg16_path="synth:1234", grad_precision="f16").to(DEV).eval()
    _, b, acts, taps, pooled, _, _ = _forward("synth:1234", 5, 7, ("noise10",), 31)
    autograd.pyramid_backward_device(m, acts, taps, pooled, _random_g_taps(taps, 35))  # the module's own setting
    assert set(m._bwd_blobs[1]) == {"f16"}
    with pytest.raises(ValueError):
        autograd.pyramid_backward_device(m, acts, taps, pooled, _random_g_taps(taps, 35), grad_precision="bf16")
