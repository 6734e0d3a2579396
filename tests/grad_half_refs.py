"""A CPU emulation of the half gradient chain (grad_precision="f16": nerf_qa_amd/autograd.py, pyramid_backward_device), the
yardstick of its tests.

It is tests/grad_replay.py's walk -- the same masks, the same transposed convolutions, the same pool Jacobian -- with
the chain's three roundings put in and nothing else:
  * per image and layer the gradient is renormalised by the power of two that brings max |g| into [8, 16) (0 for a
    zero or non-finite maximum), the running total taken out at the end;
  * the masked, renormalised gradient is rounded to half before every convolution;
  * the convolution runs on half-rounded weights with a float64 sum, and its output is rounded to half.
The pool seam (taps, the tap's own gradient, the sum) and conv1_1's step are exact.  With `rounding=False` every step is
an exact rescaling of grad_replay.replay's, so the two agree to float64 rounding (tests/test_grad_half_refs.py); with
rounding on, the distance from the replay is what a plain-f16 chain costs on a case, which the HIP chain is held to a
multiple of (HIP_FACTOR).

Nothing of nerf_qa_amd is used here.
"""
import functools

import torch
import torch.nn.functional as F

import grad_replay
from grad_replay import POOL_BEFORE, TAP_LAYERS, _nchw, l2pool_grad
from oracle import dists_oracle as do

WINDOW_TOP = 4     # max |g| 2^k in [2^3, 2^4) = [8, 16)
HIP_FACTOR = 2.0   # what the HIP chain gets of the emulation's e_max / e_rms: float32 instead of float64 accumulation and
#                    the exponent choices that follow from it.  Fixed in advance, not fitted.


def exponents(g, top=WINDOW_TOP):
    """Per image of g (n, ...): the integer k with max|g| 2^k in [2^(top-1), 2^top), 0 for a zero or non-finite maximum;
    as a float64 tensor of shape (n, 1, 1, 1)."""
    mx = g.detach().abs().flatten(1).amax(dim=1).double()
    ok = torch.isfinite(mx) & (mx > 0)
    _, e = torch.frexp(torch.where(ok, mx, torch.ones_like(mx)))  # mx = f 2^e, f in [0.5, 1)
    k = torch.where(ok, top - e.double(), torch.zeros_like(mx))
    return k.view(-1, 1, 1, 1)


def _half(t, rounding):
    return t.to(torch.float16).to(t.dtype) if rounding else t


@torch.no_grad()
def replay_half(acts, taps, g_taps, convs, rounding=True, top=WINDOW_TOP):
    """grad_replay.replay(acts, taps, g_taps, convs, float64) through the half chain's arithmetic (module docstring)."""
    dtype = torch.float64
    mask = {}
    for l in range(13):
        a = taps[TAP_LAYERS.index(l)] if l in TAP_LAYERS else acts[l]
        mask[l] = _nchw(a, torch.float32) > 0
    tp = [_nchw(t, dtype) for t in taps]
    gt = [_nchw(g, dtype) for g in g_taps]
    g = gt[4]
    K = torch.zeros((g.shape[0], 1, 1, 1), dtype=dtype)
    for l in range(12, 0, -1):
        k = exponents(g, top)
        K = K + k
        gm = _half(g * torch.exp2(k) * mask[l], rounding)
        g = _half(F.conv_transpose2d(gm, _half(convs[l][0].to(dtype), rounding), padding=1), rounding)
        if l in POOL_BEFORE:
            s = POOL_BEFORE.index(l)
            g = l2pool_grad(tp[s], g) + gt[s] * torch.exp2(K)
    k = exponents(g, top)
    K = K + k
    g = F.conv_transpose2d(g * torch.exp2(k) * mask[0], convs[0][0].to(dtype), padding=1)
    return g * torch.exp2(-K) / torch.tensor(do.IMAGENET_STD, dtype=dtype).view(1, 3, 1, 1)


def cosine_gap(got, ref):
    """1 - cosine of the two gradients over every element, in float64."""
    a, b = got.detach().cpu().double().flatten(), ref.detach().cpu().double().flatten()
    return 1.0 - (a @ b).item() / (a.norm().item() * b.norm().item())


def convs64(seed=1234, gain=1.0):
    from nerf_qa_amd import synth
    return [(w.double(), b.double()) for w, b in do.convs_from_numpy(synth.vgg16_weights(seed, gain))]


@functools.lru_cache(maxsize=None)
def oracle_case(h, w, kinds, seeds, gain=1.0):
    """A float64 CPU case with DISTS' own tap gradients: the pairs synth.frame_batch(seeds, h, w, kinds) through the
    oracle pyramid (every layer kept) and d(sum of scores)/d(taps) through dists_oracle.dists_stats with the published
    alpha / beta.  Returns (acts, taps, g_taps, convs), maps NHWC, images [x.., y..]."""
    import os

    import numpy as np
    from nerf_qa_amd import synth
    convs = convs64(gain=gain)
    xn, yn = synth.frame_batch(list(seeds), h, w, list(kinds))
    imgs = torch.cat([torch.from_numpy(xn), torch.from_numpy(yn)]).double()
    b = len(seeds)
    acts, taps = grad_replay.oracle_acts(imgs, convs)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ab = np.load(os.path.join(root, "nerf_qa_amd", "data", "dists_alpha_beta.npz"))
    alpha, beta = (torch.from_numpy(ab[k]).view(1, -1, 1, 1).double() for k in ("alpha", "beta"))
    with torch.enable_grad():
        det = [imgs.clone().requires_grad_()] + [t.permute(0, 3, 1, 2).clone().requires_grad_() for t in taps]
        s1, s2 = do.dists_stats([f[:b] for f in det], [f[b:] for f in det])
        g_nchw = torch.autograd.grad(do.dists_score(s1, s2, alpha, beta).sum(), det[1:])
    return acts, taps, [g.permute(0, 2, 3, 1).contiguous() for g in g_nchw], convs


@functools.lru_cache(maxsize=None)
def emulation_figures(h, w, kinds, seeds, gain=1.0):
    """(e_max, e_rms, 1 - cosine) of the emulation against the exact float64 replay on oracle_case(...)."""
    acts, taps, g_taps, convs = oracle_case(h, w, kinds, seeds, gain)
    exact = grad_replay.replay(acts, taps, g_taps, convs, torch.float64)
    emu = replay_half(acts, taps, g_taps, convs)
    e_max, e_rms = grad_replay.errors(emu, exact)
    return e_max, e_rms, cosine_gap(emu, exact)
