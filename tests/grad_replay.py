"""A plain high-precision reference of the pyramid's backward chain, for the gradient tests.

With every ReLU mask fixed, d(image)/d(taps) is a LINEAR map of the five tap gradients: transposed convolutions, the
L2-pool's Jacobian at the given taps, the masks, the input normalisation.  `replay` evaluates that map on the CPU in
`dtype` with torch's own operators, taking the masks from the activations it is given -- so a comparison against it
holds every pixel of the HIP chain (nerf_qa_amd/autograd.py: pyramid_backward) to float rounding, without the ReLUs that
switch sides between two float32 forwards and force the end-to-end tests' loose bounds.

Nothing of nerf_qa_amd is used here: the weights are passed in, the pool is oracle/dists_oracle.py's.
"""
import torch
import torch.nn.functional as F

from oracle import dists_oracle as do

TAP_LAYERS = (1, 3, 6, 9, 12)   # conv layers (0-based, network order) whose ReLU output is tapped: relu1_2 .. relu5_3
POOL_BEFORE = (2, 4, 7, 10)     # conv layers whose input is the L2-pool of the previous stage's tap


def _nchw(t, dtype):
    return t.detach().to("cpu", dtype).permute(0, 3, 1, 2).contiguous()


def l2pool_grad(tap, g_pooled):
    """Gradient of dists_oracle.l2pool at `tap` (NCHW) applied to `g_pooled`, by autograd in tap's dtype; the pooled
    value is recomputed here, never read from anywhere."""
    x = tap.detach().clone().requires_grad_()
    with torch.enable_grad():
        y = do.l2pool(x)
        (gx,) = torch.autograd.grad(y, x, g_pooled)
    return gx


@torch.no_grad()
def replay(acts, taps, g_taps, convs, dtype=torch.float64):
    """d/d(image), (n,3,H,W) in `dtype`, of a scalar whose gradients with respect to the five taps are `g_taps`.

    acts:   {layer 0..12: NHWC float map}; only its sign pattern is used (mask_l = act_l > 0).  Tapped layers may be
            left out: their activation is the tap.
    taps:   the five tapped maps, NHWC float (relu1_2 .. relu5_3).
    g_taps: five NHWC maps shaped as the taps.
    convs:  13 (weight OIHW, bias) pairs in network order.
    """
    mask = {}
    for l in range(13):
        a = taps[TAP_LAYERS.index(l)] if l in TAP_LAYERS else acts[l]
        mask[l] = _nchw(a, torch.float32) > 0
    tp = [_nchw(t, dtype) for t in taps]
    gt = [_nchw(g, dtype) for g in g_taps]
    g = gt[4]
    for l in range(12, 0, -1):
        g = F.conv_transpose2d(g * mask[l], convs[l][0].to(dtype), padding=1)
        if l in POOL_BEFORE:
            s = POOL_BEFORE.index(l)
            g = l2pool_grad(tp[s], g) + gt[s]
    g = F.conv_transpose2d(g * mask[0], convs[0][0].to(dtype), padding=1)
    return g / torch.tensor(do.IMAGENET_STD, dtype=dtype).view(1, 3, 1, 1)


@torch.no_grad()
def oracle_acts(x, convs):
    """dists_oracle.vgg_pyramid(x, convs) once more, keeping every layer: ({layer: NHWC}, [five taps NHWC]) in x's dtype
    (the caller checks the taps against vgg_pyramid's own)."""
    dt = x.dtype
    mean = torch.tensor(do.IMAGENET_MEAN, dtype=dt).view(1, -1, 1, 1)
    std = torch.tensor(do.IMAGENET_STD, dtype=dt).view(1, -1, 1, 1)
    h = (x - mean) / std
    acts, taps = {}, []
    for l in range(13):
        if l in POOL_BEFORE:
            h = do.l2pool(h)
        h = F.relu(F.conv2d(h, convs[l][0].to(dt), convs[l][1].to(dt), stride=1, padding=1))
        acts[l] = h.permute(0, 2, 3, 1).contiguous()
        if l in TAP_LAYERS:
            taps.append(acts[l])
    return acts, taps


def errors(got, ref):
    """(e_max, e_rms) of `got` against `ref`, over every element: max|d| / max|ref| and rms(d) / rms(ref), in float64."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    d = got - ref
    return (d.abs().max().item() / ref.abs().max().item(),
            d.pow(2).mean().sqrt().item() / ref.pow(2).mean().sqrt().item())


YARD_FLOOR = 1e-6   # a few float32 epsilons: a lucky float32 evaluation must not set a bound of zero
HIP_FACTOR = 8.0    # 4x: split16 carries 22 significant bits against float32's 24; 2x: another summation order and
#                     the per-layer power-of-two renormalisation.  Fixed in advance, not fitted.


def bound(yard):
    return HIP_FACTOR * max(yard, YARD_FLOOR)
