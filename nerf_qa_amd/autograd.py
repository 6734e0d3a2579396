"""Image gradients of DISTS: `DISTS.forward(x, y, require_grad=True)` (nerf_qa/DISTS_pytorch/DISTS_pt.py:105-108), and of
A-DISTS' default `as_loss=True` (nerf_qa/ADISTS/ADISTS.py:139-141) through `PyramidTaps`.

The reference gets them by running forward_once with autograd enabled.  Here the VALUES (S1, S2) come from the fused
HIP forward as always; when a gradient is asked for, `DistsSimilarities.backward` re-runs the pyramid layer by layer in
the float-precision mode (f32s: three-term split products) to have the activations, and walks it backwards with the
kernels of csrc/nqa_backward.hip: ReLU mask -> conv with the flipped, transposed weights -> L2-pool gradient -> ... ->
conv1_1's gradient onto the three image planes.  The per-channel statistics' gradient (DISTS_pt.py:130-141) is an affine
map of the two taps with per-(pair, channel) coefficients; those few numbers are evaluated in float64 on the device.
The alpha/beta weighted sum stays the torch expression of DISTS_pt.py, so autograd chains d(score)/d(S1, S2) into
this Function and reaches alpha and beta on its own.  No VGG weight receives a gradient (they are frozen, :51-52).

Used as a LOSS (a render x against a fixed frame y, inside an optimisation loop) the backward is dists_backward's loss
path: only the images that need a gradient are walked back, the statistics' gradient and the chain's power-of-two
renormalisation are HIP (csrc/nqa_loss_backward.hip, the scaled kernels of csrc/nqa_backward.hip) with per-image exponents
in device memory, and nothing is read back to the host.  pyramid_backward and _stats_grad are the first form: the
reference the tests pin, A-DISTS' head, and the baseline of tools/gpu_loss_step_bench.py.

A-DISTS as a loss with the gradient on y alone (x the fixed frame) has the same kind of path: AdistsLossY /
adists_backward_y, the head's backward in csrc/nqa_adists_backward.hip on top of the scoring path's staged entry points.
Under loss_head="auto" that path (and a gradient through a prepared target) is taken with window_size 21 only; under
loss_head="hip" every window in 3..63 takes it, on the generic window-moments kernels of csrc/nqa_window_moments_n.hip
(_backward_window names the window the stage backward runs with).

Against a PREPARED TARGET (nerf_qa_amd/target.py: the fixed frame's taps computed once for the whole optimisation) both
losses run one kept pyramid of y per step and nothing of x: DistsTargetSimilarities keeps the statistics' fp64 partials
from its forward and starts the backward from them, AdistsTargetLoss runs adists_backward_y's two halves in its forward
and its backward.  PairTargetLoss is the two together for a loss that sums both metrics (nerf_qa_amd/pair.py,
forward_target): one kept pyramid serves both heads, and the sum of their tap gradients goes down one chain.
DistsTargetStep (DISTS(target_step="c")) is DistsTargetSimilarities with both halves issued by the library: two calls on
one state tensor (csrc/nqa_loss_step.hip), the same launches in the same order, the same bits.

One walk each way: _pyramid_forward (pyramid_keep keeps all of it, pyramid_taps the five taps) and pyramid_backward_device,
whose rung of grad_precision is a record of _RUNGS (packer, exponent, mask, data-gradient convolution).  _target_backward
is the tail of every one-sided loss: the tap gradients of the metrics in use, one chain, the image terms.
"""
from __future__ import annotations

import math
from collections import namedtuple

import torch

from . import ops

C1 = C2 = 1e-6  # DISTS_pt.py:115-116


def _stats_grad(fx, fy, g1, g2, dims):
    """d(sum g1*S1 + g2*S2)/d(fx), /d(fy) for one tap.  fx, fy: float maps with the pixel axes `dims`; g1, g2: (B, C)
    upstream gradients of that tap's S1 / S2 columns.

    With dx = fx - mean(fx), dy = fy - mean(fy):  g_fx = [g1 dS1/dmx + g2 (2 dS2/dv dx + dS2/dcov dy)] / N, and for a mild
    distortion (S2 near 1) the two S2 terms cancel to a small remainder.  So the maps are centred FIRST (elementwise, in
    float32 around a float64 mean) and every per-channel sum is accumulated in float64: forming the same expression from
    separately rounded float32 means loses the remainder -- the error then grows with sqrt(N) (measured 1.5e-3 at 40x56,
    1.7e-2 at 160x192 against float64 autograd; this form: float32-autograd level)."""
    n = 1
    for d in dims:
        n *= fx.shape[d]
    f64 = torch.float64
    mx, my = fx.sum(dim=dims, dtype=f64) / n, fy.sum(dim=dims, dtype=f64) / n
    shape = [fx.shape[0]] + [1] * (fx.dim() - 1)
    cdim = [d for d in range(1, fx.dim()) if d not in dims][0]
    shape[cdim] = fx.shape[cdim]
    dx, dy = fx - mx.float().reshape(shape), fy - my.float().reshape(shape)
    sx, sy = dx.sum(dim=dims, dtype=f64) / n, dy.sum(dim=dims, dtype=f64) / n  # what the float32 rounding of the means left
    vx = (dx * dx).sum(dim=dims, dtype=f64) / n - sx * sx
    vy = (dy * dy).sum(dim=dims, dtype=f64) / n - sy * sy
    cov = (dx * dy).sum(dim=dims, dtype=f64) / n - sx * sy
    g1, g2 = g1.double(), g2.double()
    n1, d1 = 2 * mx * my + C1, mx * mx + my * my + C1
    ds1_dmx, ds1_dmy = (2 * my * d1 - 2 * mx * n1) / (d1 * d1), (2 * mx * d1 - 2 * my * n1) / (d1 * d1)
    n2, d2 = 2 * cov + C2, vx + vy + C2
    ds2_dcov, ds2_dv = 2 / d2, -n2 / (d2 * d2)
    b = 2 * g2 * ds2_dv / n   # coefficient of the map's own centred values
    c = g2 * ds2_dcov / n     # coefficient of the other map's centred values
    ax = g1 * ds1_dmx / n - (b * sx + c * sy)
    ay = g1 * ds1_dmy / n - (b * sy + c * sx)
    ax, ay, b, c = (t.float().reshape(shape) for t in (ax, ay, b, c))
    gx = b * dx
    gx.add_(c * dy).add_(ax)
    gy = b * dy
    gy.add_(c * dx).add_(ay)
    return gx, gy


# What a forward leaves for its backward, as named records.  KeptPyramid: acts {layer 0..12: NHWC}, taps [5 float NHWC
# maps], pooled [4 split16 maps]; acts and pooled None where only the taps were kept.  AdistsState: the front's q (8, B,
# 1475) and wgt (B, 1475), per stage the maps [gamma, tw, sw, ps_prod], y's KeptPyramid.  TargetStats: the five taps'
# per-block fp64 partials, tap 0's maps and sums.  The pair's one pyramid is its AdistsState's.
KeptPyramid = namedtuple("KeptPyramid", "acts taps pooled")
AdistsState = namedtuple("AdistsState", "q wgt maps pyramid")
TargetStats = namedtuple("TargetStats", "parts fx0 fy0 scratch")
DistsTargetState = namedtuple("DistsTargetState", "pyramid stats")
PairTargetState = namedtuple("PairTargetState", "stats adists")
# The layer facts of the walks, each derived once.  Layer l reads the L2-pool of the previous stage's tap where the stage
# changes; its own activation is split16 unless it is tapped (a tapped layer's output is a float map).
_READS_POOL = frozenset(l for l in range(1, 13) if ops.CONV_STAGE[l] != ops.CONV_STAGE[l - 1])
_SPLIT16_ACT = frozenset(range(1, 13)) - frozenset(ops.TAP_LAYERS)
# One precision of the device gradient chain: the key of its blob set, how its data-gradient weights are packed, and the
# three kernels of a layer's step -- exponent(g, k, K), mask(g, act, act_is_split16, k), conv(gm, blob, cout).  (The pool
# seam and conv1_1's step choose by their operand's dtype in ops and need no entry.)
_Rung = namedtuple("_Rung", "name pack exponent mask conv")
# "f32s": split16 operands, float out, max|g| 2^k in [128, 256).  "f16": a plain half map between layers (rounded once by
# the mask; half weights, float32 accumulator, half out) and the window [8, 16): a convolution's output is a half there,
# and 16 times the largest L1 norm of a data-gradient filter has to stay below 65504.  g is float at the top and behind
# a pool seam (whose taps, tap gradients and output stay float) on both rungs.
_RUNGS = {r.name: r for r in (
    _Rung("f32s", ops.pack_conv_split, ops.grad_exponent, ops.relu_mask_split16_scaled, ops.conv3x3_split),
    _Rung("f16", ops.pack_conv_half, ops.grad_exponent_half, ops.relu_mask_f16_scaled, ops.conv3x3_half))}


def _backward_blobs(module, dev, grad_precision="f32s"):
    """Per conv layer 1..12 the data-gradient layer: W'[ci][co][ky][kx] = W[co][ci][2-ky][2-kx], packed once per weights
    by the packer of the rung `grad_precision` (_RUNGS).  Only the set that is asked for is packed and kept: the other
    one (60 / 30 MB) is never built unasked."""
    key = module._weights_key(dev)
    cache = getattr(module, "_bwd_blobs", None)
    if cache is None or cache[0] != key:
        cache = (key, {}, module._conv_modules()[0].weight.detach().float().contiguous().to(dev))
        module.__dict__["_bwd_blobs"] = cache
    rung = _RUNGS[grad_precision]
    if rung.name not in cache[1]:
        convs = module._conv_modules()
        cache[1][rung.name] = {l: rung.pack(convs[l].weight.detach().flip(2, 3).transpose(0, 1).contiguous()).to(dev)
                               for l in range(1, 13)}
    return cache[1][rung.name], cache[2]


@torch.no_grad()
def _pyramid_forward(module, imgs, keep):
    """The one forward walk: conv1_1, layers 1..12 and the four L2-pools of `imgs` (n,3,H,W float) in f32s, as a
    KeptPyramid of everything (keep) or of the five taps alone -- the same launches in the same order either way."""
    prec = "f32s"
    packed = module._packed_weights(imgs.device, prec)
    inp = ops.conv1_1(imgs, packed, prec)  # split16 (n,H,W,64)
    acts, taps, pooled = ({0: inp}, [], []) if keep else (None, [], None)
    for l in range(1, 13):
        inp = ops.conv3x3_relu(inp, l, packed, prec)  # float for the tapped layers, split16 otherwise
        if keep:
            acts[l] = inp
        if l in ops.TAP_LAYERS:
            taps.append(inp)
        if l + 1 in _READS_POOL:
            inp = ops.l2pool(inp, prec)  # split16
            if keep:
                pooled.append(inp)
    return KeptPyramid(acts, taps, pooled)


def pyramid_keep(module, imgs):
    """The pyramid of `imgs` (n,3,H,W float) again, layer by layer in f32s, keeping every activation:
    KeptPyramid(acts {layer: NHWC}, taps [5 float NHWC maps], pooled [4 split16 maps])."""
    return _pyramid_forward(module, imgs, keep=True)


@torch.no_grad()
def pyramid_backward(module, acts, taps, pooled, g_taps):
    """d/d(image) (n,3,H,W) of a scalar whose gradients with respect to the five tapped maps are `g_taps` (float NHWC, as
    `taps`), through the activations pyramid_keep kept.

    The data-gradient convolutions take split16 (f16 hi + lo) operands, whose dynamic range is f16's -- and image
    gradients of a mean-type score are tiny (~1/N per pixel: 1e-8 at a few thousand pixels, where a half is already
    subnormal).  Everything here is LINEAR in g, so g is renormalised by an exact power of two before every layer
    (max |g| into [128, 256)) and the accumulated exponent taken out of the final image gradient."""
    blobs, w0 = _backward_blobs(module, taps[0].device)  # (the host-scaled first form is f32s only)
    # A tapped map is a ReLU output: where it is 0 the gradient stops (torch's own rule, grad * (out > 0)).  Applied HERE,
    # before anything is renormalised: A-DISTS' F.normalize gives an exactly dead channel a gradient of the order of
    # 1 / eps = 1e12 times its upstream (5e8 measured on a 40 x 56 pair), which the mask discards -- but a renormalisation
    # by max |g| taken with it in would push every live gradient below the halves' range first.
    g_taps = [g * (t > 0) for g, t in zip(g_taps, taps)]

    def normalise(t, k_total):
        mx = float(t.abs().max())
        if mx > 0 and math.isfinite(mx):
            k = 7 - math.frexp(mx)[1] + 1  # mx * 2^k in [128, 256)
            t = t * (2.0 ** k)
            k_total += k
        return t, k_total

    g, K = normalise(g_taps[4], 0)
    for l in range(12, 0, -1):
        gm = ops.relu_mask_split16(g, acts[l], l in _SPLIT16_ACT)
        g = ops.conv3x3_split(gm, blobs[l], ops.CONV_CIN[l], relu=False)  # gradient w.r.t. the layer's input
        if l in _READS_POOL:  # the input was the L2-pool of the previous stage's tap
            s = ops.CONV_STAGE[l]
            gt = g_taps[s - 1] * (2.0 ** K)  # the tap's own gradient, in the running scale
            ops.l2pool_backward(taps[s - 1], pooled[s - 1], g, gt)  # gt += pool gradient
            g = gt
        g, K = normalise(g, K)
    gm = g * (ops.split16_decode(acts[0]) > 0)  # d(ReLU) of relu1_1, float
    return ops.conv1_1_backward(gm, w0) * (2.0 ** -K)  # (n,3,H,W), the input normalisation included


def pyramid_taps(module, imgs):
    """The five float NHWC taps of `imgs` by pyramid_keep's own launches, keeping nothing else: what the statistics need of
    an image that takes no gradient.  (The same walk as pyramid_keep on purpose: the fused forward of ops.vgg_pyramid
    runs stage 1 in another kernel and agrees with these to a summation order only, and the gradient of a pair must
    not depend on whether its partner asked for one.)"""
    return _pyramid_forward(module, imgs, keep=False).taps


def _grad_precision(module, grad_precision=None):
    """The gradient chain's precision: the argument, else the module's setting ("f32s" for a module that has none)."""
    v = grad_precision or getattr(module, "grad_precision", "f32s")
    if v not in _RUNGS:
        raise ValueError(f"grad_precision must be 'f32s' or 'f16', got {v!r}")
    return v


@torch.no_grad()
def pyramid_backward_device(module, acts, taps, pooled, g_taps, masked=False, grad_precision=None):
    """pyramid_backward with the renormalisation on the device: the exponents are taken per IMAGE by a reduction kernel
    and read by the scaled forms of the chain's kernels (csrc/nqa_loss_backward.hip, nqa_backward.hip), so nothing comes
    back to the host between the first and the last launch -- the step can be enqueued ahead, and the gradient of an
    image does not depend on what else is in the batch.  With one image the f32s exponents are the host path's and the
    result is pyramid_backward's bit for bit.  masked=True: g_taps already carry their taps' ReLU masks (g * (t > 0)).

    grad_precision (None: the module's own, DISTS(grad_precision=) / ADISTS(grad_precision=)) names the rung of _RUNGS
    whose packer, exponent, mask and convolution the walk runs.  `pooled` is not read (the seam pools the tap itself)."""
    rung = _RUNGS[_grad_precision(module, grad_precision)]
    blobs, w0 = _backward_blobs(module, taps[0].device, rung.name)
    if not masked:  # BEFORE the first exponent is taken (see pyramid_backward)
        g_taps = [g * (t > 0) for g, t in zip(g_taps, taps)]
    n, dev = taps[0].shape[0], taps[0].device
    k = torch.empty(n, dtype=torch.int32, device=dev)   # the exponent of the step, per image
    K = torch.zeros(n, dtype=torch.int32, device=dev)   # the running total
    g = ops._f32c(g_taps[4])
    rung.exponent(g, k, K)
    for l in range(12, 0, -1):
        gm = rung.mask(g, acts[l], l in _SPLIT16_ACT, k)
        g = rung.conv(gm, blobs[l], ops.CONV_CIN[l])
        if l in _READS_POOL:
            s = ops.CONV_STAGE[l]
            g = ops.l2pool_backward_scaled(taps[s - 1], g, g_taps[s - 1], K)  # the tap's own gradient * 2^K + pool gradient
        rung.exponent(g, k, K)
    return ops.conv1_1_backward_scaled(g, acts[0], w0, k, K)  # d(ReLU) of relu1_1 and 2^-K inside


def _image_stats(x, y):
    """The statistics of tap 0, the raw NCHW images, through the NCHW kernels of forward_from_feats: the image goes in as
    map 0 of six, the other five are single zero pixels.  (fx, fy, S1, S2 (B, 8): columns 0..2 are the image's, scratch:
    the forward's fp64 sums, which _image_stats_grad_from starts from)."""
    b, dev = x.shape[0], x.device
    dummy = [torch.zeros((b, 1, 1, 1), dtype=torch.float32, device=dev)] * 5
    fx, fy = [x] + dummy, [y] + dummy
    s1, s2, scratch = ops.dists_stats_nchw(fx, fy, keep_scratch=True)
    return fx, fy, s1, s2, scratch


def _image_stats_grad_from(fx, fy, scratch, g1, g2, need):
    """The gradient of _image_stats towards the images, from its kept sums: zero upstream gradients for the dummy maps."""
    pad = torch.zeros((g1.shape[0], 5), dtype=torch.float32, device=g1.device)
    gx, gy = ops.dists_stats_nchw_backward(fx, fy, scratch, torch.cat([g1[:, :3], pad], 1), torch.cat([g2[:, :3], pad], 1),
                                           [need[0]] + [False] * 5, [need[1]] + [False] * 5)
    return gx[0], gy[0]


def _image_stats_grad(x, y, g1, g2, need):
    """The statistics' gradient of tap 0, the raw NCHW images: _image_stats, then its backward."""
    fx, fy, _, _, scratch = _image_stats(x, y)
    return _image_stats_grad_from(fx, fy, scratch, g1, g2, need)


@torch.no_grad()
def _dists_backward_host(module, x, y, g1, g2):
    """The first form of dists_backward, kept callable as the baseline of tools/gpu_loss_step_bench.py: both images
    through the chain, the statistics' gradient in torch, the renormalisation read back to the host per layer."""
    b = x.shape[0]
    xy = torch.cat([x, y]).float().contiguous()
    acts, taps, pooled = pyramid_keep(module, xy)
    # ---- gradients of the statistics with respect to the six taps ----
    off = 3
    g_taps = []
    for k, t in enumerate(taps):
        c = t.shape[-1]
        gx, gy = _stats_grad(t[:b], t[b:], g1[:, off:off + c], g2[:, off:off + c], dims=(1, 2))
        g_taps.append(torch.cat([gx, gy]).contiguous())
        off += c
    gx0, gy0 = _stats_grad(x.float(), y.float(), g1[:, :3], g2[:, :3], dims=(2, 3))  # tap 0 = the raw image (NCHW)
    gimg = pyramid_backward(module, acts, taps, pooled, g_taps)
    return gimg[:b] + gx0, gimg[b:] + gy0


@torch.no_grad()
def dists_backward(module, x, y, g1, g2, need=(True, True), host_scaled=False):
    """(dL/dx, dL/dy) given dL/dS1, dL/dS2 (each (B, 1475)) for the pairs (x, y), float32 (B,3,H,W) on the GPU; None for
    the side `need` does not ask for.

    Only the images that need a gradient are run through pyramid_keep and the backward chain; the other one (the fixed
    ground-truth frame of a loss) gives its taps to the statistics and nothing else: half the activations, none of its
    twelve data-gradient convolutions.  The statistics' gradient is csrc/nqa_loss_backward.hip's (fp64 sums and
    coefficients, the taps' ReLU masks folded in), the chain is pyramid_backward_device: no host read anywhere, and every
    pair's gradient is independent of the rest of the batch.  host_scaled=True runs the first form instead (both sides,
    torch statistics, host-side renormalisation)."""
    need = (bool(need[0]), bool(need[1]))
    if host_scaled:
        gx, gy = _dists_backward_host(module, x, y, g1, g2)
        return (gx if need[0] else None), (gy if need[1] else None)
    if not (need[0] or need[1]):
        return None, None
    b = x.shape[0]
    x, y = x.float().contiguous(), y.float().contiguous()
    g1, g2 = ops._f32c(g1), ops._f32c(g2)
    if need[0] and need[1]:
        acts, taps, pooled = pyramid_keep(module, torch.cat([x, y]))
        tx, ty = [t[:b] for t in taps], [t[b:] for t in taps]
    elif need[0]:
        acts, taps, pooled = pyramid_keep(module, x)
        tx, ty = taps, pyramid_taps(module, y)
    else:
        acts, taps, pooled = pyramid_keep(module, y)
        tx, ty = pyramid_taps(module, x), taps
    # ---- gradients of the statistics with respect to the taps of the images in the chain, ReLU masks included ----
    off = 3
    g_taps = []
    for t, fx, fy in zip(taps, tx, ty):
        c = t.shape[-1]
        g = torch.empty_like(t)  # laid out as `taps`: x's images, then y's, whichever are in the chain
        out_x = g[:b] if need[0] else None
        out_y = g[-b:] if need[1] else None
        ops.dists_stats_nhwc_backward(fx, fy, g1, g2, off, need[0], need[1], out_x, out_y)
        g_taps.append(g)
        off += c
    gx0, gy0 = _image_stats_grad(x, y, g1, g2, need)  # tap 0 = the raw image (NCHW)
    gimg = pyramid_backward_device(module, acts, taps, pooled, g_taps, masked=True)
    if need[0] and need[1]:
        return gimg[:b] + gx0, gimg[b:] + gy0
    return (gimg + gx0, None) if need[0] else (None, gimg + gy0)


def _adists_y_bytes(b, h, w, window=ops.WINDOW):
    """Device bytes adists_backward_y holds beside the pyramid for b pairs of h x w frames at its largest stage (relu1_2:
    the two planar copies of the taps, the NHWC gradient and the stage's workspace for a window of `window` taps)."""
    return 3 * b * 64 * h * w * 4 + int(ops.lib().nqa_adists_ts_backward_bytes_n(b, 64, h, w, window))


def _backward_window(module) -> int:
    """The window the head's HIP backward runs with: the module's own under loss_head="hip"; 21 otherwise, where a
    backward runs only with window_size 21 (ADISTS._loss_with_grad, check_target_window)."""
    return module._window() if getattr(module, "loss_head", None) == "hip" else ops.WINDOW


@torch.no_grad()
def adists_backward_y(module, x, y, u):
    """dL/dy (B,3,H,W) of a loss over A-DISTS' D_b with dL/dD = u (B,) on the device, for a FIXED x: the one-sided loss
    path of ADISTS.forward (a render y optimised against a ground-truth frame x, the reference's own argument order,
    prep.py:186).  HIP from end to end and without one device -> host read: x gives its taps (pyramid_taps) and, through
    the scoring path's staged entry points, q, the channel weights and the probability chain ps_prod -- constants here;
    y's pyramid is kept (pyramid_keep), every stage's T / S terms and y's normalisation are differentiated by
    csrc/nqa_adists_backward.hip (ops.adists_ts_backward, ReLU masks folded in, gradients written as NHWC) and the five tap
    gradients go down pyramid_backward_device.  Bitwise repeatable; a pair's gradient does not depend on the rest of
    the batch.  Batches whose scratch would pass NQA_MAX_WORKSPACE_GB run in slices of pairs."""
    x, y, u = x.float().contiguous(), y.float().contiguous(), ops._f32c(u)
    b, _, h, w = x.shape
    win = _backward_window(module)
    n = ops._max_pairs(lambda k: _adists_y_bytes(k, h, w, win), b)
    if n < b:
        return torch.cat([adists_backward_y(module, x[i:i + n], y[i:i + n], u[i:i + n]) for i in range(0, b, n)])
    tx = pyramid_taps(module, x)
    _, state = adists_y_forward(module, x, tx, y)  # (D comes out on the way and is not needed here)
    return adists_y_backward(module, x, tx, y, state, u)


@torch.no_grad()
def adists_y_forward(module, x, tx, y, keep=True, kept=None):
    """The first half of adists_backward_y, up to D: x, y float32 contiguous (B,3,H,W), tx the five float NHWC taps of x
    (pyramid_taps).  Returns (D (B,), state: AdistsState), what adists_y_backward needs; keep=False runs y through
    pyramid_taps instead of pyramid_keep (the pyramid's acts and pooled are then None: a value without a gradient to
    follow).  kept = (acts, ty, pooled): y's pyramid as a caller already holds it (the pair loss, which shares it with
    DISTS); no pyramid launch runs here then, and `keep` is not looked at."""
    b, _, h, w = x.shape
    prec, dev, ws = "f32s", x.device, module._ws
    n = module._window()  # (a value for any window; adists_y_backward follows it at 21, and at every n under "hip")
    pyramid = _pyramid_forward(module, y, keep) if kept is None else KeptPyramid(*kept)
    ty = pyramid.taps
    # ---- what the head takes from x alone, and the per-channel scalars of both: the forward's own kernels ----
    q = torch.empty((8, b, ops.TOTAL_CHNS), dtype=torch.float32, device=dev)
    wgt = torch.empty((b, ops.TOTAL_CHNS), dtype=torch.float32, device=dev)
    ops.adists_front_into(x, y, [torch.cat([a, c]) for a, c in zip(tx, ty)], prec, q, wgt, ws)
    dims, _ = ops.adists_chain_dims(h, w, n)
    maps = [torch.empty((4, b) + d, dtype=torch.float32, device=dev) for d in dims]  # gamma, tw, sw, ps_prod per stage
    off = 0
    for k, c in enumerate(ops.CHNS):
        fx, fy = (x, y) if k == 0 else (tx[k - 1], ty[k - 1])
        ops.adists_window_stage_into(fx, fy, q[:, :, off:off + c].contiguous(), wgt[:, off:off + c].contiguous(), prec, 0,
                                     maps[k][0], maps[k][1], maps[k][2], n)
        off += c
    d = torch.empty((b,), dtype=torch.float32, device=dev)
    ops.adists_chain_into([m[0] for m in maps], [m[1] for m in maps], [m[2] for m in maps], h, w, [m[3] for m in maps], d,
                          None, ws, n)
    return d, AdistsState(q, wgt, maps, pyramid)


def _adists_y_tap_grads(module, x, tx, y, state, u):
    """(g0, g_taps) of A-DISTS towards y for dL/dD = u (B,): the image term (B,3,H,W) and the five masked NHWC tap
    gradients, each a buffer of its own that the caller may add to."""
    q, wgt, maps, ty = state.q, state.wgt, state.maps, state.pyramid.taps
    prec, ws, win = "f32s", module._ws, _backward_window(module)
    g0 = ops.adists_ts_backward(x, y, q, wgt, maps[0][3], u, mask=False, coff=0, ws=ws, window=win)
    off, g_taps = 3, []
    for k in range(1, 6):
        px, py = ops.nhwc_to_nchw_f32(tx[k - 1], prec), ops.nhwc_to_nchw_f32(ty[k - 1], prec)
        g_taps.append(ops.adists_ts_backward(px, py, q, wgt, maps[k][3], u, mask=True, coff=off, nhwc=True, ws=ws,
                                                window=win))
        off += ops.CHNS[k]
    return g0, g_taps


def _dists_y_tap_grads(target, ty, stats, g1, g2, into=None):
    """(gy0, g_taps) of the DISTS statistics towards y for dL/dS1, dL/dS2 = g1, g2 (each (B, 1475)), from the forward's
    kept sums `stats` (no second sums pass): tap 0's image term (B,3,H,W) and the five masked NHWC tap gradients -- fresh
    maps, or ADDED in place into `into`, another metric's gradients of the same taps (no map of their own, no add pass)."""
    g1, g2 = ops._f32c(g1), ops._f32c(g2)
    off, g_taps = 3, []
    for k, (fx, fy, part) in enumerate(zip(target.taps, ty, stats.parts)):
        if into is None:
            g_taps.append(ops.dists_stats_nhwc_backward_from(fx, fy, part, g1, g2, off, need_x=False)[1])
        else:
            g_taps.append(ops.dists_stats_nhwc_grad_y_add(fx, fy, part, g1, g2, off, into[k]))
        off += fx.shape[-1]
    _, gy0 = _image_stats_grad_from(stats.fx0, stats.fy0, stats.scratch, g1, g2, (False, True))
    return gy0, g_taps


def _target_backward(module, pyramid, adists=None, dists=None):
    """dL/dy over y's kept `pyramid`, the tail of every one-sided loss path: the tap gradients of the metrics in use (adists
    / dists: the arguments of _adists_y_tap_grads / _dists_y_tap_grads; None runs nothing), DISTS' added into A-DISTS'
    -- the chain is linear in them -- then ONE pyramid_backward_device on `module`'s blobs, then the image terms."""
    terms, g_taps = [], None
    if adists is not None:
        g0, g_taps = _adists_y_tap_grads(*adists)
        terms.append(g0)
    if dists is not None:
        gy0, g_taps = _dists_y_tap_grads(*dists, into=g_taps)
        terms.append(gy0)
    gy = pyramid_backward_device(module, pyramid.acts, pyramid.taps, pyramid.pooled, g_taps, masked=True)
    for term in terms:
        gy = gy + term
    return gy


def _loss_u(grad, b, as_loss):
    """u = dL/dD (B,) on the device from the upstream gradient of 1 - mean(D) (as_loss) or of 1 - D (B,)."""
    g = grad.detach().float()
    return (g.reshape(1) * (-1.0 / b)).expand(b).contiguous() if as_loss else (-g).contiguous()


@torch.no_grad()
def adists_y_backward(module, x, tx, y, state, u):
    """The second half of adists_backward_y: dL/dy for dL/dD = u (B,) from what adists_y_forward(keep=True) returned:
    the six stages' gradients towards y's maps, then the chain."""
    return _target_backward(module, state.pyramid, adists=(module, x, tx, y, state, u))


class AdistsLossY(torch.autograd.Function):
    """(x fixed, y) -> 1 - mean(D) of A-DISTS, differentiable in y alone.  The value is the scoring path's own (the fused
    kernel, ADISTS._score); x and y are all that is saved; the backward is adists_backward_y with u = -grad / B formed on
    the device."""

    @staticmethod
    def forward(ctx, x, y, module):
        ctx.module = module
        ctx.save_for_backward(x, y)
        return 1 - module._score(x, y, module.precision_for(x.shape[-2], x.shape[-1])).mean()

    @staticmethod
    def backward(ctx, grad):
        x, y = ctx.saved_tensors
        if not ctx.needs_input_grad[1]:
            return None, None, None
        return None, adists_backward_y(ctx.module, x, y, _loss_u(grad, x.shape[0], True)).to(y.dtype), None


def check_target_window(module) -> None:
    """ValueError for a gradient through forward_target with a window other than 21 unless the module was built with
    loss_head="hip": under "auto" and "torch" the head's backward stays on the 21-tap kernels (nqa_window_moments,
    nqa_adists_ts_backward); "hip" runs their generic forms (the _n entry points) for every window in 3..63."""
    n = module._window()
    if n != ops.WINDOW and getattr(module, "loss_head", None) != "hip":
        raise ValueError(f"forward_target differentiates through 21-tap HIP kernels only, and this module has "
                         f"window_size={n}: for a gradient call adists(x, y) (as_loss=True), whose torch head "
                         "differentiates any window, or build the module with loss_head=\"hip\", whose HIP backward takes "
                         "every window in 3..63; forward_target without a gradient works for every window")


def adists_target_fits(target, window=ops.WINDOW) -> None:
    """NqaError for a target whose batch's A-DISTS scratch (_adists_y_bytes) would pass NQA_MAX_WORKSPACE_GB."""
    b, _, h, w = target.shape
    if ops._max_pairs(lambda k: _adists_y_bytes(k, h, w, window), b) < b:
        from ._lib import NqaError
        raise NqaError(f"forward_target: {b} pairs of {h} x {w} need {_adists_y_bytes(b, h, w, window)} bytes of scratch beside the "
                       "pyramid, more than NQA_MAX_WORKSPACE_GB allows: pass the target in slices (target[i:j])")


def adists_target_d(module, target, y, keep, kept=None):
    """(D, state) of adists_y_forward for a prepared target (nerf_qa_amd/target.py) as the x side.  A target is used
    WHOLE: there is no slicing by NQA_MAX_WORKSPACE_GB here, and a batch whose scratch (_adists_y_bytes) would pass that
    budget is refused with NqaError -- prepare or slice the target in smaller batches.  kept: y's pyramid where the
    caller already holds it (adists_y_forward)."""
    adists_target_fits(target, _backward_window(module))
    return adists_y_forward(module, target.x, list(target.taps), y.detach().float().contiguous(), keep=keep, kept=kept)


class AdistsTargetLoss(torch.autograd.Function):
    """(prepared target, y) -> 1 - mean(D) of A-DISTS (as_loss) or 1 - D (B,), differentiable in y: AdistsLossY for a
    target whose taps are already there.  The forward is adists_y_forward -- ONE kept pyramid of y, the front, the six
    window stages and the chain, in f32s -- and keeps its state; the backward is adists_y_backward on it, with u = dL/dD
    formed on the device.  No pyramid of x, no second pass over y, no device -> host read."""

    @staticmethod
    def forward(ctx, y, target, module, as_loss):
        d, state = adists_target_d(module, target, y, keep=True)
        ctx.module, ctx.target, ctx.state, ctx.as_loss = module, target, state, as_loss
        ctx.save_for_backward(y)
        return 1 - d.mean() if as_loss else 1 - d

    @staticmethod
    def backward(ctx, grad):
        (y,) = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        u = _loss_u(grad, y.shape[0], ctx.as_loss)
        t = ctx.target
        gy = adists_y_backward(ctx.module, t.x, list(t.taps), y.detach().float().contiguous(), ctx.state, u)
        return gy.to(y.dtype), None, None, None


class PyramidTaps(torch.autograd.Function):
    """images (n,3,H,W) -> the five tapped maps relu1_2 .. relu5_3 as float NCHW tensors, differentiable in the images
    (ADISTS.forward(as_loss=True) runs forward_once WITH autograd, ADISTS.py:139-141; the frozen VGG weights get no
    gradient).  Values from the fused f32s forward; backward = pyramid_keep + pyramid_backward_device."""

    @staticmethod
    def forward(ctx, imgs, module):
        prec = "f32s"
        imgs = imgs.float().contiguous()
        taps = ops.vgg_pyramid(imgs, module._packed_weights(imgs.device, prec), prec, module._ws)
        ctx.module = module
        ctx.save_for_backward(imgs)
        return tuple(ops.nhwc_to_nchw_f32(t, prec) for t in taps)

    @staticmethod
    def backward(ctx, *grads):
        (imgs,) = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None
        acts, taps, pooled = pyramid_keep(ctx.module, imgs)
        g_taps = [(torch.zeros_like(t) if g is None else g.detach().float().permute(0, 2, 3, 1).contiguous())
                  for g, t in zip(grads, taps)]
        return pyramid_backward_device(ctx.module, acts, taps, pooled, g_taps), None


class DistsSimilarities(torch.autograd.Function):
    """(x, y) -> (S1, S2), each (B, 1475), differentiable in x and y."""

    @staticmethod
    def forward(ctx, x, y, module):
        prec = "f32s"  # gradients are formed in float precision; the values come from the same mode for consistency
        s1, s2 = ops.dists_forward(x, y, module._packed_weights(x.device, prec), prec, module._ws)
        ctx.module = module
        ctx.save_for_backward(x, y)
        return s1, s2

    @staticmethod
    def backward(ctx, g1, g2):
        x, y = ctx.saved_tensors
        gx, gy = dists_backward(ctx.module, x, y, g1.contiguous(), g2.contiguous(), need=ctx.needs_input_grad[:2])
        return gx, gy, None


@torch.no_grad()
def dists_target_stats(target, y, ty):
    """(S1, S2, kept: TargetStats) of a prepared target against y (float32 contiguous) with taps ty: per tap 1..5 the
    sums kernel and the fold (ops.dists_stats_target), tap 0 through _image_stats."""
    b, dev = y.shape[0], y.device
    s1 = torch.empty((b, ops.TOTAL_CHNS), dtype=torch.float32, device=dev)
    s2 = torch.empty((b, ops.TOTAL_CHNS), dtype=torch.float32, device=dev)
    off, parts = 3, []
    for fx, fy in zip(target.taps, ty):
        parts.append(ops.dists_stats_target(fx, fy, s1, s2, off))
        off += fx.shape[-1]
    fx0, fy0, a1, a2, scratch = _image_stats(target.x, y)
    s1[:, :3] = a1[:, :3]
    s2[:, :3] = a2[:, :3]
    return s1, s2, TargetStats(parts, fx0, fy0, scratch)


def dists_target_similarities(module, target, y):
    """(S1, S2) of a prepared target against y with no gradient to form: y's taps by pyramid_taps, the statistics of
    DistsTargetSimilarities, nothing kept."""
    y = y.detach().float().contiguous()
    s1, s2, _ = dists_target_stats(target, y, pyramid_taps(module, y))
    return s1, s2


@torch.no_grad()
def dists_target_forward(module, target, y):
    """(S1, S2, state) of a prepared target against y (float32 contiguous) WITH what a gradient needs: ONE kept pyramid
    of y (pyramid_keep) and the statistics, whose fp64 partials are kept.  state: DistsTargetState."""
    pyramid = pyramid_keep(module, y)
    s1, s2, stats = dists_target_stats(target, y, pyramid.taps)
    return s1, s2, DistsTargetState(pyramid, stats)


@torch.no_grad()
def dists_target_backward(module, target, state, g1, g2):
    """dL/dy given dL/dS1, dL/dS2 (each (B, 1475)) from dists_target_forward's state: per tap the coefficient and
    gradient launches of the loss path started from the kept partials (no second sums pass, no pyramid), tap 0 from its
    kept sums, then pyramid_backward_device.  The same kernels on the same operands as dists_backward(need=(False,
    True)): that path's gradient bit for bit."""
    return _target_backward(module, state.pyramid, dists=(target, state.pyramid.taps, state.stats, g1, g2))


class DistsTargetSimilarities(torch.autograd.Function):
    """(prepared target, y) -> (S1, S2), each (B, 1475), differentiable in y: DistsSimilarities for a target whose taps
    are already there (nerf_qa_amd/target.py).  forward = dists_target_forward, whose state the Function keeps; backward
    = dists_target_backward.  Nothing of x runs, nothing is computed twice, and there is no device -> host read in
    either direction."""

    @staticmethod
    def forward(ctx, y, target, module):
        yf = y.detach().float().contiguous()
        s1, s2, state = dists_target_forward(module, target, yf)
        ctx.module, ctx.target, ctx.state, ctx.dtype = module, target, state, y.dtype
        ctx.save_for_backward(yf)
        return s1, s2

    @staticmethod
    def backward(ctx, g1, g2):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        ctx.saved_tensors  # (y itself is in the state; this is autograd's check that it was not changed in place since)
        return dists_target_backward(ctx.module, ctx.target, ctx.state, g1, g2).to(ctx.dtype), None, None


def dists_target_step_state(module, target):
    """An uninitialised state tensor (uint8) for one step of DistsTargetStep on `target` in the module's gradient rung.  A
    target is used WHOLE: NqaError where the state would pass NQA_MAX_WORKSPACE_GB or the step does not take the shape."""
    from ._lib import NqaError
    b, _, h, w = target.shape
    rung = _grad_precision(module)
    nbytes = ops.dists_target_step_bytes(b, h, w, rung)
    if not nbytes:
        raise NqaError(f"forward_target (target_step='c'): {b} pairs of {h} x {w} are more than one step takes: "
                       + ops.lib().nqa_last_error().decode())
    if ops._max_pairs(lambda k: ops.dists_target_step_bytes(k, h, w, rung), b) < b:
        raise NqaError(f"forward_target (target_step='c'): {b} pairs of {h} x {w} need a state of {nbytes} bytes, more than "
                       "NQA_MAX_WORKSPACE_GB allows: pass the target in slices (target[i:j])")
    return torch.empty(nbytes, dtype=torch.uint8, device=target.device)


class DistsTargetStep(torch.autograd.Function):
    """DistsTargetSimilarities as the library's two step calls (DISTS(target_step="c"); include/nqa.h, "the prepared-target
    loss step"): forward = nqa_dists_target_step_forward, backward = nqa_dists_target_step_backward, both on ONE state
    tensor that the Function keeps -- the launches of dists_target_forward / dists_target_backward in their order, issued
    by the library instead of from here, so (S1, S2) and dL/dy are that Function's bit for bit.  The kept part of the
    state is only read by the backward: a second backward (retain_graph=True) gives the same bits."""

    @staticmethod
    def forward(ctx, y, target, module):
        yf = y.detach().float().contiguous()
        rung = _grad_precision(module)
        state = dists_target_step_state(module, target)
        s1, s2 = ops.dists_target_step_forward(target.x, target.taps, yf, module._packed_weights(yf.device, "f32s"), rung,
                                               state)
        ctx.module, ctx.target, ctx.state, ctx.rung, ctx.dtype = module, target, state, rung, y.dtype
        ctx.save_for_backward(yf)
        return s1, s2

    @staticmethod
    def backward(ctx, g1, g2):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        (yf,) = ctx.saved_tensors
        blobs, w0 = _backward_blobs(ctx.module, yf.device, ctx.rung)
        t = ctx.target
        gy = ops.dists_target_step_backward(t.x, t.taps, yf, g1, g2, blobs, w0, ctx.rung, ctx.state)
        return gy.to(ctx.dtype), None, None


def pair_target_values(adists_module, target, y):
    """(S1, S2, D) of a prepared target against y with no gradient to form: y's taps by pyramid_taps ONCE (the target's
    owner runs them), then the statistics of dists_target_similarities and the head of adists_target_d on those taps.
    Nothing is kept."""
    y = y.detach().float().contiguous()
    ty = pyramid_taps(target.owner(), y)
    s1, s2, _ = dists_target_stats(target, y, ty)
    d, _ = adists_target_d(adists_module, target, y, keep=False, kept=(None, ty, None))
    return s1, s2, d


@torch.no_grad()
def pair_target_forward(adists_module, target, y):
    """(S1, S2, D, state) of a prepared target against y (float32 contiguous) WITH what a gradient of either metric
    needs: ONE kept pyramid of y (pyramid_keep on the target's owner), then dists_target_stats and the A-DISTS half of
    adists_y_forward on it -- the launches of dists_target_forward and of adists_target_d on the same operands, so the
    values are theirs bit for bit.  state: PairTargetState."""
    pyramid = pyramid_keep(target.owner(), y)
    s1, s2, stats = dists_target_stats(target, y, pyramid.taps)
    d, astate = adists_target_d(adists_module, target, y, keep=True, kept=pyramid)
    return s1, s2, d, PairTargetState(stats, astate)


@torch.no_grad()
def pair_target_backward(adists_module, target, y, state, g1, g2, u):
    """dL/dy from pair_target_forward's state, given dL/dS1, dL/dS2 (each (B, 1475), or both None: DISTS unused) and
    u = dL/dD (B,) on the device (or None: A-DISTS unused): _target_backward with both metrics, A-DISTS' tap gradients
    written first and DISTS' added into them, one chain over the sum on the target's owner's weight blobs.  An unused
    metric runs none of its launches; the result is then dists_target_backward's / adists_y_backward's bit for bit."""
    pyramid = state.adists.pyramid
    return _target_backward(target.owner(), pyramid,
                            None if u is None else (adists_module, target.x, list(target.taps), y, state.adists, u),
                            None if g1 is None else (target, pyramid.taps, state.stats, g1, g2))


class PairTargetLoss(torch.autograd.Function):
    """(prepared target, y) -> (S1, S2, a): DISTS' similarities, each (B, 1475), and A-DISTS' 1 - mean(D) (as_loss) or
    1 - D (B,), all differentiable in y and hanging on ONE node: DistsTargetSimilarities and AdistsTargetLoss for a loss
    that sums the two metrics (nerf_qa_amd/pair.py, forward_target).  forward = pair_target_forward, whose state the
    Function keeps; backward = pair_target_backward with u = dL/dD formed on the device.  A value the loss never used
    arrives as None and runs nothing.  No device -> host read in either direction."""

    @staticmethod
    def forward(ctx, y, target, adists_module, as_loss):
        yf = y.detach().float().contiguous()
        s1, s2, d, state = pair_target_forward(adists_module, target, yf)
        ctx.owner = target.owner()  # (the target holds it weakly; the backward needs its weights)
        ctx.adists, ctx.target, ctx.state, ctx.as_loss, ctx.dtype = adists_module, target, state, as_loss, y.dtype
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(yf)
        return s1, s2, (1 - d.mean() if as_loss else 1 - d)

    @staticmethod
    def backward(ctx, g1, g2, ga):
        if not ctx.needs_input_grad[0] or (g1 is None and g2 is None and ga is None):
            return None, None, None, None
        (y,) = ctx.saved_tensors
        b = y.shape[0]
        u = None if ga is None else _loss_u(ga, b, ctx.as_loss)
        if (g1 is None) != (g2 is None):  # a loss over one of S1 / S2 alone: the other's upstream is zero
            zero = torch.zeros((b, ops.TOTAL_CHNS), dtype=torch.float32, device=y.device)
            g1, g2 = (zero if g1 is None else g1), (zero if g2 is None else g2)
        gy = pair_target_backward(ctx.adists, ctx.target, y, ctx.state, g1, g2, u)
        return gy.to(ctx.dtype), None, None, None


class FeatsSimilarities(torch.autograd.Function):
    """(feats0[0..5], feats1[0..5]) -> (S1, S2), each (B, sum C), differentiable in all twelve maps: forward_from_feats
    under autograd (DISTS_pt.py:181-202; the training loss of the reference's no-reference models, model_nr_v8.py:258-265).
    Values from the same statistics kernel as the no-grad call; backward = two launches of csrc/nqa_stats_backward.hip
    on the forward's fp64 sums, for the maps that need a gradient only.  Each gradient comes back in its map's dtype and
    shape."""

    @staticmethod
    def forward(ctx, *feats):
        f = [ops._f32c(t) for t in feats]
        s1, s2, scratch = ops.dists_stats_nchw(f[:6], f[6:], keep_scratch=True)
        ctx.save_for_backward(*f)
        ctx.scratch = scratch
        ctx.dtypes = [t.dtype for t in feats]
        return s1, s2

    @staticmethod
    def backward(ctx, g1, g2):
        f = ctx.saved_tensors
        need = list(ctx.needs_input_grad)
        if not any(need):
            return (None,) * 12
        gx, gy = ops.dists_stats_nchw_backward(f[:6], f[6:], ctx.scratch, g1, g2, need[:6], need[6:])
        return tuple(None if g is None else g.to(dt) for g, dt in zip(gx + gy, ctx.dtypes))


class WindowMoments(torch.autograd.Function):
    """(x, y | None, window = 21) -> the window x window Gaussian window means of NCHW maps (ops.window_moments: two maps of
    x alone, five of a pair), differentiable in both: what the A-DISTS head is built from (ADISTS.py:79-86, :165-175).
    Saves x and y only; the backward is one launch of csrc/nqa_window_moments.hip (21) or csrc/nqa_window_moments_n.hip
    (every other window in 3..63) for the sides that need a gradient, in which no window's term can reach a pixel
    outside that window.  Gradients come back in the inputs' dtype and shape."""

    @staticmethod
    def forward(ctx, x, y=None, window=ops.WINDOW):
        fx, fy = ops._f32c(x), None if y is None else ops._f32c(y)
        ctx.save_for_backward(fx, fy)
        ctx.set_materialize_grads(False)  # an unused map's gradient stays None: its pass of the backward is skipped
        ctx.dtypes = (x.dtype, None if y is None else y.dtype)
        ctx.window = ops.check_window(window)
        return ops.window_moments(fx, fy, ctx.window)

    @staticmethod
    def backward(ctx, *grads):
        fx, fy = ctx.saved_tensors
        need = (ctx.needs_input_grad[0], fy is not None and ctx.needs_input_grad[1])
        if not any(need):
            return None, None, None
        extra = {} if ctx.window == ops.WINDOW else {"window": ctx.window}  # (the default window: the call as it always was)
        gx, gy = ops.window_moments_backward(fx, fy, grads, need, **extra)
        return (None if gx is None else gx.to(ctx.dtypes[0])), (None if gy is None else gy.to(ctx.dtypes[1])), None
