"""DISTS and A-DISTS of the same frames from ONE VGG pyramid.

The reference's offline scoring loops ask for both metrics of every batch (prep.py:185-190, test2_prep.py:146-193,
data_prep.py:57-104):

    adists_model(ref, render, as_loss=False)
    dists_model(ref, render, batch_average=False)

Both run the same frozen VGG-16 over the same 2B images.  A-DISTS already forms, for its channel norms and global-branch
moments, the fp64 per-(pair, channel) sums of all six taps with the statistics kernels DISTS uses; DISTS' S1 / S2 are
one finalisation launch on those sums (include/nqa.h, nqa_adists_dists_forward).  score_pair returns what the two
modules' own forward calls return, for the cost of the A-DISTS call.

What score_pair and score_group do not do: image gradients (that is forward_target below: both metrics as ONE loss
against a prepared target, one kept pyramid of the render and one backward chain per step; for any other gradient use
the modules separately), and the DISTS fast rungs -- the pair runs in A-DISTS'
precision (f32 / f32s under its `auto`, or its named mode), which is at least as accurate as any rung DISTS' `auto`
would pick; the DISTS calibration and the flat-frame guard are not consulted, and nothing here waits on the host after
the first call for a (device, weights, size), so the call can be captured into a hipGraph.
"""
from __future__ import annotations

import weakref

import torch

from . import ops
from ._lib import NqaError, prec_id

_SAME_WEIGHTS = weakref.WeakKeyDictionary()  # adists module -> {(device, both weights keys): verdict}


def pair_precision(dists_model, adists_model, h: int, w: int) -> str:
    """The mode score_pair runs frames of h x w in: A-DISTS' (a function of the frame size alone).  A DISTS module whose
    precision is "auto" goes along; one with a NAMED precision that differs is refused."""
    prec = adists_model.precision_for(h, w)
    asked = getattr(dists_model, "precision", "auto")
    if asked != "auto" and prec_id(asked) != prec_id(prec):
        raise ValueError(f"score_pair runs {h}x{w} frames in A-DISTS' precision {prec!r}, but the DISTS module asks for "
                         f"precision={asked!r}: give both modules the same named precision, leave DISTS on 'auto', or "
                         "score with the modules separately")
    return prec


def _check_same_weights(dists_model, adists_model, dev, who="score_pair") -> None:
    """Both modules must hold the same thirteen conv layers: compared on the device once per (device, weights of both
    modules) -- one host wait, on the first call only -- and remembered."""
    key = (dists_model._weights_key(dev), adists_model._weights_key(dev))
    memo = _SAME_WEIGHTS.setdefault(adists_model, {})
    same = memo.get(key)
    if same is None:
        if len(memo) > 16:  # (weights that keep changing: do not pile verdicts up)
            memo.clear()
        same = memo[key] = all(
            a.weight.shape == b.weight.shape and torch.equal(a.weight.detach().to(dev), b.weight.detach().to(dev))
            and torch.equal(a.bias.detach().to(dev), b.bias.detach().to(dev))
            for a, b in zip(dists_model._conv_modules(), adists_model._conv_modules()))
    if not same:
        raise NqaError(f"{who}: the DISTS and the A-DISTS module hold different VGG-16 weights "
                       f"({getattr(dists_model, 'vgg_source', '?')} vs {getattr(adists_model, 'vgg_source', '?')}); "
                       "one shared pyramid cannot serve both -- score with the modules separately")


def score_pair(dists_model, adists_model, x, y, batch_average=False, as_loss=False, as_map=False):
    """(dists_model(x, y, batch_average=batch_average), adists_model(x, y, as_loss=as_loss, as_map=as_map)) from one
    pyramid: each value has the shape, dtype and meaning of that module's own forward for those flags (the A-DISTS half
    bit for bit; the DISTS half as DISTS(precision=<pair precision>), through the module's own alpha / beta weighting, so
    alpha and beta receive gradients as in its forward).  x is the reference frame for both (prep.py:186-189).

    Raises ValueError for shapes that differ, images that require grad, or a DISTS module with a named precision other
    than the one the pair runs in (pair_precision); NqaError for modules with different VGG weights or tensors off the
    GPU."""
    if x.shape != y.shape or x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"expected two (B,3,H,W) tensors of equal shape, got {tuple(x.shape)} / {tuple(y.shape)}")
    if torch.is_grad_enabled() and (x.requires_grad or y.requires_grad):
        raise ValueError("score_pair does not differentiate through the shared pyramid: detach the images, or call the "
                         "modules separately (DISTS(require_grad=True), ADISTS(as_loss=True))")
    h, w = int(x.shape[-2]), int(x.shape[-1])
    prec = pair_precision(dists_model, adists_model, h, w)
    if not (x.is_cuda and y.is_cuda):
        raise NqaError("nerf_qa_amd runs on the GPU only: got tensors on %s / %s (move inputs and the modules to cuda; "
                       "there is no CPU fallback)" % (x.device, y.device))
    dev = x.device
    _check_same_weights(dists_model, adists_model, dev)
    ws, n = adists_model._ws, adists_model._window()
    with torch.no_grad():
        if as_map:
            d, s1, s2, m = ops.adists_dists_forward(x, y, adists_model._packed_weights(dev, prec), prec, ws, with_map=True,
                                                    window=n)
            b = m.shape[0]
            a_out = m.unsqueeze(1).expand(b, b, *m.shape[1:]).contiguous()  # (ADISTS.forward: the reference's broadcast)
        else:
            d, s1, s2 = adists_model._batched(
                x, y, prec, lambda a, b, packed: ops.adists_dists_forward(a, b, packed, prec, ws, window=n))
            a_out = 1 - d.mean() if as_loss else 1 - d
    return dists_model._weighted(s1, s2, batch_average), a_out


def score_group(dists_model, adists_model, ref, renders):
    """(DISTS (R,K), A-DISTS (R,K)) of K renders against ONE reference for R such groups, from one pyramid of R + R*K
    images: ref (R,3,H,W), renders (R,K,3,H,W), entry [r, k] the pair (ref[r], renders[r, k]) with x = the reference.
    The contract of score_pair for batch_average=False, as_loss=False: the A-DISTS half is
    adists_model.forward_group(ref, renders) bit for bit; the DISTS half is DISTS(precision=<pair precision>)
    .forward_group, folded from the sums A-DISTS forms anyway, through the module's own alpha / beta weighting.  The pair
    runs in A-DISTS' precision (pair_precision).  Raises as score_pair does."""
    r, k, h, w = adists_model._group_checks(ref, renders, "score_group")
    prec = pair_precision(dists_model, adists_model, h, w)
    dev = ref.device
    _check_same_weights(dists_model, adists_model, dev)
    with torch.no_grad():
        d, s1, s2 = ops.adists_forward_group(ref, renders, adists_model._packed_weights(dev, prec), prec, adists_model._ws,
                                             with_dists=True, window=adists_model._window())
    return dists_model._weighted(s1, s2, False).reshape(r, k), (1 - d).reshape(r, k)


def forward_target(dists_model, adists_model, target, y, batch_average=False, as_loss=True):
    """(dists_model.forward_target(target, y, require_grad=True, batch_average=batch_average),
    adists_model.forward_target(target, y, as_loss=as_loss)) for a loss that uses BOTH metrics against one prepared
    target: each value has the shape, dtype and meaning of that module's own call, bit for bit.  Always in f32s; the
    DISTS half goes through the module's own alpha / beta weighting, so alpha and beta receive gradients as everywhere.

    Where y requires grad (grad mode on) both values hang on ONE autograd node (autograd.PairTargetLoss): a step is one
    kept pyramid of y for both heads and, whatever loss is built from the two values, ONE backward chain over the sum
    of their tap gradients -- against two pyramids and two chains for the two modules' calls.  A value the loss does not
    use costs nothing in the backward, and y.grad is then the other module's own bit for bit.  Nothing is read back to
    the host.  Without a gradient to form, y gives its taps once and both heads run on them; nothing is kept.

    `target` comes from the prepare_target of EITHER module (with equal VGG weights both prepare the same taps).
    The gradient chain runs in the two modules' grad_precision, which must be the same ("f32s" | "f16").
    ValueError for modules that name different ones, a target of a third module, one prepared before its owner's VGG
    weights changed, and a shape that does not fit; NqaError for modules with different VGG weights, tensors off the GPU, and a batch whose A-DISTS
    scratch would pass NQA_MAX_WORKSPACE_GB (pass target[i:j] slices); ValueError too where y requires grad, the A-DISTS
    module's window_size is not 21 and its loss_head is not "hip" (ADISTS.forward_target): with loss_head="hip" the pair
    step differentiates at every window in 3..63."""
    from . import autograd, target as tgt
    gp = [getattr(m, "grad_precision", "f32s") for m in (dists_model, adists_model)]
    if gp[0] != gp[1]:  # (one chain carries both metrics' gradients: the same kind of rule as pair_precision)
        raise ValueError(f"forward_target runs ONE gradient chain for both metrics, but the DISTS module asks for "
                         f"grad_precision={gp[0]!r} and the A-DISTS module for {gp[1]!r}: give both the same")
    tgt.check_pair(dists_model, adists_model, target, y)
    _check_same_weights(dists_model, adists_model, y.device, "forward_target")
    autograd.adists_target_fits(target, autograd._backward_window(adists_model))
    if torch.is_grad_enabled() and y.requires_grad:
        autograd.check_target_window(adists_model)
        s1, s2, a = autograd.PairTargetLoss.apply(y, target, adists_model, bool(as_loss))
    else:
        s1, s2, d = autograd.pair_target_values(adists_model, target, y)
        a = 1 - d.mean() if as_loss else 1 - d
    return dists_model._weighted(s1, s2, batch_average), a
