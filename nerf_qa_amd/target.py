"""A prepared target: the fixed side of a loss, run through the pyramid ONCE.

When a render y is optimised against a ground-truth frame x, x is the same at every iteration, and so are its five
tapped maps.  `DISTS.prepare_target(x)` / `ADISTS.prepare_target(x)` compute them once (autograd.pyramid_taps: the very
launches the loss path uses, so that a gradient does not depend on which interface asked for it), and
`forward_target(target, y, ...)` then runs one kept pyramid of y per step and nothing of x (autograd.py,
DistsTargetSimilarities / AdistsTargetLoss).

A target belongs to the module that prepared it and to that module's VGG weights as they were then: it carries the
module's `_weights_key`, and a target whose key no longer matches is refused.  It holds device tensors of one process and
does not pickle, as the scratch fields of the modules never travel.  (pair.forward_target, both metrics as one loss, takes
a target of either of its two modules: check_pair.)
"""
from __future__ import annotations

import weakref

import torch

from ._lib import NqaError


class PreparedTarget:
    """x (B,3,H,W) as contiguous float32 and its five float NHWC taps relu1_2 .. relu5_3, all detached; `key` is the
    preparing module's _weights_key, `owner` a weak reference to that module."""

    __slots__ = ("x", "taps", "key", "owner", "kind")

    def __init__(self, x, taps, key, owner, kind):
        self.x, self.taps, self.key, self.owner, self.kind = x, tuple(taps), key, owner, kind

    @property
    def shape(self):
        return self.x.shape

    @property
    def device(self):
        return self.x.device

    @property
    def nbytes(self) -> int:
        """Device bytes the target holds (a slice reports its own share of the storage it views)."""
        return sum(t.numel() * t.element_size() for t in (self.x,) + self.taps)

    def __len__(self) -> int:
        return int(self.x.shape[0])

    def __getitem__(self, s):
        """target[i:j]: the same pairs' frames and taps as VIEWS (no copy); only a slice of step 1 is taken (a single pair
        is target[i:i+1]; for any other selection see select)."""
        if not isinstance(s, slice) or s.step not in (None, 1):
            raise TypeError("a prepared target is sliced as target[i:j] (views); use target.select(indices) to gather")
        sub = PreparedTarget(self.x[s], [t[s] for t in self.taps], self.key, self.owner, self.kind)
        if len(sub) == 0:
            raise ValueError(f"the slice {s.start}:{s.stop} of a target of {len(self)} frames is empty")
        return sub

    def select(self, idx) -> "PreparedTarget":
        """A NEW target of the frames idx (a LongTensor of indices into the batch, in that order, repeats allowed)."""
        if not torch.is_tensor(idx) or idx.dtype != torch.long or idx.dim() != 1 or idx.numel() == 0:
            raise ValueError("select expects a non-empty 1-D LongTensor of frame indices")
        idx = idx.to(self.x.device)
        return PreparedTarget(self.x.index_select(0, idx), [t.index_select(0, idx) for t in self.taps], self.key,
                              self.owner, self.kind)

    def __reduce_ex__(self, protocol):
        raise TypeError("a prepared target holds device tensors tied to one module's packed weights and does not pickle: "
                        "keep the frames and call prepare_target again where they are needed")

    def __repr__(self):
        return f"PreparedTarget({self.kind}, shape={tuple(self.shape)}, device={self.device}, {self.nbytes} bytes)"


def _gpu_image(who: str, t, name: str):
    if not torch.is_tensor(t) or t.dim() != 4 or t.shape[1] != 3 or t.numel() == 0:
        raise ValueError(f"{who} expects {name} of shape (B,3,H,W), got {tuple(getattr(t, 'shape', ()))}")
    if not t.is_cuda:
        raise NqaError("nerf_qa_amd runs on the GPU only: got a tensor on %s "
                       "(move inputs and the module to cuda; there is no CPU fallback)" % t.device)


def prepare(module, x, kind: str) -> PreparedTarget:
    """What DISTS.prepare_target and ADISTS.prepare_target share."""
    from . import autograd
    _gpu_image("prepare_target", x, "x")
    if torch.is_grad_enabled() and x.requires_grad:
        raise ValueError("prepare_target takes the FIXED side of a loss and gives it no gradient: detach the frames (for a "
                         "gradient towards x use forward with both images)")
    given, x = x, x.detach().float().contiguous()
    if x.data_ptr() == given.data_ptr():  # the target's own copy: the caller's tensor may change, the taps would not
        x = x.clone()
    taps = autograd.pyramid_taps(module, x)
    return PreparedTarget(x, [t.detach() for t in taps], module._weights_key(x.device), weakref.ref(module), kind)


def check(module, target, y, kind: str) -> None:
    """The argument checks of forward_target: ValueError for a target that is not this module's or not current and for
    shapes that do not fit, NqaError for tensors off the GPU."""
    if not isinstance(target, PreparedTarget):
        raise ValueError(f"forward_target expects what prepare_target returned, got {type(target).__name__}")
    if target.kind != kind or target.owner() is not module:
        raise ValueError(f"this target was prepared by another module ({target.kind}): a target belongs to the module "
                         "instance whose prepare_target made it")
    _check_current(module, target, y)


def check_pair(dists_module, adists_module, target, y) -> None:
    """check for pair.forward_target, which takes a target of EITHER of its two modules (both prepare the same taps when
    they hold the same VGG weights, which the caller verifies): the target's owner must be one of the two, under its own
    kind, and the target current for THAT module.  (A module's own forward_target goes on refusing
    the other module's targets: check is unchanged.)"""
    if not isinstance(target, PreparedTarget):
        raise ValueError(f"forward_target expects what prepare_target returned, got {type(target).__name__}")
    owner = target.owner()
    if owner is None or not ((target.kind == "DISTS" and owner is dists_module) or
                             (target.kind == "ADISTS" and owner is adists_module)):
        raise ValueError(f"this target was prepared by another module ({target.kind}): pair.forward_target takes a target "
                         "made by the prepare_target of one of its two modules")
    _check_current(owner, target, y)


def _check_current(module, target, y) -> None:
    """What check and check_pair ask of y and of the target once its owner is settled."""
    _gpu_image("forward_target", y, "y")
    if y.device != target.device:
        raise NqaError("tensors on different devices")
    if target.key != module._weights_key(y.device):
        raise ValueError("this target was prepared before the module's VGG weights changed (or moved): its taps are stale, "
                         "call prepare_target again")
    if tuple(y.shape) != tuple(target.shape):
        raise ValueError(f"target and y differ in shape: {tuple(target.shape)} vs {tuple(y.shape)}")
