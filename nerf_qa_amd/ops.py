"""Tensor-level wrappers over the C ABI (include/nqa.h).

PyTorch is plumbing here: it owns device memory and the current HIP stream; every
number is produced by the kernels in libnqa_hip.so.  All functions require CUDA (ROCm)
tensors and raise otherwise -- there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import operator
import os
from typing import List, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import NUM_CONVS, PREC_DTYPE, TOTAL_CHNS, check, lib, prec_id, ptr, stream_ptr

CHNS = (3, 64, 128, 256, 512, 512)
CONV_COUT = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
CONV_CIN = (3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512)
CONV_STAGE = (0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4)


def _need_cuda(*ts: torch.Tensor) -> torch.device:
    dev = ts[0].device
    for t in ts:
        if not t.is_cuda:
            raise _lib.NqaError("nerf_qa_amd runs on the GPU only: got a tensor on %s "
                                "(move inputs and the module to cuda; there is no CPU fallback)" % t.device)
        if t.device != dev:
            raise _lib.NqaError("tensors on different devices")
    return dev


def _on(dev: torch.device):
    """The library launches on the current HIP device: make that the tensors' device for the duration of the
    call and restore the caller's afterwards (a process that drives several GPUs from one thread would
    otherwise launch on the wrong one -- or, if we left it switched, allocate on the wrong one later)."""
    return torch.cuda.device(dev)


def _call(dev: torch.device, fn, *args) -> None:
    if dev.index is not None and dev.index != torch.cuda.current_device():
        with _on(dev):
            check(fn(*args))
    else:
        check(fn(*args))


def _f32c(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def pyramid_dims(h: int, w: int):
    dims = [(h, w)]
    for _ in range(4):
        h, w = (h + 1) // 2, (w + 1) // 2
        dims.append((h, w))
    return dims


def pack_vgg_weights(convs: Sequence, prec) -> torch.Tensor:
    """13 (weight OIHW, bias) pairs (numpy or torch, any device) -> packed blob (CPU uint8 tensor)."""
    p = prec_id(prec)
    if len(convs) != NUM_CONVS:
        raise ValueError("expected 13 conv layers")
    ws, bs = [], []
    for li, (w, b) in enumerate(convs):
        w = np.ascontiguousarray(w.detach().cpu().numpy() if torch.is_tensor(w) else w, dtype=np.float32)
        b = np.ascontiguousarray(b.detach().cpu().numpy() if torch.is_tensor(b) else b, dtype=np.float32)
        if w.shape != (CONV_COUT[li], CONV_CIN[li], 3, 3) or b.shape != (CONV_COUT[li],):
            raise ValueError(f"conv {li}: unexpected shape {w.shape} / {b.shape}")
        ws.append(w)
        bs.append(b)
    nbytes = lib().nqa_packed_weights_bytes(p)
    blob = torch.empty(nbytes, dtype=torch.uint8)
    wp = (C.c_void_p * NUM_CONVS)(*[w.ctypes.data for w in ws])
    bp = (C.c_void_p * NUM_CONVS)(*[b.ctypes.data for b in bs])
    check(lib().nqa_pack_vgg_weights(wp, bp, p, blob.data_ptr()))
    return blob


TAP_LAYERS = (1, 3, 6, 9, 12)  # conv layers whose output is tapped (relu1_2 .. relu5_3)


def _stage_dtype(p: int, stage: int) -> torch.dtype:
    """Element type of the maps of pyramid stage `stage` (0-based) in mode p: in a mixed mode the stage's own."""
    return PREC_DTYPE[_lib.stage_prec(p, stage)]


def conv1_1(x: torch.Tensor, packed: torch.Tensor, prec) -> torch.Tensor:
    """relu1_1 as NHWC in prec's activation format ("f32s": split16 bytes in a float32 tensor, see
    include/nqa.h Layouts; split16_decode turns them into floats).  A mixed mode: the exact float conv, half out."""
    p = prec_id(prec)
    dev = _need_cuda(x, packed)
    x = _f32c(x)
    n, c, h, w = x.shape
    assert c == 3
    out = torch.empty((n, h, w, 64), dtype=_stage_dtype(p, 0), device=dev)
    _call(dev, lib().nqa_conv1_1, ptr(x), n, h, w, ptr(packed), p, ptr(out), stream_ptr(dev))
    return out


def _out_or_empty(out, shape, dtype, dev: torch.device) -> torch.Tensor:
    """A caller-owned output (tests pre-fill it, so that a store the kernel skipped shows) or a fresh torch.empty."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    _need_cuda(out)
    assert out.device == dev and out.dtype == dtype and tuple(out.shape) == tuple(shape) and out.is_contiguous()
    return out


def conv1_fused(x: torch.Tensor, packed: torch.Tensor, prec, out: torch.Tensor | None = None) -> torch.Tensor:
    """relu1_2 (NHWC) straight from the image: conv1_1 + conv1_2 in one kernel (16-bit modes and "f32s": float out; a
    mixed mode: two-term weights, half out, only where the pyramid fuses stage 1 -- NqaError for W < 16).  out: a
    contiguous tensor of the result's shape and dtype to write into instead of a new one."""
    p = prec_id(prec)
    dev = _need_cuda(x, packed)
    x = _f32c(x)
    n, c, h, w = x.shape
    assert c == 3
    out = _out_or_empty(out, (n, h, w, 64), _stage_dtype(p, 0), dev)
    _call(dev, lib().nqa_conv1_fused, ptr(x), n, h, w, ptr(packed), p, ptr(out), stream_ptr(dev))
    return out


def conv3x3_relu(inp: torch.Tensor, layer: int, packed: torch.Tensor, prec, out: torch.Tensor | None = None) -> torch.Tensor:
    """One VGG conv layer, NHWC.  "f32s": split16 in; float out for TAP_LAYERS, split16 out otherwise.  A mixed mode:
    half in and out where the layer's stage is a 16-bit one, the f32s formats behind it.  out: as conv1_fused's."""
    p = prec_id(prec)
    dev = _need_cuda(inp, packed)
    assert inp.dtype == _stage_dtype(p, CONV_STAGE[layer]) and inp.is_contiguous()
    n, h, w, c = inp.shape
    assert c == CONV_CIN[layer]
    out = _out_or_empty(out, (n, h, w, CONV_COUT[layer]), inp.dtype, dev)
    _call(dev, lib().nqa_conv3x3_relu, ptr(inp), n, h, w, layer, ptr(packed), p, ptr(out), stream_ptr(dev))
    return out


def l2pool(inp: torch.Tensor, prec) -> torch.Tensor:
    """L2-pool of a tapped map, NHWC.  "f32s": float in, split16 out (it feeds the next conv).  A mixed mode: the pool
    between two of its 16-bit stages (half in, half out); its boundary pool is l2pool_f16_to_split16."""
    p = prec_id(prec)
    dev = _need_cuda(inp)
    assert inp.dtype == _stage_dtype(p, 0) and inp.is_contiguous()
    n, h, w, c = inp.shape
    out = torch.empty((n, (h + 1) // 2, (w + 1) // 2, c), dtype=inp.dtype, device=dev)
    _call(dev, lib().nqa_l2pool, ptr(inp), n, h, w, c, p, ptr(out), stream_ptr(dev))
    return out


def l2pool_f16_to_split16(inp: torch.Tensor) -> torch.Tensor:
    """The L2-pool behind a mixed mode's last 16-bit stage: half NHWC in, split16 records out (float32-typed tensor)."""
    dev = _need_cuda(inp)
    assert inp.dtype == torch.float16 and inp.is_contiguous()
    n, h, w, c = inp.shape
    out = torch.empty((n, (h + 1) // 2, (w + 1) // 2, c), dtype=torch.float32, device=dev)
    _call(dev, lib().nqa_l2pool_f16_to_split16, ptr(inp), n, h, w, c, ptr(out), stream_ptr(dev))
    return out


def conv_pool_stats(inp: torch.Tensor, layer: int, packed: torch.Tensor, prec, pooled: torch.Tensor | None = None,
                    sums: torch.Tensor | None = None):
    """The stage-closing conv `layer` + ReLU + L2-pool + statistics sums in ONE kernel (include/nqa.h,
    nqa_conv_pool_stats): `inp` is the 2B-image NHWC batch of the layer's input (x images then y images); returns
    (pooled (2B, ceil(H/2), ceil(W/2), Cout) in the next stage's input dtype, sums float64 (B, Cout, 5) = sum x, sum y,
    sum x^2, sum y^2, sum xy over the tap's pixels).  Raises NqaError where no fused form exists (only conv2_2 so far).  pooled, sums:
    contiguous tensors of those shapes and dtypes to write into instead of new ones."""
    p = prec_id(prec)
    dev = _need_cuda(inp, packed)
    assert inp.is_contiguous() and inp.shape[0] % 2 == 0
    n, h, w, c = inp.shape
    assert c == CONV_CIN[layer]
    b = n // 2
    cout = CONV_COUT[layer]
    pooled = _out_or_empty(pooled, (n, (h + 1) // 2, (w + 1) // 2, cout),
                           PREC_DTYPE[_lib.stage_prec(p, CONV_STAGE[layer] + 1)] if p in _lib.MIXED_STAGES else inp.dtype, dev)
    sums = _out_or_empty(sums, (b, cout, 5), torch.float64, dev)
    nbytes = lib().nqa_conv_pool_workspace_bytes(b, h, w, layer)
    ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
    _call(dev, lib().nqa_conv_pool_stats, ptr(inp), b, h, w, layer, ptr(packed), p, ptr(pooled), ptr(sums), ptr(ws), ws.numel(),
          stream_ptr(dev))
    return pooled, sums


def conv1_pool_stats(x: torch.Tensor, y: torch.Tensor, packed: torch.Tensor, prec, pooled: torch.Tensor | None = None,
                     sums: torch.Tensor | None = None):
    """Stage 1 + L2-pool + tap-1 statistics in ONE kernel from the raw frames (include/nqa.h, nqa_conv1_pool_stats):
    x, y (B,3,H,W) float32 -> (pooled relu1_2 (2B, ceil(H/2), ceil(W/2), 64) f16 NHWC, x images first; sums float64 (B, 64, 5)).
    pooled, sums: as conv_pool_stats'."""
    p = prec_id(prec)
    dev = _need_cuda(x, y, packed)
    x, y = _f32c(x), _f32c(y)
    b, c, h, w = x.shape
    assert c == 3 and y.shape == x.shape
    pooled = _out_or_empty(pooled, (2 * b, (h + 1) // 2, (w + 1) // 2, 64), torch.float16, dev)
    sums = _out_or_empty(sums, (b, 64, 5), torch.float64, dev)
    nbytes = lib().nqa_conv_pool_workspace_bytes(b, h, w, 1)
    ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
    _call(dev, lib().nqa_conv1_pool_stats, ptr(x), ptr(y), b, h, w, ptr(packed), p, ptr(pooled), ptr(sums), ptr(ws), ws.numel(),
          stream_ptr(dev))
    return pooled, sums


def _pair_maps(who: str, feat: torch.Tensor, b: int, p: int, dims: int) -> None:
    if p not in PREC_DTYPE:
        raise ValueError(f"{who}: prec {p} is not one of the kernel-level modes")
    if feat.dim() != dims or int(b) <= 0 or feat.shape[0] != 2 * int(b) or feat.numel() == 0 or feat.dtype != PREC_DTYPE[p] \
            or not feat.is_contiguous():
        raise ValueError(f"{who}: expected contiguous {PREC_DTYPE[p]} ({2 * int(b)}, {'H, W' if dims == 4 else 'HW'}, C), "
                         f"the x maps then the y maps, got {feat.dtype} {tuple(feat.shape)}")


def pool_stats(feat: torch.Tensor, b: int, prec, pooled: torch.Tensor | None = None, sums: torch.Tensor | None = None,
               to_split16: bool = False):
    """L2-pool + the five statistics sums of ONE tap in one pass, as the pair forwards launch it (include/nqa.h,
    nqa_pool_stats): feat (2b, H, W, C) NHWC in prec's storage type, the b x maps then the b y maps -> (pooled (2b,
    ceil(H/2), ceil(W/2), C) as l2pool writes it -- split16 records in a float32 tensor for "f32s" -- and sums float64
    (b, C, 5) = sum x, sum y, sum x^2, sum y^2, sum xy).  to_split16: the mixed modes' boundary form (prec "f16": half in,
    split16 records out).  pooled, sums: as conv_pool_stats'."""
    p = prec_id(prec)
    dev = _need_cuda(feat)
    _pair_maps("pool_stats", feat, b, p, 4)
    if to_split16 and p != _lib.PREC_F16:
        raise ValueError("pool_stats: to_split16 is the f16 -> split16 boundary form (prec 'f16')")
    n, h, w, c = feat.shape
    b = int(b)
    pooled = _out_or_empty(pooled, (n, (h + 1) // 2, (w + 1) // 2, c), torch.float32 if to_split16 else feat.dtype, dev)
    sums = _out_or_empty(sums, (b, c, 5), torch.float64, dev)
    nbytes = lib().nqa_pool_stats_workspace_bytes(b, h, w, c, p)
    ws = torch.full((max(nbytes, 256),), 0xFF, dtype=torch.uint8, device=dev)  # (a block that never ran leaves NaN sums)
    if to_split16:
        _call(dev, lib().nqa_pool_stats_f16_to_split16, ptr(feat), b, h, w, c, ptr(pooled), ptr(sums), ptr(ws), nbytes,
              stream_ptr(dev))
    else:
        _call(dev, lib().nqa_pool_stats, ptr(feat), b, h, w, c, p, ptr(pooled), ptr(sums), ptr(ws), nbytes, stream_ptr(dev))
    return pooled, sums


def stats_nhwc(feat: torch.Tensor, b: int, prec, sums: torch.Tensor | None = None) -> torch.Tensor:
    """The five statistics sums of the last tap as the pair forwards launch them (include/nqa.h, nqa_stats_nhwc): feat
    (2b, HW, C) NHWC in prec's storage type, the b x maps then the b y maps -> sums float64 (b, C, 5).  sums: as
    conv_pool_stats'."""
    p = prec_id(prec)
    dev = _need_cuda(feat)
    _pair_maps("stats_nhwc", feat, b, p, 3)
    _, hw, c = feat.shape
    b = int(b)
    sums = _out_or_empty(sums, (b, c, 5), torch.float64, dev)
    nbytes = lib().nqa_stats_nhwc_workspace_bytes(b, hw, c, p)
    ws = torch.full((max(nbytes, 256),), 0xFF, dtype=torch.uint8, device=dev)  # (a block that never ran leaves NaN sums)
    _call(dev, lib().nqa_stats_nhwc, ptr(feat), b, hw, c, p, ptr(sums), ptr(ws), nbytes, stream_ptr(dev))
    return sums


def pool_stats_grid(b: int, h: int, w: int, c: int, prec) -> tuple:
    """(TR, TC, tiles across, tiles per pair, blocks of the launch) of pool_stats for these arguments, from the launcher's
    own planning function (no device is touched)."""
    g = (C.c_int * 5)()
    check(lib().nqa_pool_stats_grid(int(b), int(h), int(w), int(c), prec_id(prec), g))
    return tuple(g)


def stats_nhwc_grid(b: int, hw: int, c: int, prec) -> tuple:
    """(pixels per block, blocks per pair, pixels a block takes side by side) of stats_nhwc for these arguments."""
    g = (C.c_int * 3)()
    check(lib().nqa_stats_nhwc_grid(int(b), int(hw), int(c), prec_id(prec), g))
    return tuple(g)


def nhwc_to_nchw_f32(inp: torch.Tensor, prec) -> torch.Tensor:
    p = prec_id(prec)
    dev = _need_cuda(inp)
    assert inp.dtype == PREC_DTYPE[p] and inp.is_contiguous()
    n, h, w, c = inp.shape
    out = torch.empty((n, c, h, w), dtype=torch.float32, device=dev)
    _call(dev, lib().nqa_nhwc_to_nchw_f32, ptr(inp), n, h, w, c, p, ptr(out), stream_ptr(dev))
    return out


class Workspace:
    """Grow-only device scratch, one buffer per (module, device, HIP stream): avoids allocator traffic per call, and two
    streams that run the same module side by side (ADISTS' two half-batches) never share scratch.  At most MAX_STREAMS
    buffers are kept (the least recently used one goes first): a caller that scores from many short-lived streams does
    not pile up gigabytes of scratch."""

    MAX_STREAMS = 8

    def __init__(self):
        self.bufs = {}

    def get(self, nbytes: int, dev: torch.device) -> torch.Tensor:
        key = (str(dev), torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else 0)
        buf = self.bufs.pop(key, None)
        if buf is None or buf.numel() < nbytes:
            buf = None  # (released before the larger one is requested)
            while len(self.bufs) >= self.MAX_STREAMS:
                self.bufs.pop(next(iter(self.bufs)))
            buf = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
        self.bufs[key] = buf  # (re-inserted: most recently used last)
        return buf


def tap_prec(prec, k: int) -> int:
    """Precision id of tapped map k (0 = relu1_2 .. 4 = relu5_3) in mode `prec` ("f32m": half, half, half, float, float)."""
    return _lib.stage_prec(prec_id(prec), k)


def vgg_pyramid(x: torch.Tensor, packed: torch.Tensor, prec, ws: Workspace | None = None) -> List[torch.Tensor]:
    """Five tapped maps relu1_2..relu5_3 as NHWC tensors in prec's dtype (per tap in "f32m", see tap_prec)."""
    p = prec_id(prec)
    dev = _need_cuda(x, packed)
    x = _f32c(x)
    n, c, h, w = x.shape
    assert c == 3
    taps = [torch.empty((n, hk, wk, ck), dtype=PREC_DTYPE[_lib.stage_prec(p, k)], device=dev)
            for k, ((hk, wk), ck) in enumerate(zip(pyramid_dims(h, w), CHNS[1:]))]
    nbytes = lib().nqa_workspace_bytes(n, h, w, p)
    buf = (ws or Workspace()).get(nbytes, dev)
    tp = (C.c_void_p * 5)(*[ptr(t) for t in taps])
    _call(dev, lib().nqa_vgg_pyramid, ptr(x), n, h, w, ptr(packed), p, ptr(buf), buf.numel(), tp, stream_ptr(dev))
    return taps


def _max_pairs(bytes_for, b: int) -> int:
    """Slice size for a batch whose workspace would exceed NQA_MAX_WORKSPACE_GB (default 96, a third of an
    MI355X's HBM): the batch then runs in equal slices (pairs are independent, so the results are the same)."""
    budget = int(float(os.environ.get("NQA_MAX_WORKSPACE_GB", "96")) * (1 << 30))
    if b <= 1 or bytes_for(b) <= budget:
        return b
    lo, hi = 1, b  # bytes_for is monotone in the batch size
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if bytes_for(mid) <= budget:
            lo = mid
        else:
            hi = mid - 1
    slices = -(-b // lo)
    return -(-b // slices)  # equal slices rather than full ones plus a remainder


def dists_forward(x: torch.Tensor, y: torch.Tensor, packed: torch.Tensor, prec, ws: Workspace | None = None):
    """(S1, S2), each float32 (B, 1475): both pyramids + statistics in one enqueue."""
    p = prec_id(prec)
    dev = _need_cuda(x, y, packed)
    x, y = _f32c(x), _f32c(y)
    if x.shape != y.shape or x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"expected two (B,3,H,W) tensors of equal shape, got {tuple(x.shape)} / {tuple(y.shape)}")
    b, _, h, w = x.shape
    mb = _max_pairs(lambda n: lib().nqa_workspace_bytes(2 * n, h, w, p), b)
    if mb < b:
        parts = [dists_forward(x[i:i + mb], y[i:i + mb], packed, prec, ws) for i in range(0, b, mb)]
        return torch.cat([q[0] for q in parts]), torch.cat([q[1] for q in parts])
    s1 = torch.empty((b, TOTAL_CHNS), dtype=torch.float32, device=dev)
    s2 = torch.empty((b, TOTAL_CHNS), dtype=torch.float32, device=dev)
    nbytes = lib().nqa_workspace_bytes(2 * b, h, w, p)
    buf = (ws or Workspace()).get(nbytes, dev)
    _call(dev, lib().nqa_dists_forward, ptr(x), ptr(y), b, h, w, ptr(packed), p, ptr(buf), buf.numel(), ptr(s1), ptr(s2),
                                  stream_ptr(dev))
    return s1, s2


def _group_dims(ref: torch.Tensor, renders: torch.Tensor):
    """(R, K, H, W) of a (R,3,H,W) reference batch and its (R,K,3,H,W) renders; ValueError where they do not fit."""
    if ref.dim() != 4 or ref.shape[1] != 3 or renders.dim() != 5 or renders.shape[0] != ref.shape[0] \
            or renders.shape[2:] != ref.shape[1:] or ref.numel() == 0 or renders.numel() == 0:
        raise ValueError(f"expected references (R,3,H,W) and renders (R,K,3,H,W), got {tuple(ref.shape)} / "
                         f"{tuple(renders.shape)}")
    return int(ref.shape[0]), int(renders.shape[1]), int(ref.shape[2]), int(ref.shape[3])


def dists_forward_group(ref: torch.Tensor, renders: torch.Tensor, packed: torch.Tensor, prec,
                        ws: Workspace | None = None):
    """(S1, S2), each float32 (R*K, 1475), of K renders against ONE reference for R such groups: ref (R,3,H,W), renders
    (R,K,3,H,W), pair r * K + k = (ref[r], renders[r, k]).  The references go through the pyramid once per group
    (include/nqa.h, nqa_dists_forward_group).  Groups are independent: a batch whose workspace would exceed
    NQA_MAX_WORKSPACE_GB runs in equal slices over R."""
    p = prec_id(prec)
    dev = _need_cuda(ref, renders, packed)
    r, k, h, w = _group_dims(ref, renders)
    ref, renders = _f32c(ref), _f32c(renders)
    mr = _max_pairs(lambda n: lib().nqa_dists_group_workspace_bytes(n, k, h, w, p), r)
    mr = max(1, min(mr, 65535 // k))  # (pairs of one call: the library's limit)
    if mr < r:
        parts = [dists_forward_group(ref[i:i + mr], renders[i:i + mr], packed, prec, ws) for i in range(0, r, mr)]
        return torch.cat([q[0] for q in parts]), torch.cat([q[1] for q in parts])
    s1 = torch.empty((r * k, TOTAL_CHNS), dtype=torch.float32, device=dev)
    s2 = torch.empty((r * k, TOTAL_CHNS), dtype=torch.float32, device=dev)
    nbytes = lib().nqa_dists_group_workspace_bytes(r, k, h, w, p)
    buf = (ws or Workspace()).get(nbytes, dev)
    _call(dev, lib().nqa_dists_forward_group, ptr(ref), ptr(renders), r, k, h, w, ptr(packed), p, ptr(buf), buf.numel(),
          ptr(s1), ptr(s2), stream_ptr(dev))
    return s1, s2


def _group_maps(who: str, feat: torch.Tensor, r: int, k: int, p: int, nchw: bool):
    """(C, HW) of the n = r + r*k maps of a group statistics call; ValueError where feat does not fit."""
    if p not in PREC_DTYPE:
        raise ValueError(f"{who}: prec {p} is not one of the kernel-level modes")
    want = torch.float32 if nchw else PREC_DTYPE[p]
    if feat.dim() != 3 or r <= 0 or k <= 0 or feat.shape[0] != r + r * k or feat.numel() == 0 or feat.dtype != want \
            or not feat.is_contiguous():
        raise ValueError(f"{who}: expected contiguous {want} ({r + r * k}, "
                         f"{'C, HW' if nchw else 'HW, C'}), got {feat.dtype} {tuple(feat.shape)}")
    return (int(feat.shape[1]), int(feat.shape[2])) if nchw else (int(feat.shape[2]), int(feat.shape[1]))


def dists_group_stats(feat: torch.Tensor, r: int, k: int, prec, nchw: bool = False, s1: torch.Tensor | None = None,
                      s2: torch.Tensor | None = None, scratch: torch.Tensor | None = None):
    """(S1, S2), each float32 (r*k, C), of ONE map's group statistics as dists_forward_group launches them (include/nqa.h,
    nqa_dists_group_stats).  feat holds n = r + r*k maps, the r references first, render (i, j) at map r + i*k + j:
    nchw=True float32 planes (n, C, HW); else NHWC (n, HW, C) in prec's storage type.  s1, s2: as conv_pool_stats'
    outputs; scratch: a uint8 tensor of at least nqa_dists_group_stats_bytes to use instead of a new one."""
    p = prec_id(prec)
    dev = _need_cuda(feat)
    r, k = int(r), int(k)
    c, hw = _group_maps("dists_group_stats", feat, r, k, p, nchw)
    s1 = _out_or_empty(s1, (r * k, c), torch.float32, dev)
    s2 = _out_or_empty(s2, (r * k, c), torch.float32, dev)
    nbytes = lib().nqa_dists_group_stats_bytes(r, k, hw, c, p, int(nchw))
    if scratch is None:
        scratch = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
    else:
        _need_cuda(scratch)
        assert scratch.device == dev and scratch.dtype == torch.uint8 and scratch.numel() >= nbytes and scratch.is_contiguous()
    _call(dev, lib().nqa_dists_group_stats, ptr(feat), r, k, hw, c, p, int(nchw), ptr(scratch), scratch.numel(), ptr(s1),
          ptr(s2), stream_ptr(dev))
    return s1, s2


def dists_group_sums(feat: torch.Tensor, r: int, k: int, prec, nchw: bool = False, sums: torch.Tensor | None = None):
    """The five sums behind dists_group_stats, float64 (r*k, C, 5) = sum x, sum y, sum x^2, sum y^2, sum xy with x the
    pair's reference (include/nqa.h, nqa_dists_group_sums): the same launch, its partials folded.  feat, nchw: as
    dists_group_stats'; sums: as conv_pool_stats'."""
    p = prec_id(prec)
    dev = _need_cuda(feat)
    r, k = int(r), int(k)
    c, hw = _group_maps("dists_group_sums", feat, r, k, p, nchw)
    sums = _out_or_empty(sums, (r * k, c, 5), torch.float64, dev)
    nbytes = lib().nqa_dists_group_stats_bytes(r, k, hw, c, p, int(nchw))
    ws = torch.full((max(nbytes, 256),), 0xFF, dtype=torch.uint8, device=dev)  # (a block that never ran leaves NaN sums)
    _call(dev, lib().nqa_dists_group_sums, ptr(feat), r, k, hw, c, p, int(nchw), ptr(ws), nbytes, ptr(sums), stream_ptr(dev))
    return sums


def dists_group_stats_grid(r: int, k: int, hw: int, c: int, prec, nchw: bool = False) -> tuple:
    """(pixels per block, blocks per map, pixels a block takes side by side, the largest item count of a thread) of the
    group statistics launch for these arguments, from the launcher's own planning functions (no device is touched)."""
    g = (C.c_int * 4)()
    check(lib().nqa_dists_group_stats_grid(int(r), int(k), int(hw), int(c), prec_id(prec), int(nchw), g))
    return tuple(g)


def _feats_args(feats0: Sequence[torch.Tensor], feats1: Sequence[torch.Tensor]):
    """Two lists of six NCHW maps -> (device, float32 contiguous maps 0 and 1, B, the C / H / W / pointer arrays)."""
    if len(feats0) != 6 or len(feats1) != 6:
        raise ValueError("expected six feature maps per image")
    dev = _need_cuda(*feats0, *feats1)
    f0 = [_f32c(f) for f in feats0]
    f1 = [_f32c(f) for f in feats1]
    b = f0[0].shape[0]
    for a, c in zip(f0, f1):
        if a.shape != c.shape or a.dim() != 4 or a.shape[0] != b:
            raise ValueError("feature lists disagree in shape")
    cs = (C.c_int * 6)(*[f.shape[1] for f in f0])
    hs = (C.c_int * 6)(*[f.shape[2] for f in f0])
    wsz = (C.c_int * 6)(*[f.shape[3] for f in f0])
    p0 = (C.c_void_p * 6)(*[ptr(f) for f in f0])
    p1 = (C.c_void_p * 6)(*[ptr(f) for f in f1])
    return dev, f0, f1, b, cs, hs, wsz, p0, p1


def dists_stats_nchw(feats0: Sequence[torch.Tensor], feats1: Sequence[torch.Tensor], keep_scratch: bool = False,
                     s1: torch.Tensor | None = None, s2: torch.Tensor | None = None, scratch: torch.Tensor | None = None):
    """(S1, S2) from two lists of six float32 NCHW feature maps (forward_from_feats).

    keep_scratch=True returns (S1, S2, scratch): the forward's per-block fp64 sums, which dists_stats_nchw_backward
    reads (pass it unchanged, with the same maps).  s1, s2: as conv_pool_stats' outputs; scratch: a uint8 tensor of at
    least nqa_stats_scratch_bytes to use instead of a new one."""
    dev, f0, f1, b, cs, hs, wsz, p0, p1 = _feats_args(feats0, feats1)
    ctot = sum(f.shape[1] for f in f0)
    s1 = _out_or_empty(s1, (b, ctot), torch.float32, dev)
    s2 = _out_or_empty(s2, (b, ctot), torch.float32, dev)
    nbytes = lib().nqa_stats_scratch_bytes(b, cs, hs, wsz)
    if scratch is None:
        scratch = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
    else:
        _need_cuda(scratch)
        assert scratch.device == dev and scratch.dtype == torch.uint8 and scratch.numel() >= nbytes and scratch.is_contiguous()
    _call(dev, lib().nqa_dists_stats_nchw, p0, p1, b, cs, hs, wsz, ptr(scratch), scratch.numel(), ptr(s1), ptr(s2),
                                     stream_ptr(dev))
    if keep_scratch:
        return s1, s2, scratch
    return s1, s2


def dists_stats_nchw_backward(feats0: Sequence[torch.Tensor], feats1: Sequence[torch.Tensor], scratch: torch.Tensor,
                              g_s1: torch.Tensor, g_s2: torch.Tensor, need0: Sequence[bool], need1: Sequence[bool]):
    """(g0, g1): lists of six float32 NCHW gradients dL/dfeats0[k], dL/dfeats1[k] given dL/dS1, dL/dS2 (B, ctot), or
    None where need0[k] / need1[k] is False (nothing is computed for those).  scratch: what
    dists_stats_nchw(feats0, feats1, keep_scratch=True) returned, unchanged."""
    if len(need0) != 6 or len(need1) != 6:
        raise ValueError("expected six flags per list")
    dev, f0, f1, b, cs, hs, wsz, p0, p1 = _feats_args(feats0, feats1)
    _need_cuda(f0[0], scratch, g_s1, g_s2)
    ctot = sum(f.shape[1] for f in f0)
    g_s1, g_s2 = _f32c(g_s1), _f32c(g_s2)
    if tuple(g_s1.shape) != (b, ctot) or tuple(g_s2.shape) != (b, ctot):
        raise ValueError(f"expected gradients of shape {(b, ctot)}, got {tuple(g_s1.shape)} / {tuple(g_s2.shape)}")
    g0 = [torch.empty_like(f) if n else None for f, n in zip(f0, need0)]
    g1 = [torch.empty_like(f) if n else None for f, n in zip(f1, need1)]
    coef = torch.empty(max(lib().nqa_stats_backward_bytes(b, cs), 256), dtype=torch.uint8, device=dev)
    q0 = (C.c_void_p * 6)(*[None if g is None else ptr(g) for g in g0])
    q1 = (C.c_void_p * 6)(*[None if g is None else ptr(g) for g in g1])
    _call(dev, lib().nqa_dists_stats_nchw_backward, p0, p1, b, cs, hs, wsz, ptr(scratch), scratch.numel(), ptr(g_s1),
          ptr(g_s2), ptr(coef), coef.numel(), q0, q1, stream_ptr(dev))
    return g0, g1


def dists_score(s1: torch.Tensor, s2: torch.Tensor, alpha: torch.Tensor, beta: torch.Tensor) -> torch.Tensor:
    """score (B,) = 1 - sum(alpha*S1 + beta*S2)/(sum alpha + sum beta), fused kernel (no autograd)."""
    dev = _need_cuda(s1, s2, alpha, beta)
    s1, s2 = _f32c(s1), _f32c(s2)
    a, b_ = _f32c(alpha.detach().reshape(-1)), _f32c(beta.detach().reshape(-1))
    assert s1.shape == s2.shape and s1.shape[1] == TOTAL_CHNS == a.numel() == b_.numel()
    out = torch.empty((s1.shape[0],), dtype=torch.float32, device=dev)
    _call(dev, lib().nqa_dists_score, ptr(s1), ptr(s2), ptr(a), ptr(b_), s1.shape[0], ptr(out), stream_ptr(dev))
    return out


DEFAULT_CONV_VARIANT = 1  # the library's start-up value (include/nqa.h)


CONV_PLAIN_GRID, CONV_MIXED_GRID = 256, 512  # implicit-GEMM grid on maps with 1 <= W % 32 <= 16: never / always mixed


def set_conv_variant(v: int) -> None:
    check(lib().nqa_set_conv_variant(int(v)))


def mixed_grid_launches() -> int:
    """Mixed-grid conv launches (32-wide tiles + 16-wide edge tiles) of this thread since the last call."""
    n = lib().nqa_set_conv_variant(1024)
    if n < 0:
        check(n)
    return n


def dists_fused_taps(b: int, h: int, w: int, prec) -> tuple:
    """Taps (1..5) whose L2-pool and statistics nqa_dists_forward runs inside the stage-closing conv kernel for this
    shape and mode (the calling thread's conv variant bits 64 / 128 switch them off)."""
    f = (C.c_int * 6)()
    check(lib().nqa_dists_fused_taps(int(b), int(h), int(w), prec_id(prec), f))
    return tuple(k for k in range(6) if f[k])


def timing_enable(on: bool) -> None:
    check(lib().nqa_timing_enable(1 if on else 0))


def timing_collect():
    n = (C.c_int * len(_lib.K_NAMES))()
    ms = (C.c_double * len(_lib.K_NAMES))()
    check(lib().nqa_timing_collect(n, ms))
    return {name: (n[i], ms[i]) for i, name in enumerate(_lib.K_NAMES)}


CONV_WINDOW_GENERIC = 2048  # set_conv_variant bit: a 21-tap A-DISTS window runs on the generic window kernels too
# set_conv_variant bit: window=21 on window_moments / window_moments_backward / adists_ts_backward runs the generic
# window-moments kernels (csrc/nqa_window_moments_n.hip) too
CONV_MOMENTS_GENERIC = 4096
WINDOW_MIN, WINDOW_MAX = 3, 63  # the A-DISTS window sizes the library takes (include/nqa.h)


def check_window(window, who: str = "window") -> int:
    """The A-DISTS window size as an int; ValueError naming the range for anything but an integer in 3..63."""
    try:
        n = None if isinstance(window, (bool, str)) else operator.index(window)
    except TypeError:
        n = None
    if n is None or not WINDOW_MIN <= n <= WINDOW_MAX:
        raise ValueError(f"{who} must be an integer in {WINDOW_MIN}..{WINDOW_MAX} (the HIP window kernels' range), "
                         f"got {window!r}")
    return n


def adists_forward(x: torch.Tensor, y: torch.Tensor, packed: torch.Tensor, prec, ws: Workspace | None = None,
                   with_map: bool = False, window: int = 21):
    """D (B,) float32 of ADISTS.forward (ADISTS.py:147-191); the caller returns 1-D or 1-mean(D).

    with_map=True also returns the as_map=True distortion map (ADISTS.py:188-189,193) as (B,H,W).
    window: the module's window_size (3..63; 21 runs the specialised kernels)."""
    p, n = prec_id(prec), check_window(window)
    dev = _need_cuda(x, y, packed)
    x, y = _f32c(x), _f32c(y)
    if x.shape != y.shape or x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"expected two (B,3,H,W) tensors of equal shape, got {tuple(x.shape)} / {tuple(y.shape)}")
    b, _, h, w = x.shape
    mb = _max_pairs(lambda k: lib().nqa_adists_workspace_bytes_n(k, h, w, n, p), b)
    if mb < b:
        parts = [adists_forward(x[i:i + mb], y[i:i + mb], packed, prec, ws, with_map, n) for i in range(0, b, mb)]
        if with_map:
            return torch.cat([q[0] for q in parts]), torch.cat([q[1] for q in parts])
        return torch.cat(parts)
    d = torch.empty((b,), dtype=torch.float32, device=dev)
    nbytes = lib().nqa_adists_workspace_bytes_n(b, h, w, n, p)
    buf = (ws or Workspace()).get(nbytes, dev)
    if with_map:
        m = torch.empty((b, h, w), dtype=torch.float32, device=dev)
        _call(dev, lib().nqa_adists_forward_map_n, ptr(x), ptr(y), b, h, w, n, ptr(packed), p, ptr(buf), buf.numel(),
              ptr(d), ptr(m), stream_ptr(dev))
        return d, m
    _call(dev, lib().nqa_adists_forward_n, ptr(x), ptr(y), b, h, w, n, ptr(packed), p, ptr(buf), buf.numel(), ptr(d),
          stream_ptr(dev))
    return d


def adists_dists_forward(x: torch.Tensor, y: torch.Tensor, packed: torch.Tensor, prec, ws: Workspace | None = None,
                         with_map: bool = False, window: int = 21):
    """(D (B,), S1 (B,1475), S2 (B,1475)[, map (B,H,W)]) from ONE pyramid: adists_forward's D (and map), bit for bit, plus
    the similarities dists_forward computes for the same pairs in `prec`, folded from the sums A-DISTS forms anyway
    (include/nqa.h, nqa_adists_dists_forward).  window: as adists_forward's."""
    p, n = prec_id(prec), check_window(window)
    dev = _need_cuda(x, y, packed)
    x, y = _f32c(x), _f32c(y)
    if x.shape != y.shape or x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"expected two (B,3,H,W) tensors of equal shape, got {tuple(x.shape)} / {tuple(y.shape)}")
    b, _, h, w = x.shape
    mb = _max_pairs(lambda k: lib().nqa_adists_workspace_bytes_n(k, h, w, n, p), b)
    if mb < b:
        parts = [adists_dists_forward(x[i:i + mb], y[i:i + mb], packed, prec, ws, with_map, n) for i in range(0, b, mb)]
        return tuple(torch.cat([q[j] for q in parts]) for j in range(4 if with_map else 3))
    d = torch.empty((b,), dtype=torch.float32, device=dev)
    s1 = torch.empty((b, TOTAL_CHNS), dtype=torch.float32, device=dev)
    s2 = torch.empty((b, TOTAL_CHNS), dtype=torch.float32, device=dev)
    m = torch.empty((b, h, w), dtype=torch.float32, device=dev) if with_map else None
    nbytes = lib().nqa_adists_workspace_bytes_n(b, h, w, n, p)
    buf = (ws or Workspace()).get(nbytes, dev)
    _call(dev, lib().nqa_adists_dists_forward_n, ptr(x), ptr(y), b, h, w, n, ptr(packed), p, ptr(buf), buf.numel(),
          ptr(d), ptr(s1), ptr(s2), ptr(m) if with_map else None, stream_ptr(dev))
    return (d, s1, s2, m) if with_map else (d, s1, s2)


def adists_forward_group(ref: torch.Tensor, renders: torch.Tensor, packed: torch.Tensor, prec,
                         ws: Workspace | None = None, with_dists: bool = False, window: int = 21):
    """D (R*K,) float32 of K renders against ONE reference for R such groups: ref (R,3,H,W), renders (R,K,3,H,W), pair
    r * K + k = (ref[r], renders[r, k]) with x = the reference.  Everything A-DISTS takes from x alone runs once per
    reference (include/nqa.h, nqa_adists_forward_group).  with_dists=True returns (D, S1, S2), S1 / S2 (R*K,1475) the
    DISTS similarities of the same pairs from the same sums.  Groups are independent: a batch of more than 65 535 pairs,
    or one whose workspace would exceed NQA_MAX_WORKSPACE_GB, runs in equal slices over R.  window: as adists_forward's."""
    p, n = prec_id(prec), check_window(window)
    dev = _need_cuda(ref, renders, packed)
    r, k, h, w = _group_dims(ref, renders)
    ref, renders = _f32c(ref), _f32c(renders)
    mr = _max_pairs(lambda j: lib().nqa_adists_group_workspace_bytes_n(j, k, h, w, n, p), r)
    mr = max(1, min(mr, 65535 // k))  # (pairs of one call: the library's limit)
    if mr < r:
        parts = [adists_forward_group(ref[i:i + mr], renders[i:i + mr], packed, prec, ws, with_dists, n)
                 for i in range(0, r, mr)]
        if with_dists:
            return tuple(torch.cat([q[j] for q in parts]) for j in range(3))
        return torch.cat(parts)
    d = torch.empty((r * k,), dtype=torch.float32, device=dev)
    s1 = torch.empty((r * k, TOTAL_CHNS), dtype=torch.float32, device=dev) if with_dists else None
    s2 = torch.empty((r * k, TOTAL_CHNS), dtype=torch.float32, device=dev) if with_dists else None
    nbytes = lib().nqa_adists_group_workspace_bytes_n(r, k, h, w, n, p)
    buf = (ws or Workspace()).get(nbytes, dev)
    _call(dev, lib().nqa_adists_forward_group_n, ptr(ref), ptr(renders), r, k, h, w, n, ptr(packed), p, ptr(buf),
          buf.numel(), ptr(d), ptr(s1) if with_dists else None, ptr(s2) if with_dists else None, stream_ptr(dev))
    return (d, s1, s2) if with_dists else d


def adists_window_stage_group(fx: torch.Tensor, fy: torch.Tensor, q: torch.Tensor, wgt: torch.Tensor, prec,
                              strip: int = 0, window: int = 21, out=None):
    """One stage of the group window pass as adists_forward_group launches it (include/nqa.h,
    nqa_adists_window_stage_group): fx the R references' maps, fy the R*K renders' (pair r * K + k), q (8,R*K,C), wgt
    (R,C); maps as adists_window_stage takes them.  Returns gamma (R, mh, mw) and tw, sw (R*K, mh, mw); out = (gamma,
    tw, sw): caller-owned contiguous float32 maps of those shapes to write instead (tests place them between guards)."""
    p, strip, n = prec_id(prec), int(strip), check_window(window)
    dev = _need_cuda(fx, fy, q, wgt)
    r = int(wgt.shape[0]) if wgt.dim() == 2 else 0
    b, h, w, c, shape = _window_stage_dims(fx, fy, q, wgt, p, strip, "adists_window_stage_group", r, n)
    if out is None:
        gamma = torch.empty((r,) + shape[1:], dtype=torch.float32, device=dev)
        tw = torch.empty(shape, dtype=torch.float32, device=dev)
        sw = torch.empty(shape, dtype=torch.float32, device=dev)
    else:
        gamma, tw, sw = out
        _need_cuda(gamma, tw, sw)
        for t, sh in ((gamma, (r,) + shape[1:]), (tw, shape), (sw, shape)):
            if tuple(t.shape) != sh or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"adists_window_stage_group: outputs must be contiguous float32 {sh}, got {t.dtype} "
                                 f"{tuple(t.shape)}")
    _call(dev, lib().nqa_adists_window_stage_group_n, ptr(fx), ptr(fy), r, b // r, h, w, n, c, p, ptr(q), ptr(wgt), strip,
          ptr(gamma), ptr(tw), ptr(sw), stream_ptr(dev))
    return gamma, tw, sw


def adists_chain_group(gamma: Sequence[torch.Tensor], tw: Sequence[torch.Tensor], sw: Sequence[torch.Tensor], h: int,
                       w: int, ws: Workspace | None = None, window: int = 21):
    """The back part of adists_forward_group as it launches it (include/nqa.h, nqa_adists_chain_group): gamma six
    (R, mh, mw) maps, tw / sw six (R*K, mh, mw) maps for an h x w frame -> (ps_prod: six (R, mh, mw) maps, D (R*K,))."""
    _chain_lists(gamma=gamma, tw=tw, sw=sw)
    dev = _need_cuda(*gamma, *tw, *sw)
    h, w, n = int(h), int(w), check_window(window)
    r = int(gamma[0].shape[0]) if gamma[0].dim() == 3 else 0
    b, dims = _chain_dims(gamma, tw, sw, h, w, "adists_chain_group", r, n)
    ps = [torch.empty((r,) + dm, dtype=torch.float32, device=dev) for dm in dims]
    d = torch.empty((b,), dtype=torch.float32, device=dev)
    nbytes = lib().nqa_adists_chain_group_bytes_n(r, b // r, h, w, n)
    buf = (ws or Workspace()).get(nbytes, dev)
    arr = lambda ts: (C.c_void_p * 6)(*[ptr(t) for t in ts])
    _call(dev, lib().nqa_adists_chain_group_n, arr(gamma), arr(tw), arr(sw), r, b // r, h, w, n, ptr(buf), buf.numel(), arr(ps),
          ptr(d), stream_ptr(dev))
    return ps, d


def _window_stage_dims(fx: torch.Tensor, fy: torch.Tensor, q: torch.Tensor, wgt: torch.Tensor, p: int, strip: int,
                       who: str = "adists_window_stage", r: int | None = None, window: int = 21):
    """Every check of adists_window_stage (or, with the group count r, adists_window_stage_group) on its inputs;
    (B, H, W, C, shape of a per-pair output map).  C is q's: 3 means float32 NCHW planes, anything else NHWC taps in
    prec's storage type.  The x-side tensors (fx, wgt) have r rows, or B without r; the pair-side ones (fy, q) B."""
    if p not in PREC_DTYPE:
        raise ValueError(f"{who}: prec {p} is not one of the kernel-level modes")
    if q.dim() != 3 or q.shape[0] != 8 or q.shape[2] not in CHNS:
        raise ValueError(f"{who}: q must be (8, B, C) with C in {sorted(set(CHNS))}, got {tuple(q.shape)}")
    b, c = int(q.shape[1]), int(q.shape[2])
    nx = b if r is None else r
    if nx <= 0 or b % nx:
        raise ValueError(f"{who}: {b} pairs do not divide into {nx} groups")
    if fx.dim() != 4 or fy.dim() != 4 or fx.shape[1:] != fy.shape[1:] or fx.numel() == 0:
        raise ValueError(f"{who}: expected two non-empty 4-d taps of equal image shape, got {tuple(fx.shape)} / "
                         f"{tuple(fy.shape)}")
    if c == 3:
        h, w = int(fx.shape[2]), int(fx.shape[3])
        one, want = (3, h, w), torch.float32
    else:
        h, w = int(fx.shape[1]), int(fx.shape[2])
        one, want = (h, w, c), PREC_DTYPE[p]
    for name, t, sh, dt in (("fx", fx, (nx,) + one, want), ("fy", fy, (b,) + one, want),
                            ("q", q, (8, b, c), torch.float32), ("wgt", wgt, (nx, c), torch.float32)):
        if tuple(t.shape) != sh or t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"{who}: {name} must be contiguous {dt} {sh}, got {t.dtype} {tuple(t.shape)}"
                             f"{'' if t.is_contiguous() else ' (not contiguous)'}")
    windowed = h >= window and w >= window
    out = (b, h - window + 1, w - window + 1) if windowed else (b, 1, 1)
    if strip < 0 or (windowed and strip > out[1]):
        raise ValueError(f"{who}: strip {strip} outside [0, {out[1] if windowed else 0}]")
    return b, h, w, c, out


def adists_window_stage(fx: torch.Tensor, fy: torch.Tensor, q: torch.Tensor, wgt: torch.Tensor, prec, strip: int = 0,
                        window: int = 21):
    """One stage of the A-DISTS heavy pass as adists_forward launches it (include/nqa.h, nqa_adists_window_stage):
    (gamma, tw, sw), each (B, H-20, W-20) float32, or (B, 1, 1) from the global branch when H or W is under 21.
    q (8,B,C) and wgt (B,C) float32; fx, fy (B,3,H,W) float32 planes for C == 3, else (B,H,W,C) NHWC taps in prec's
    storage type.  strip: see the header (0 = the launcher's choice).  window: 3..63 in place of 21 (the generic
    kernels; nqa_adists_window_stage_n)."""
    n = check_window(window)
    _need_cuda(fx, fy, q, wgt)
    out_shape = _window_stage_dims(fx, fy, q, wgt, prec_id(prec), int(strip), window=n)[4]
    out = torch.empty((3,) + out_shape, dtype=torch.float32, device=fx.device)
    adists_window_stage_into(fx, fy, q, wgt, prec, strip, out[0], out[1], out[2], n)
    return out[0], out[1], out[2]


def adists_window_stage_into(fx, fy, q, wgt, prec, strip, gamma, tw, sw, window: int = 21) -> None:
    """adists_window_stage into caller-owned contiguous float32 maps of the shape it would return (tests place them
    between guard regions).  Every check of adists_window_stage applies."""
    p, strip, n = prec_id(prec), int(strip), check_window(window)
    dev = _need_cuda(fx, fy, q, wgt, gamma, tw, sw)
    b, h, w, c, shape = _window_stage_dims(fx, fy, q, wgt, p, strip, window=n)
    for t in (gamma, tw, sw):
        if tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"adists_window_stage: outputs must be contiguous float32 {shape}, got {t.dtype} "
                             f"{tuple(t.shape)}")
    _call(dev, lib().nqa_adists_window_stage_n, ptr(fx), ptr(fy), b, h, w, n, c, p, ptr(q), ptr(wgt), strip, ptr(gamma),
          ptr(tw), ptr(sw), stream_ptr(dev))


def adists_window_grid(b: int, h: int, w: int, c: int, prec, strip: int = 0) -> tuple:
    """(column groups, row strips, strip height) of the LDS window kernel for these arguments under the calling thread's
    conv variant, from the launcher's own function; zeros where another kernel would run."""
    g = (C.c_int * 3)()
    check(lib().nqa_adists_window_grid(int(b), int(h), int(w), int(c), prec_id(prec), int(strip), g))
    return tuple(g)


def adists_chain_dims(h: int, w: int, window: int = 21):
    """([(mh, mw)] of the six stages' maps for an h x w frame, the number of windowed stages), from the library's own plan
    (include/nqa.h, nqa_adists_chain_dims_n)."""
    mh, mw = (C.c_int * 6)(), (C.c_int * 6)()
    n = lib().nqa_adists_chain_dims_n(int(h), int(w), check_window(window), mh, mw)
    if n < 0:
        check(n)
    return list(zip(mh, mw)), n


def _chain_lists(**lists) -> None:
    for name, ts in lists.items():
        if not isinstance(ts, (list, tuple)) or len(ts) != 6 or not all(torch.is_tensor(t) for t in ts):
            raise ValueError(f"adists_chain: {name} must be a list of six tensors, one per stage")


def _chain_dims(gamma, tw, sw, h: int, w: int, who: str = "adists_chain", r: int | None = None, window: int = 21):
    """Every check of adists_chain (or, with the group count r, adists_chain_group) on its inputs but their device;
    (B, [(mh, mw)] per stage).  The x-side maps (gamma) have r rows, or B without r; the pair-side ones (tw, sw) B."""
    _chain_lists(gamma=gamma, tw=tw, sw=sw)
    if gamma[0].dim() != 3 or tw[0].dim() != 3 or gamma[0].shape[0] == 0:
        raise ValueError(f"{who}: maps must be (B, mh, mw), got {tuple(gamma[0].shape)} / {tuple(tw[0].shape)}")
    if int(h) <= 0 or int(w) <= 0:
        raise ValueError(f"{who}: bad frame size {h} x {w}")
    b = int(gamma[0].shape[0]) if r is None else int(tw[0].shape[0])
    nx = b if r is None else r
    if nx <= 0 or b % nx:
        raise ValueError(f"{who}: {b} pairs do not divide into {nx} groups")
    dims, _ = adists_chain_dims(h, w, window)
    for name, ts, n in (("gamma", gamma, nx), ("tw", tw, b), ("sw", sw, b)):
        for k, t in enumerate(ts):
            sh = (n,) + dims[k]
            if tuple(t.shape) != sh or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"{who}: {name}[{k}] must be contiguous float32 {sh}, got {t.dtype} "
                                 f"{tuple(t.shape)}{'' if t.is_contiguous() else ' (not contiguous)'}")
    return b, dims


def adists_chain(gamma: Sequence[torch.Tensor], tw: Sequence[torch.Tensor], sw: Sequence[torch.Tensor], h: int, w: int,
                 with_map: bool = True, ws: Workspace | None = None, window: int = 21):
    """The back part of adists_forward as it launches it (include/nqa.h, nqa_adists_chain): from the six stages' gamma /
    tw / sw maps, each (B, mh, mw) float32 for an h x w frame (adists_chain_dims), to (ps_prod: six (B, mh, mw) maps,
    D (B,), map (B,h,w) or None)."""
    _chain_lists(gamma=gamma, tw=tw, sw=sw)
    dev = _need_cuda(*gamma, *tw, *sw)
    b, dims = _chain_dims(gamma, tw, sw, h, w, window=check_window(window))
    ps = [torch.empty((b,) + d, dtype=torch.float32, device=dev) for d in dims]
    d = torch.empty((b,), dtype=torch.float32, device=dev)
    m = torch.empty((b, int(h), int(w)), dtype=torch.float32, device=dev) if with_map else None
    adists_chain_into(gamma, tw, sw, h, w, ps, d, m, ws, window)
    return ps, d, m


def adists_chain_into(gamma, tw, sw, h: int, w: int, ps_prod, d, map_out=None, ws: Workspace | None = None,
                      window: int = 21) -> None:
    """adists_chain into caller-owned contiguous float32 outputs of the shapes it would return (tests place them between
    guard regions); map_out None: no map.  Every check of adists_chain applies."""
    _chain_lists(gamma=gamma, tw=tw, sw=sw, ps_prod=ps_prod)
    outs = list(ps_prod) + [d] + ([] if map_out is None else [map_out])
    if not all(torch.is_tensor(t) for t in outs):
        raise ValueError("adists_chain: d (and map_out, if given) must be tensors")
    dev = _need_cuda(*gamma, *tw, *sw, *outs)
    n = check_window(window)
    b, dims = _chain_dims(gamma, tw, sw, h, w, window=n)
    h, w = int(h), int(w)
    want = [(b,) + dm for dm in dims] + [(b,)] + ([] if map_out is None else [(b, h, w)])
    for t, sh in zip(outs, want):
        if tuple(t.shape) != sh or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"adists_chain: outputs must be contiguous float32, here {sh}, got {t.dtype} {tuple(t.shape)}")
    nbytes = lib().nqa_adists_chain_bytes_n(b, h, w, n)
    buf = (ws or Workspace()).get(nbytes, dev)
    arr = lambda ts: (C.c_void_p * 6)(*[ptr(t) for t in ts])
    _call(dev, lib().nqa_adists_chain_n, arr(gamma), arr(tw), arr(sw), b, h, w, n, ptr(buf), buf.numel(), arr(ps_prod), ptr(d),
          None if map_out is None else ptr(map_out), stream_ptr(dev))


def _front_dims(x: torch.Tensor, y: torch.Tensor, taps, p: int):
    """Every check of adists_front on its inputs but their device; (B, [H_k], [W_k]) for k = 0..5."""
    if p not in PREC_DTYPE:
        raise ValueError(f"adists_front: prec {p} is not one of the kernel-level modes")
    if not isinstance(taps, (list, tuple)) or len(taps) != 5 or not all(torch.is_tensor(t) for t in taps):
        raise ValueError("adists_front: taps must be a list of five tensors")
    if not (torch.is_tensor(x) and torch.is_tensor(y)) or x.dim() != 4 or x.shape != y.shape or x.shape[1] != 3 \
            or x.numel() == 0:
        raise ValueError("adists_front: expected two non-empty (B,3,H,W) images of equal shape")
    b = int(x.shape[0])
    hs, ws = [int(x.shape[2])], [int(x.shape[3])]
    for name, t in (("x", x), ("y", y)):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"adists_front: {name} must be contiguous float32, got {t.dtype}"
                             f"{'' if t.is_contiguous() else ' (not contiguous)'}")
    for k, t in enumerate(taps):
        if t.dim() != 4 or t.shape[0] != 2 * b or t.shape[3] != CHNS[k + 1] or t.numel() == 0 \
                or t.dtype != PREC_DTYPE[p] or not t.is_contiguous():
            raise ValueError(f"adists_front: tap {k + 1} must be contiguous {PREC_DTYPE[p]} ({2 * b}, H, W, {CHNS[k + 1]}), "
                             f"got {t.dtype} {tuple(t.shape)}{'' if t.is_contiguous() else ' (not contiguous)'}")
        hs.append(int(t.shape[1]))
        ws.append(int(t.shape[2]))
    return b, hs, ws


def adists_front(x: torch.Tensor, y: torch.Tensor, taps: Sequence[torch.Tensor], prec, ws: Workspace | None = None):
    """The front part of adists_forward as it launches it (include/nqa.h, nqa_adists_front): from the images (B,3,H,W)
    float32 and the five tapped maps, each (2B, H_k, W_k, C_k) NHWC in prec's storage type with the x images first, to
    (q (8,B,1475), wgt (B,1475)) float32.  q[2] holds the folded per-channel entropy hsum.  The taps' sizes are free."""
    b = _front_dims(x, y, taps, prec_id(prec))[0]
    dev = _need_cuda(x, y, *taps)
    q = torch.empty((8, b, TOTAL_CHNS), dtype=torch.float32, device=dev)
    wgt = torch.empty((b, TOTAL_CHNS), dtype=torch.float32, device=dev)
    adists_front_into(x, y, taps, prec, q, wgt, ws)
    return q, wgt


def adists_front_into(x, y, taps, prec, q, wgt, ws: Workspace | None = None) -> None:
    """adists_front into caller-owned contiguous float32 outputs of the shapes it would return (tests place them between
    guard regions).  Every check of adists_front applies."""
    p = prec_id(prec)
    b, hs, wss = _front_dims(x, y, taps, p)
    if not (torch.is_tensor(q) and torch.is_tensor(wgt)):
        raise ValueError("adists_front: q and wgt must be tensors")
    for name, t, sh in (("q", q, (8, b, TOTAL_CHNS)), ("wgt", wgt, (b, TOTAL_CHNS))):
        if tuple(t.shape) != sh or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"adists_front: {name} must be contiguous float32 {sh}, got {t.dtype} {tuple(t.shape)}")
    dev = _need_cuda(x, y, *taps, q, wgt)
    hk, wk = (C.c_int * 6)(*hs), (C.c_int * 6)(*wss)
    nbytes = lib().nqa_adists_front_bytes(b, hk, wk, p)
    if nbytes == 0:
        raise _lib.NqaError(f"libnqa_hip: {lib().nqa_last_error().decode()}")
    buf = (ws or Workspace()).get(nbytes, dev)
    tp = (C.c_void_p * 5)(*[ptr(t) for t in taps])
    _call(dev, lib().nqa_adists_front, ptr(x), ptr(y), tp, b, hk, wk, p, ptr(buf), buf.numel(), ptr(q), ptr(wgt),
          stream_ptr(dev))


def adists_front_grid(b: int, dims: Sequence, prec) -> list:
    """[(statistics blocks, TR, TC, entropy blocks)] for k = 0..5 of adists_front on B = b pairs with the image and the
    five taps of dims[k] = (H_k, W_k), from the library's own planning functions; TR, TC are the pool pass' tile (taps
    1..4, zeros elsewhere)."""
    if len(dims) != 6:
        raise ValueError("adists_front_grid: dims must hold six (H, W) pairs")
    hk, wk = (C.c_int * 6)(*[int(d[0]) for d in dims]), (C.c_int * 6)(*[int(d[1]) for d in dims])
    g = (C.c_int * 24)()
    check(lib().nqa_adists_front_grid(int(b), hk, wk, prec_id(prec), g))
    return [tuple(g[4 * k:4 * k + 4]) for k in range(6)]


# ---- input preparation ---------------------------------------------------
def u8hwc_to_f32nchw(frames: torch.Tensor, pil_roundtrip: bool = False) -> torch.Tensor:
    """ToTensor on the device: uint8 (n,H,W,3) -> float32 (n,3,H,W) / 255 (prep.py:89, data.py:80)."""
    dev = _need_cuda(frames)
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
        raise ValueError(f"expected uint8 (n,H,W,3), got {frames.dtype} {tuple(frames.shape)}")
    frames = frames.contiguous()
    n, h, w, _ = frames.shape
    out = torch.empty((n, 3, h, w), dtype=torch.float32, device=dev)
    _call(dev, lib().nqa_u8hwc_to_f32nchw, ptr(frames), n, h, w, int(pil_roundtrip), ptr(out), stream_ptr(dev))
    return out


def resize_bilinear_f32(x: torch.Tensor, size) -> torch.Tensor:
    """F.interpolate(x, size=size, mode='bilinear', align_corners=False) for float32 (n,C,H,W)."""
    dev = _need_cuda(x)
    x = _f32c(x)
    if x.dim() != 4:
        raise ValueError(f"expected (n,C,H,W), got {tuple(x.shape)}")
    ho, wo = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
    n, c, h, w = x.shape
    out = torch.empty((n, c, ho, wo), dtype=torch.float32, device=dev)
    _call(dev, lib().nqa_resize_bilinear_f32, ptr(x), n * c, h, w, ho, wo, ptr(out), stream_ptr(dev))
    return out


def u8_resize_bilinear_f32(frames: torch.Tensor, size) -> torch.Tensor:
    """ToTensor + F.interpolate(bilinear, align_corners=False) fused: uint8 (n,H,W,3) -> float32 (n,3,h,w)."""
    dev = _need_cuda(frames)
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
        raise ValueError(f"expected uint8 (n,H,W,3), got {frames.dtype} {tuple(frames.shape)}")
    frames = frames.contiguous()
    ho, wo = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
    n, h, w, _ = frames.shape
    out = torch.empty((n, 3, ho, wo), dtype=torch.float32, device=dev)
    _call(dev, lib().nqa_u8_resize_bilinear_f32, ptr(frames), n, h, w, ho, wo, ptr(out), stream_ptr(dev))
    return out


def resize_pil_bilinear_u8(frames: torch.Tensor, size, ws: Workspace | None = None) -> torch.Tensor:
    """PIL Image.resize((W,H), BILINEAR) on uint8 (n,H,W,3) frames, bit-exact; size = (Hout, Wout)."""
    dev = _need_cuda(frames)
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
        raise ValueError(f"expected uint8 (n,H,W,3), got {frames.dtype} {tuple(frames.shape)}")
    frames = frames.contiguous()
    n, h, w, _ = frames.shape
    ho, wo = int(size[0]), int(size[1])
    out = torch.empty((n, ho, wo, 3), dtype=torch.uint8, device=dev)
    nbytes = lib().nqa_resize_pil_workspace_bytes(n, h, w, ho, wo)
    buf = (ws or Workspace()).get(nbytes, dev)
    _call(dev, lib().nqa_resize_pil_bilinear_u8, ptr(frames), n, h, w, ho, wo, ptr(buf), buf.numel(), ptr(out),
                                           stream_ptr(dev))
    return out


# ---- score-map targets (nerf_nr_qa_prep_4.py:71-133) ---------------------------------------------
def _score_maps_dims(maps: torch.Tensor):
    """Every check of score_maps on its input but its device; (F, K, H, W)."""
    if not torch.is_tensor(maps) or maps.dim() != 4 or maps.numel() == 0:
        raise ValueError(f"score_maps: maps must be a non-empty (F, K, H, W) tensor, got {tuple(getattr(maps, 'shape', ()))}")
    if maps.dtype != torch.float32 or not maps.is_contiguous():
        raise ValueError(f"score_maps: maps must be contiguous float32, got {maps.dtype}"
                         f"{'' if maps.is_contiguous() else ' (not contiguous)'}")
    return tuple(int(s) for s in maps.shape)


def score_maps(maps: torch.Tensor, ws: Workspace | None = None):
    """The arithmetic the reference's dataset prep runs on the CPU after as_map=True (include/nqa.h, nqa_score_maps):
    from maps (F, K, H, W) float32 -- frame f's K distortion maps, one per render -- to (rgb (F, K, H, W, 3) uint8 with
    the channels (mean, map k, std), logs (F, 2K + 4) float64: K x log_max, K x log_min, std_max, std_min, mean_max,
    mean_min)."""
    f, k, h, w = _score_maps_dims(maps)
    dev = _need_cuda(maps)
    rgb = torch.empty((f, k, h, w, 3), dtype=torch.uint8, device=dev)
    logs = torch.empty((f, 2 * k + 4), dtype=torch.float64, device=dev)
    score_maps_into(maps, rgb, logs, ws)
    return rgb, logs


def score_maps_into(maps: torch.Tensor, rgb: torch.Tensor, logs: torch.Tensor, ws: Workspace | None = None) -> None:
    """score_maps into caller-owned contiguous outputs of the shapes and types it would return (tests place them between
    guard regions).  Every check of score_maps applies."""
    f, k, h, w = _score_maps_dims(maps)
    if not (torch.is_tensor(rgb) and torch.is_tensor(logs)):
        raise ValueError("score_maps: rgb and logs must be tensors")
    for name, t, sh, dt in (("rgb", rgb, (f, k, h, w, 3), torch.uint8), ("logs", logs, (f, 2 * k + 4), torch.float64)):
        if tuple(t.shape) != sh or t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"score_maps: {name} must be contiguous {dt} {sh}, got {t.dtype} {tuple(t.shape)}")
    dev = _need_cuda(maps, rgb, logs)
    nbytes = lib().nqa_score_maps_workspace_bytes(f, k, h, w)
    if nbytes == 0:
        raise _lib.NqaError(f"libnqa_hip: {lib().nqa_last_error().decode()}")
    buf = (ws or Workspace()).get(nbytes, dev)
    _call(dev, lib().nqa_score_maps, ptr(maps), f, k, h, w, ptr(buf), buf.numel(), ptr(rgb), ptr(logs), stream_ptr(dev))


# ---- split16 (NQA_PREC_F32S activation format between conv layers; tests and tools only) ----------
def split16_encode(a: torch.Tensor) -> torch.Tensor:
    """float32 NHWC (..., C) -> split16 bytes viewed as float32 of the same shape (4 bytes per element)."""
    dev = _need_cuda(a)
    a = _f32c(a)
    c = a.shape[-1]
    out = torch.empty_like(a)
    _call(dev, lib().nqa_split16_encode, ptr(a), a.numel() // c, c, ptr(out), stream_ptr(dev))
    return out


def split16_decode(a: torch.Tensor) -> torch.Tensor:
    dev = _need_cuda(a)
    assert a.dtype == torch.float32 and a.is_contiguous()
    c = a.shape[-1]
    out = torch.empty_like(a)
    _call(dev, lib().nqa_split16_decode, ptr(a), a.numel() // c, c, ptr(out), stream_ptr(dev))
    return out


# ---- backward pass of the DISTS pyramid (require_grad=True; include/nqa.h, nqa_backward.hip) -----------------------
def _pack_conv(fmt: str, w) -> torch.Tensor:
    """One 3x3 layer (float32 OIHW), zero bias -> CPU uint8 blob by the library's packer of row format `fmt`."""
    w = np.ascontiguousarray(w.detach().cpu().numpy() if torch.is_tensor(w) else w, dtype=np.float32)
    cout, cin = int(w.shape[0]), int(w.shape[1])
    assert w.shape[2:] == (3, 3)
    nbytes = getattr(lib(), f"nqa_packed_conv_{fmt}_bytes")(cout, cin)
    if not nbytes:
        raise ValueError(f"pack_conv_{fmt}: unsupported layer shape {w.shape}")
    blob = torch.empty(nbytes, dtype=torch.uint8)
    check(getattr(lib(), f"nqa_pack_conv_{fmt}")(w.ctypes.data, cout, cin, blob.data_ptr()))
    return blob


def pack_conv_split(w) -> torch.Tensor:
    """One 3x3 layer (float32 OIHW, cout % 64 == 0, cin % 16 == 0) in the f32s row format, zero bias -> CPU uint8 blob."""
    return _pack_conv("split", w)


def conv3x3_split(inp: torch.Tensor, blob: torch.Tensor, cout: int, relu: bool = False) -> torch.Tensor:
    """split16 NHWC (n,H,W,cin) -> float32 NHWC (n,H,W,cout) through a layer packed by pack_conv_split."""
    dev = _need_cuda(inp, blob)
    assert inp.dtype == torch.float32 and inp.is_contiguous()
    n, h, w, cin = inp.shape
    out = torch.empty((n, h, w, cout), dtype=torch.float32, device=dev)
    _call(dev, lib().nqa_conv3x3_split, ptr(inp), n, h, w, cin, cout, ptr(blob), int(relu), ptr(out), stream_ptr(dev))
    return out


def relu_mask_split16(g: torch.Tensor, act: torch.Tensor, act_is_split16: bool) -> torch.Tensor:
    """g * (act > 0) as split16 records (float32-typed tensor of g's shape); act: float map or split16 records."""
    dev = _need_cuda(g, act)
    g = _f32c(g)
    assert act.dtype == torch.float32 and act.is_contiguous() and act.shape == g.shape
    c = g.shape[-1]
    out = torch.empty_like(g)
    _call(dev, lib().nqa_relu_mask_split16, ptr(g), ptr(act), int(act_is_split16), g.numel() // c, c, ptr(out),
          stream_ptr(dev))
    return out


def l2pool_backward(tap: torch.Tensor, pooled_split16: torch.Tensor, g_pooled: torch.Tensor, g_tap: torch.Tensor) -> None:
    """g_tap += d(L2-pool)/d(tap) applied to g_pooled; tap, g_tap float (n,H,W,C); pooled_split16, g_pooled (n,Ho,Wo,C).
    The kernel forms the pooled value from `tap` in float; `pooled_split16` is only checked for its shape."""
    dev = _need_cuda(tap, pooled_split16, g_pooled, g_tap)
    n, h, w, c = tap.shape
    assert g_tap.shape == tap.shape and g_tap.is_contiguous() and tap.is_contiguous() and tap.dtype == torch.float32
    assert g_pooled.shape == pooled_split16.shape == (n, (h + 1) // 2, (w + 1) // 2, c)
    _call(dev, lib().nqa_l2pool_backward, ptr(tap), ptr(pooled_split16), ptr(_f32c(g_pooled)), n, h, w, c, ptr(g_tap),
          stream_ptr(dev))


def conv1_1_backward(gm: torch.Tensor, w0: torch.Tensor) -> torch.Tensor:
    """g * (relu1_1 > 0), float NHWC (n,H,W,64) -> gradient of the raw image, float NCHW (n,3,H,W); w0: conv1_1's OIHW weights."""
    dev = _need_cuda(gm, w0)
    gm, w0 = _f32c(gm), _f32c(w0)
    n, h, w, c = gm.shape
    assert c == 64 and tuple(w0.shape) == (64, 3, 3, 3)
    out = torch.empty((n, 3, h, w), dtype=torch.float32, device=dev)
    _call(dev, lib().nqa_conv1_1_backward, ptr(gm), ptr(w0), n, h, w, ptr(out), stream_ptr(dev))
    return out


# ---- DISTS as a loss: the same chain without a device -> host read (include/nqa.h, nqa_loss_backward.hip) ----------
def _tap_grad_maps(tx: torch.Tensor, need_x: bool, need_y: bool, out_x: torch.Tensor | None, out_y: torch.Tensor | None):
    """(gx, gy) the statistics-gradient wrappers write: per side the caller's out_x / out_y, else a new map like the
    tap tx, None where it is not needed; contiguous float maps of the tap's shape on its device."""
    gx = (torch.empty_like(tx) if out_x is None else out_x) if need_x else None
    gy = (torch.empty_like(tx) if out_y is None else out_y) if need_y else None
    for g in (gx, gy):
        assert g is None or (g.shape == tx.shape and g.dtype == torch.float32 and g.is_contiguous() and g.device == tx.device)
    return gx, gy


def dists_stats_nhwc_backward(tx: torch.Tensor, ty: torch.Tensor, g_s1: torch.Tensor, g_s2: torch.Tensor, col: int,
                              need_x: bool = True, need_y: bool = True, out_x: torch.Tensor | None = None,
                              out_y: torch.Tensor | None = None):
    """(gx, gy): d(sum g_s1 S1 + g_s2 S2)/d(tx), /d(ty) for one pair of float NHWC taps (B,H,W,C), each times its tap's
    ReLU mask (t > 0); None where need_x / need_y is False (nothing is computed for it).  g_s1, g_s2: float (B, ctot)
    upstream gradients, the tap's C columns starting at `col`.  out_x / out_y: where to write (tx's shape), else new."""
    dev = _need_cuda(tx, ty, g_s1, g_s2)
    assert tx.dtype == ty.dtype == torch.float32 and tx.is_contiguous() and ty.is_contiguous() and tx.shape == ty.shape
    assert g_s1.dtype == g_s2.dtype == torch.float32 and g_s1.is_contiguous() and g_s2.is_contiguous()
    b, h, w, c = tx.shape
    if g_s1.shape != g_s2.shape or g_s1.dim() != 2 or g_s1.shape[0] != b or col < 0 or col + c > g_s1.shape[1]:
        raise ValueError(f"expected gradients of shape ({b}, >= {col + c}), got {tuple(g_s1.shape)} / {tuple(g_s2.shape)}")
    gx, gy = _tap_grad_maps(tx, need_x, need_y, out_x, out_y)
    if gx is None and gy is None:
        return None, None
    nbytes = lib().nqa_dists_stats_nhwc_backward_bytes(b, h, w, c)
    if not nbytes:
        raise _lib.NqaError(f"dists_stats_nhwc_backward: unsupported tap shape {tuple(tx.shape)}")
    buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _call(dev, lib().nqa_dists_stats_nhwc_backward, ptr(tx), ptr(ty), b, h, w, c, ptr(g_s1) + 4 * col, ptr(g_s2) + 4 * col,
          g_s1.shape[1], ptr(buf), buf.numel(), None if gx is None else ptr(gx), None if gy is None else ptr(gy),
          stream_ptr(dev))
    return gx, gy


def _tap_pair(who: str, tx: torch.Tensor, ty: torch.Tensor, s_a: torch.Tensor, s_b: torch.Tensor, col: int):
    """The checks dists_stats_target and dists_stats_nhwc_backward_from share: a pair of contiguous float NHWC taps and two
    contiguous float (B, ctot) rows of per-channel values that hold the tap's C columns from `col`."""
    dev = _need_cuda(tx, ty, s_a, s_b)
    assert tx.dtype == ty.dtype == torch.float32 and tx.is_contiguous() and ty.is_contiguous() and tx.shape == ty.shape
    assert s_a.dtype == s_b.dtype == torch.float32 and s_a.is_contiguous() and s_b.is_contiguous()
    b, c = tx.shape[0], tx.shape[3]
    if s_a.shape != s_b.shape or s_a.dim() != 2 or s_a.shape[0] != b or col < 0 or col + c > s_a.shape[1]:
        raise ValueError(f"{who}: expected rows of shape ({b}, >= {col + c}), got {tuple(s_a.shape)} / {tuple(s_b.shape)}")
    return dev


def dists_stats_target(tx: torch.Tensor, ty: torch.Tensor, s1: torch.Tensor, s2: torch.Tensor, col: int) -> torch.Tensor:
    """S1 / S2 of one pair of float NHWC taps (B,H,W,C) into columns col .. col + C of s1, s2 (float (B, ctot)); returns the
    sums' per-block fp64 partials (a uint8 tensor), which dists_stats_nhwc_backward_from starts from."""
    dev = _tap_pair("dists_stats_target", tx, ty, s1, s2, col)
    b, h, w, c = tx.shape
    nbytes = lib().nqa_dists_stats_target_bytes(b, h, w, c)
    if not nbytes:
        raise _lib.NqaError(f"dists_stats_target: unsupported tap shape {tuple(tx.shape)}")
    part = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _call(dev, lib().nqa_dists_stats_target, ptr(tx), ptr(ty), b, h, w, c, ptr(part), part.numel(), ptr(s1) + 4 * col,
          ptr(s2) + 4 * col, s1.shape[1], stream_ptr(dev))
    return part


def dists_stats_nhwc_backward_from(tx: torch.Tensor, ty: torch.Tensor, part: torch.Tensor, g_s1: torch.Tensor,
                                   g_s2: torch.Tensor, col: int, need_x: bool = True, need_y: bool = True,
                                   out_x: torch.Tensor | None = None, out_y: torch.Tensor | None = None):
    """dists_stats_nhwc_backward without its sums pass: `part` is what dists_stats_target returned for the same taps.  The
    result is that call's bit for bit."""
    dev = _tap_pair("dists_stats_nhwc_backward_from", tx, ty, g_s1, g_s2, col)
    assert part.dtype == torch.uint8 and part.is_contiguous() and part.device == dev
    b, h, w, c = tx.shape
    gx, gy = _tap_grad_maps(tx, need_x, need_y, out_x, out_y)
    if gx is None and gy is None:
        return None, None
    nbytes = lib().nqa_dists_stats_nhwc_backward_from_bytes(b, c)
    if not nbytes:
        raise _lib.NqaError(f"dists_stats_nhwc_backward_from: unsupported tap shape {tuple(tx.shape)}")
    coef = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _call(dev, lib().nqa_dists_stats_nhwc_backward_from, ptr(tx), ptr(ty), b, h, w, c, ptr(part), part.numel(),
          ptr(g_s1) + 4 * col, ptr(g_s2) + 4 * col, g_s1.shape[1], ptr(coef), coef.numel(),
          None if gx is None else ptr(gx), None if gy is None else ptr(gy), stream_ptr(dev))
    return gx, gy


def dists_stats_nhwc_grad_y_add(tx: torch.Tensor, ty: torch.Tensor, part: torch.Tensor, g_s1: torch.Tensor,
                                g_s2: torch.Tensor, col: int, gy: torch.Tensor) -> torch.Tensor:
    """gy += the gy of dists_stats_nhwc_backward_from(tx, ty, part, g_s1, g_s2, col, need_x=False), in place: that call
    followed by one float add, bit for bit, without the map and the pass of its own.  gy: contiguous float, ty's shape
    (another metric's gradient of the same tap).  Returns gy."""
    dev = _tap_pair("dists_stats_nhwc_grad_y_add", tx, ty, g_s1, g_s2, col)
    assert part.dtype == torch.uint8 and part.is_contiguous() and part.device == dev
    _tap_grad_maps(tx, False, True, None, gy)
    b, h, w, c = tx.shape
    nbytes = lib().nqa_dists_stats_nhwc_backward_from_bytes(b, c)
    if not nbytes:
        raise _lib.NqaError(f"dists_stats_nhwc_grad_y_add: unsupported tap shape {tuple(tx.shape)}")
    coef = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _call(dev, lib().nqa_dists_stats_nhwc_grad_y_add, ptr(tx), ptr(ty), b, h, w, c, ptr(part), part.numel(),
          ptr(g_s1) + 4 * col, ptr(g_s2) + 4 * col, g_s1.shape[1], ptr(coef), coef.numel(), ptr(gy), stream_ptr(dev))
    return gy


# ---- the prepared-target loss step as two library calls (include/nqa.h, "the prepared-target loss step"; nqa_loss_step.hip) ----
GRAD_PREC_ID = {"f32s": _lib.PREC_F32S, "f16": _lib.PREC_F16}  # the rungs of the gradient chain as the step calls name them


def dists_target_step_bytes(b: int, h: int, w: int, grad_precision: str = "f32s") -> int:
    """Bytes of the state block of one step for b pairs of h x w frames on the rung grad_precision; 0 for a shape the
    step does not take (no device is touched)."""
    return int(lib().nqa_dists_target_step_bytes(int(b), int(h), int(w), GRAD_PREC_ID[grad_precision]))


def _step_args(who: str, x: torch.Tensor, x_taps: Sequence[torch.Tensor], y: torch.Tensor, state: torch.Tensor):
    dev = _need_cuda(x, y, state, *x_taps)
    assert len(x_taps) == 5 and all(t.dtype == torch.float32 and t.is_contiguous() for t in x_taps), who
    assert x.dtype == y.dtype == torch.float32 and x.is_contiguous() and y.is_contiguous() and x.shape == y.shape, who
    assert state.dtype == torch.uint8 and state.is_contiguous(), who
    b, _, h, w = x.shape
    return dev, b, h, w, (C.c_void_p * 5)(*[ptr(t) for t in x_taps])


def dists_target_step_forward(x: torch.Tensor, x_taps: Sequence[torch.Tensor], y: torch.Tensor, packed: torch.Tensor,
                              grad_precision: str, state: torch.Tensor, s1: torch.Tensor | None = None,
                              s2: torch.Tensor | None = None):
    """(S1, S2), each float32 (B, 1475), of a prepared target (x, its five float NHWC taps) against y, with everything a
    gradient needs left in `state` (uint8, at least dists_target_step_bytes): ONE library call.  packed: the f32s blob."""
    dev, b, h, w, tp = _step_args("dists_target_step_forward", x, x_taps, y, state)
    _need_cuda(packed)
    s1 = _out_or_empty(s1, (b, TOTAL_CHNS), torch.float32, dev)
    s2 = _out_or_empty(s2, (b, TOTAL_CHNS), torch.float32, dev)
    _call(dev, lib().nqa_dists_target_step_forward, ptr(x), tp, ptr(y), b, h, w, ptr(packed), GRAD_PREC_ID[grad_precision],
          ptr(state), state.numel(), ptr(s1), ptr(s2), stream_ptr(dev))
    return s1, s2


def dists_target_step_backward(x: torch.Tensor, x_taps: Sequence[torch.Tensor], y: torch.Tensor, g_s1: torch.Tensor,
                               g_s2: torch.Tensor, blobs, w0: torch.Tensor, grad_precision: str, state: torch.Tensor,
                               gy: torch.Tensor | None = None) -> torch.Tensor:
    """dL/dy, float32 (B,3,H,W), given dL/dS1, dL/dS2 (B, 1475) from the state dists_target_step_forward left for the same
    arguments: ONE library call.  blobs: {layer 1..12: its data-gradient layer packed for the rung}; w0: conv1_1's float
    OIHW weights on the device."""
    dev, b, h, w, tp = _step_args("dists_target_step_backward", x, x_taps, y, state)
    _need_cuda(g_s1, g_s2, w0, *[blobs[l] for l in range(1, 13)])
    g_s1, g_s2, w0 = _f32c(g_s1), _f32c(g_s2), _f32c(w0)
    assert tuple(g_s1.shape) == tuple(g_s2.shape) == (b, TOTAL_CHNS) and tuple(w0.shape) == (64, 3, 3, 3)
    gy = _out_or_empty(gy, (b, 3, h, w), torch.float32, dev)
    lp = (C.c_void_p * 12)(*[ptr(blobs[l]) for l in range(1, 13)])
    _call(dev, lib().nqa_dists_target_step_backward, ptr(x), tp, ptr(y), b, h, w, ptr(g_s1), ptr(g_s2), lp, ptr(w0),
          GRAD_PREC_ID[grad_precision], ptr(state), state.numel(), ptr(gy), stream_ptr(dev))
    return gy


def dists_score_backward(alpha: torch.Tensor, beta: torch.Tensor, g_score: torch.Tensor):
    """(dL/dS1, dL/dS2), each float32 (B, 1475), of dists_score for dL/dscore = g_score (B,): -g_score[b] * alpha[c] / w and
    -g_score[b] * beta[c] / w with w = sum(alpha) + sum(beta) (no autograd; the library's kernel)."""
    dev = _need_cuda(alpha, beta, g_score)
    a, b_, g = _f32c(alpha.detach().reshape(-1)), _f32c(beta.detach().reshape(-1)), _f32c(g_score.detach().reshape(-1))
    assert a.numel() == b_.numel() == TOTAL_CHNS
    g1 = torch.empty((g.numel(), TOTAL_CHNS), dtype=torch.float32, device=dev)
    g2 = torch.empty_like(g1)
    _call(dev, lib().nqa_dists_score_backward, ptr(a), ptr(b_), ptr(g), g.numel(), ptr(g1), ptr(g2), stream_ptr(dev))
    return g1, g2


def _exponent_args(who: str, g: torch.Tensor, k: torch.Tensor, k_total: torch.Tensor | None):
    """What grad_exponent and grad_exponent_half check and allocate alike: g contiguous, k and k_total int32 with one
    entry per image g[i] -> (device, images, elements per image, the reduction's scratch, k_total's pointer or None)."""
    dev = _need_cuda(g, k)
    n = g.shape[0]
    assert g.is_contiguous()
    assert k.dtype == torch.int32 and k.is_contiguous() and k.numel() == n
    assert k_total is None or (k_total.dtype == torch.int32 and k_total.is_contiguous() and k_total.numel() == n
                               and k_total.device == dev)
    per = g.numel() // n
    nbytes = lib().nqa_grad_exponent_bytes(n, per)
    if not nbytes:
        raise _lib.NqaError(f"{who}: unsupported shape {tuple(g.shape)} (elements per image must be a multiple of 4)")
    return dev, n, per, torch.empty(nbytes, dtype=torch.uint8, device=dev), None if k_total is None else ptr(k_total)


def grad_exponent(g: torch.Tensor, k: torch.Tensor, k_total: torch.Tensor | None = None) -> None:
    """k[i] (int32, on the device) = the exponent with max|g[i]| * 2^k[i] in [128, 256), 0 where that maximum is 0 or
    not finite; k_total[i] += k[i].  g: float, image i = g[i].  Nothing comes back to the host."""
    assert g.dtype == torch.float32
    dev, n, per, buf, kt = _exponent_args("grad_exponent", g, k, k_total)
    _call(dev, lib().nqa_grad_exponent, ptr(g), n, per, ptr(buf), buf.numel(), ptr(k), kt, stream_ptr(dev))


def relu_mask_split16_scaled(g: torch.Tensor, act: torch.Tensor, act_is_split16: bool, k: torch.Tensor) -> torch.Tensor:
    """relu_mask_split16(g * 2^k[image], act): the exponents (int32, one per image g[i]) are read on the device."""
    dev = _need_cuda(g, act, k)
    g = _f32c(g)
    assert act.dtype == torch.float32 and act.is_contiguous() and act.shape == g.shape
    n, c = g.shape[0], g.shape[-1]
    assert k.dtype == torch.int32 and k.is_contiguous() and k.numel() == n
    out = torch.empty_like(g)
    _call(dev, lib().nqa_relu_mask_split16_scaled, ptr(g), ptr(act), int(act_is_split16), n, g.numel() // (n * c), c, ptr(k),
          ptr(out), stream_ptr(dev))
    return out


def l2pool_backward_scaled(tap: torch.Tensor, g_pooled: torch.Tensor, g_tap: torch.Tensor, k_total: torch.Tensor) -> torch.Tensor:
    """g_tap * 2^k_total[image] + d(L2-pool)/d(tap) applied to g_pooled, as a new float (n,H,W,C) tensor.  g_pooled: a
    float map or a half one (the f16 chain's), each through its own entry point; the two agree bit for bit on the halves
    converted to float (include/nqa.h)."""
    dev = _need_cuda(tap, g_pooled, g_tap, k_total)
    n, h, w, c = tap.shape
    assert tap.dtype == torch.float32 and tap.is_contiguous()
    assert g_tap.shape == tap.shape and g_tap.dtype == torch.float32 and g_tap.is_contiguous()
    assert g_pooled.shape == (n, (h + 1) // 2, (w + 1) // 2, c)
    assert k_total.dtype == torch.int32 and k_total.is_contiguous() and k_total.numel() == n
    half = g_pooled.dtype == torch.float16
    g_pooled = g_pooled.contiguous() if half else _f32c(g_pooled)
    out = torch.empty_like(tap)
    _call(dev, lib().nqa_l2pool_backward_scaled_half if half else lib().nqa_l2pool_backward_scaled, ptr(tap), ptr(g_pooled),
          ptr(g_tap), ptr(k_total), n, h, w, c, ptr(out), stream_ptr(dev))
    return out


def conv1_1_backward_scaled(g: torch.Tensor, relu1_1_split16: torch.Tensor | None, w0: torch.Tensor, k: torch.Tensor,
                            k_total: torch.Tensor) -> torch.Tensor:
    """conv1_1_backward(g * 2^k[image] * (relu1_1 > 0), w0) * 2^-k_total[image]: float NHWC (n,H,W,64) -> float NCHW
    (n,3,H,W).  relu1_1_split16: conv1_1's f32s output (None: no mask).  g: a float map or a half one (the f16 chain's),
    each through its own entry point; the two agree bit for bit on the halves converted to float (include/nqa.h)."""
    dev = _need_cuda(g, w0, k, k_total)
    half = g.dtype == torch.float16
    g, w0 = (g.contiguous() if half else _f32c(g)), _f32c(w0)
    n, h, w, c = g.shape
    assert c == 64 and tuple(w0.shape) == (64, 3, 3, 3)
    assert relu1_1_split16 is None or (relu1_1_split16.shape == g.shape and relu1_1_split16.dtype == torch.float32
                                       and relu1_1_split16.is_contiguous() and relu1_1_split16.device == dev)
    for t in (k, k_total):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.numel() == n
    out = torch.empty((n, 3, h, w), dtype=torch.float32, device=dev)
    _call(dev, lib().nqa_conv1_1_backward_scaled_half if half else lib().nqa_conv1_1_backward_scaled, ptr(g),
          None if relu1_1_split16 is None else ptr(relu1_1_split16), ptr(w0), ptr(k), ptr(k_total), n, h, w, ptr(out),
          stream_ptr(dev))
    return out


# ---- the half gradient chain: grad_precision="f16" (include/nqa.h, "The same chain on HALF gradient maps") ----------
def pack_conv_half(w) -> torch.Tensor:
    """One 3x3 layer (float32 OIHW, cout % 64 == 0, cin % 32 == 0) as f16 rows, zero bias -> CPU uint8 blob."""
    return _pack_conv("half", w)


def _is_grad_map(g: torch.Tensor) -> bool:
    """Whether g is a half map (else it must be float); contiguous either way."""
    assert g.dtype in (torch.float16, torch.float32) and g.is_contiguous()
    return g.dtype == torch.float16


def conv3x3_half(inp: torch.Tensor, blob: torch.Tensor, cout: int) -> torch.Tensor:
    """f16 NHWC (n,H,W,cin) -> f16 NHWC (n,H,W,cout) through a layer packed by pack_conv_half: no bias, no ReLU."""
    dev = _need_cuda(inp, blob)
    assert inp.dtype == torch.float16 and inp.is_contiguous()
    n, h, w, cin = inp.shape
    out = torch.empty((n, h, w, cout), dtype=torch.float16, device=dev)
    _call(dev, lib().nqa_conv3x3_half, ptr(inp), n, h, w, cin, cout, ptr(blob), ptr(out), stream_ptr(dev))
    return out


def grad_exponent_half(g: torch.Tensor, k: torch.Tensor, k_total: torch.Tensor | None = None) -> None:
    """grad_exponent for the half chain: k[i] with max|g[i]| * 2^k[i] in [8, 16); g float or half, image i = g[i]."""
    half = _is_grad_map(g)
    dev, n, per, buf, kt = _exponent_args("grad_exponent_half", g, k, k_total)
    _call(dev, lib().nqa_grad_exponent_half, ptr(g), int(half), n, per, ptr(buf), buf.numel(), ptr(k), kt, stream_ptr(dev))


def relu_mask_f16_scaled(g: torch.Tensor, act: torch.Tensor, act_is_split16: bool, k: torch.Tensor) -> torch.Tensor:
    """(g * 2^k[image]) * (act > 0) rounded to half once, as a plain f16 NHWC map of g's shape; g float or half, act a
    float map or split16 records; the exponents (int32, one per image g[i]) are read on the device."""
    dev = _need_cuda(g, act, k)
    half = _is_grad_map(g)
    assert act.dtype == torch.float32 and act.is_contiguous() and act.shape == g.shape
    n, c = g.shape[0], g.shape[-1]
    assert k.dtype == torch.int32 and k.is_contiguous() and k.numel() == n
    out = torch.empty(g.shape, dtype=torch.float16, device=dev)
    _call(dev, lib().nqa_relu_mask_f16_scaled, ptr(g), int(half), ptr(act), int(act_is_split16), n, g.numel() // (n * c), c,
          ptr(k), ptr(out), stream_ptr(dev))
    return out


# ---- windowed moments of the A-DISTS head (include/nqa.h, nqa_window_moments.hip) ---------------------------------
WINDOW = 21  # the library's window: the normalised 21-tap Gaussian of sigma 7, as head.gauss_1d(21, .)


def _window_planes(x: torch.Tensor, y: torch.Tensor | None):
    dev = _need_cuda(*([x] if y is None else [x, y]))
    for t in (x,) if y is None else (x, y):
        if t.dim() != 4 or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"window_moments: expected contiguous float32 NCHW maps, got {t.dtype} {tuple(t.shape)}")
    if y is not None and y.shape != x.shape:
        raise ValueError(f"window_moments: x {tuple(x.shape)} and y {tuple(y.shape)} differ")
    return dev


def window_moments(x: torch.Tensor, y: torch.Tensor | None = None, window: int = WINDOW):
    """The n x n Gaussian window means (n = window, 3..63; sigma n / 3, head.gauss_1d's taps) of float32 NCHW maps
    (B,C,H,W), each (B,C,H-n+1,W-n+1): (E[x], E[x^2]) of x alone, (E[x], E[y], E[x^2], E[y^2], E[xy]) of a pair.  One
    launch; the products are formed in registers.  21 runs the specialised kernels, every other size the generic ones."""
    win = check_window(window)
    dev = _window_planes(x, y)
    b, c, h, w = x.shape
    n = 2 if y is None else 5
    out = torch.empty((n, b, c, max(h - win + 1, 0), max(w - win + 1, 0)), dtype=torch.float32, device=dev)
    _call(dev, lib().nqa_window_moments_forward_n, ptr(x), None if y is None else ptr(y), b * c, h, w, win, ptr(out),
          stream_ptr(dev))
    return out.unbind(0)


def window_moments_backward(x: torch.Tensor, y: torch.Tensor | None, grads: Sequence, need=(True, True),
                            window: int = WINDOW):
    """(gx, gy) of window_moments(x, y, window) for the upstream gradients `grads` of its maps (two without y, five with; None =
    zero): gx = W^T g_x + 2 x W^T g_xx + y W^T g_xy and its mirror, every pixel summing over the windows that contain it.
    None where need[i] is False (nothing is computed for that side; the other is bit-identical) and for gy without y."""
    win = check_window(window)
    dev = _window_planes(x, y)
    b, c, h, w = x.shape
    grads = list(grads)
    if len(grads) != (2 if y is None else 5):
        raise ValueError(f"window_moments_backward: expected {2 if y is None else 5} upstream maps, got {len(grads)}")
    g5 = [grads[0], None, grads[1], None, None] if y is None else grads
    shape = (b, c, h - win + 1, w - win + 1)
    for i, g in enumerate(g5):
        if g is None:
            continue
        _need_cuda(x, g)
        if tuple(g.shape) != shape:
            raise ValueError(f"window_moments_backward: upstream map of shape {tuple(g.shape)}, expected {shape}")
        g5[i] = _f32c(g)
    need_x, need_y = bool(need[0]), bool(need[1]) and y is not None
    if not (need_x or need_y):
        return None, None
    gx = torch.empty_like(x) if need_x else None
    gy = torch.empty_like(y) if need_y else None
    _call(dev, lib().nqa_window_moments_backward_n, ptr(x), None if y is None else ptr(y), b * c, h, w, win,
          *[None if g is None else ptr(g) for g in g5], None if gx is None else ptr(gx), None if gy is None else ptr(gy),
          stream_ptr(dev))
    return gx, gy


# ---- one stage of the A-DISTS head's backward towards y (include/nqa.h, nqa_adists_backward.hip) ------------------
def adists_ts_backward(x: torch.Tensor, y: torch.Tensor, q: torch.Tensor, wgt: torch.Tensor, ps: torch.Tensor,
                       u: torch.Tensor, mask: bool, coff: int = 0, nhwc: bool = False, ws: Workspace | None = None,
                       out: torch.Tensor | None = None, window: int = WINDOW) -> torch.Tensor:
    """dL/dy of one A-DISTS stage with x fixed (include/nqa.h, nqa_adists_ts_backward): x, y float32 planar maps
    (B,C,H,W); q (8,B,ctot) and wgt (B,ctot) as adists_front leaves them, the stage's channels at columns coff .. coff+C;
    ps (B,mh,mw) the stage's ps_prod of adists_chain; u (B,) = dL/dD.  mask: times the ReLU mask (y > 0).  Returns the
    gradient planar (B,C,H,W), or NHWC (B,H,W,C) with nhwc=True (what pyramid_backward_device takes).  window: the
    stage's window size n (3..63): windowed where H, W >= n, with ps (B,H-n+1,W-n+1), else the global branch."""
    win = check_window(window)
    dev = _need_cuda(x, y, q, wgt, ps, u)
    for t in (x, y):
        if t.dim() != 4 or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() == 0:
            raise ValueError(f"adists_ts_backward: expected non-empty contiguous float32 NCHW maps, got {t.dtype} {tuple(t.shape)}")
    if y.shape != x.shape:
        raise ValueError(f"adists_ts_backward: x {tuple(x.shape)} and y {tuple(y.shape)} differ")
    b, c, h, w = (int(v) for v in x.shape)
    coff = int(coff)
    if q.dim() != 3 or q.shape[0] != 8 or q.shape[1] != b or coff < 0 or coff + c > q.shape[2]:
        raise ValueError(f"adists_ts_backward: q must be (8, {b}, ctot) with columns {coff} .. {coff + c} inside, got {tuple(q.shape)}")
    ctot = int(q.shape[2])
    windowed = h >= win and w >= win
    mshape = (b, h - win + 1, w - win + 1) if windowed else (b, 1, 1)
    for name, t, sh in (("q", q, (8, b, ctot)), ("wgt", wgt, (b, ctot)), ("ps", ps, mshape), ("u", u, (b,))):
        if tuple(t.shape) != sh or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"adists_ts_backward: {name} must be contiguous float32 {sh}, got {t.dtype} {tuple(t.shape)}")
    shape = (b, h, w, c) if nhwc else (b, c, h, w)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"adists_ts_backward: out must be contiguous float32 {shape}, got {out.dtype} {tuple(out.shape)}")
    nbytes = lib().nqa_adists_ts_backward_bytes_n(b, c, h, w, win)
    buf = (ws or Workspace()).get(max(nbytes, 16), dev)
    _call(dev, lib().nqa_adists_ts_backward_n, ptr(x), ptr(y), b, c, h, w, win, ptr(q), ptr(wgt), ctot, coff, ptr(ps), ptr(u),
          int(bool(mask)), int(bool(nhwc)), ptr(buf), buf.numel(), ptr(out), stream_ptr(dev))
    return out
