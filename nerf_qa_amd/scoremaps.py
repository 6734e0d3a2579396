"""Score-map targets of the no-reference dataset prep: the build's counterpart of the one loop of the reference that
calls A-DISTS with as_map=True (nerf_nr_qa_prep_4.py:55-146).

Per frame of a scene and per render directory of that scene the script runs `adists_model(render, gt, as_map=True)`
(:70), then on the CPU in float64: clamp at 1e-10, per-pixel std and mean across the K renders, amin / amax per map and
of the std and mean maps, a -log10 rescale of each to 0..255, one (mean, map, std) byte image per render (:71-135), and
six '{:.4e}' columns of the -log10 extrema per frame (:137-146).  Here the K maps of a frame come from one batched call
and everything after them is three HIP kernels (csrc/nqa_score_maps.hip): nothing crosses to the host but what the
caller reads.  Reading and writing image files and the pandas grouping stay with the caller.
"""
from __future__ import annotations

from typing import Dict, List

import torch

from . import ops
from ._lib import NqaError


def to_str(array) -> str:
    """nerf_nr_qa_prep_4.py:137-139: the list of '{:.4e}' strings, as Python prints a list of str."""
    return str(["{:.4e}".format(num) for num in array])


def center_crop(img: torch.Tensor, scale: float = 0.7) -> torch.Tensor:
    """The crop of nerf_nr_qa_prep_4.py:62-66 on the last two axes of `img` (..., H, W), as a view: h, w = int(H * scale),
    int(W * scale) (truncated), offsets (H - h) // 2, (W - w) // 2."""
    big_h, big_w = int(img.shape[-2]), int(img.shape[-1])
    h, w = int(big_h * scale), int(big_w * scale)
    i, j = (big_h - h) // 2, (big_w - w) // 2
    return img[..., i:i + h, j:j + w]


class ScoreMaps:
    """What score_maps returns.  With renders given as (F,K,3,H,W): rgb (F,K,H,W,3) uint8, maps (F,K,H,W) float32, logs
    (F,2K+4) float64, all on the device; log_max / log_min (F,K) and log_std_max / log_std_min / log_mean_max /
    log_mean_min (F,) are views of logs -- the values :80-99 append per frame.  With renders given as (K,3,H,W) the
    leading F axis is dropped everywhere."""

    def __init__(self, rgb, maps, logs, single: bool):
        k = maps.shape[1]
        if single:
            rgb, maps, logs = rgb[0], maps[0], logs[0]
        self.rgb, self.maps, self.logs = rgb, maps, logs
        self.log_max, self.log_min = logs[..., :k], logs[..., k:2 * k]
        self.log_std_max, self.log_std_min = logs[..., 2 * k], logs[..., 2 * k + 1]
        self.log_mean_max, self.log_mean_min = logs[..., 2 * k + 2], logs[..., 2 * k + 3]


def _checks(renders, gt, who="score_maps"):
    """The argument checks of score_maps, in the wording of ADISTS._group_checks; (renders (F,K,3,H,W), gt (F,3,H,W),
    whether the caller gave one frame without an F axis)."""
    shapes = f"{tuple(getattr(renders, 'shape', ()))} / {tuple(getattr(gt, 'shape', ()))}"
    expects = f"{who} expects renders (K,3,H,W) or (F,K,3,H,W) and ground truth (3,H,W), (1,3,H,W) or (F,3,H,W), got {shapes}"
    if not (torch.is_tensor(renders) and torch.is_tensor(gt)) or renders.dim() not in (4, 5) or gt.dim() not in (3, 4) \
            or renders.numel() == 0 or gt.numel() == 0:
        raise ValueError(expects)
    single = renders.dim() == 4
    r5 = renders[None] if single else renders
    g4 = gt[None] if gt.dim() == 3 else gt
    f = r5.shape[0]
    if r5.shape[2] != 3 or g4.shape[1:] != r5.shape[2:] or g4.shape[0] not in (1, f) or (single and g4.shape[0] != 1):
        raise ValueError(expects)
    if torch.is_grad_enabled() and (renders.requires_grad or gt.requires_grad):
        raise ValueError(f"{who} does not differentiate: detach the images, or call forward(x, y, as_loss=True) per pair")
    if not (renders.is_cuda and gt.is_cuda):
        raise NqaError("nerf_qa_amd runs on the GPU only: got tensors on %s / %s (move inputs and the module to cuda; "
                       "there is no CPU fallback)" % (renders.device, gt.device))
    if renders.device != gt.device:
        raise NqaError("tensors on different devices")
    return r5, g4.expand(f, *g4.shape[1:]), single


def _pair_maps(adists, renders, gt):
    """(F,K,H,W): the K * F pairs (render, its frame's ground truth) through the module's own batched scoring call."""
    f, k, _, h, w = renders.shape
    prec, ws, n = adists.precision_for(h, w), adists._ws, adists._window()
    x = renders.reshape(f * k, 3, h, w)
    y = gt[:, None].expand(f, k, 3, h, w).reshape(f * k, 3, h, w)
    _, m = adists._batched(x, y, prec, lambda a, b, packed: ops.adists_forward(a, b, packed, prec, ws, with_map=True,
                                                                               window=n))
    return m.reshape(f, k, h, w)


def _shared_bytes(pairs: int, h: int, w: int, window: int) -> int:
    """Device bytes the shared path holds for `pairs` renders beside their images: the five float taps of every image,
    the ground truth's expanded to the pairs, both joined for the front (4 * 122 floats per pixel and image in all:
    64 + 128/4 + 256/16 + 512/64 + 512/256), and the largest of the staged calls' own workspaces."""
    return 4 * pairs * 122 * h * w * 4 + int(ops.lib().nqa_adists_workspace_bytes_n(pairs, h, w, window, ops.prec_id("f32s")))


def _shared_chunk(adists, renders, gt):
    """(F,K,H,W) for renders (F,K,3,H,W), gt (F,3,H,W) float32 contiguous from ONE pyramid of the F * (K + 1) images:
    autograd.adists_y_forward's own sequence of staged calls (x = the renders), with the chain's map pointer."""
    from . import autograd
    f, k, _, h, w = renders.shape
    b, prec, dev, ws, n = f * k, "f32s", renders.device, adists._ws, adists._window()
    x = renders.reshape(b, 3, h, w)
    y = gt[:, None].expand(f, k, 3, h, w).reshape(b, 3, h, w).contiguous()
    taps = autograd.pyramid_taps(adists, torch.cat([x, gt]))
    tx = [t[:b] for t in taps]
    ty = [t[b:, None].expand(f, k, *t.shape[1:]).reshape(b, *t.shape[1:]).contiguous() for t in taps]
    q = torch.empty((8, b, ops.TOTAL_CHNS), dtype=torch.float32, device=dev)
    wgt = torch.empty((b, ops.TOTAL_CHNS), dtype=torch.float32, device=dev)
    ops.adists_front_into(x, y, [torch.cat([a, c]) for a, c in zip(tx, ty)], prec, q, wgt, ws)
    dims, _ = ops.adists_chain_dims(h, w, n)
    maps = [torch.empty((4, b) + d, dtype=torch.float32, device=dev) for d in dims]  # gamma, tw, sw, ps_prod per stage
    off = 0
    for s, c in enumerate(ops.CHNS):
        fx, fy = (x, y) if s == 0 else (tx[s - 1], ty[s - 1])
        ops.adists_window_stage_into(fx, fy, q[:, :, off:off + c].contiguous(), wgt[:, off:off + c].contiguous(), prec, 0,
                                     maps[s][0], maps[s][1], maps[s][2], n)
        off += c
    d = torch.empty((b,), dtype=torch.float32, device=dev)
    out = torch.empty((b, h, w), dtype=torch.float32, device=dev)
    ops.adists_chain_into([m[0] for m in maps], [m[1] for m in maps], [m[2] for m in maps], h, w, [m[3] for m in maps], d,
                          out, ws, n)
    return out.reshape(f, k, h, w)


def _shared_maps(adists, renders, gt):
    """_shared_chunk over slices of frames -- or, where one frame's renders do not fit, of its renders -- so that the
    scratch stays under NQA_MAX_WORKSPACE_GB (a slice of renders runs its frame's ground truth again)."""
    f, k, _, h, w = renders.shape
    n = adists._window()
    renders, gt = renders.float().contiguous(), gt.float().contiguous()
    mf = ops._max_pairs(lambda frames: _shared_bytes(frames * k, h, w, n), f)
    mk = ops._max_pairs(lambda pairs: _shared_bytes(pairs, h, w, n), k) if mf == 1 else k
    if mf == f and mk == k:
        return _shared_chunk(adists, renders, gt)
    out = torch.empty((f, k, h, w), dtype=torch.float32, device=renders.device)
    for f0 in range(0, f, mf):
        for k0 in range(0, k, mk):
            out[f0:f0 + mf, k0:k0 + mk] = _shared_chunk(adists, renders[f0:f0 + mf, k0:k0 + mk].contiguous(), gt[f0:f0 + mf])
    return out


def _frames_per_call(k: int, h: int, w: int) -> int:
    """How many frames one nqa_score_maps call takes (include/nqa.h: F * K <= 65535, F * K * H * W * 3 < 2^31); at least
    one, so that a single frame past the limits meets the library's own refusal."""
    return max(1, min(65535 // k, ((1 << 31) - 1) // (k * h * w * 3)))


def score_maps(adists, renders, gt, share_gt: bool = False) -> ScoreMaps:
    """The score-map targets of nerf_nr_qa_prep_4.py:55-135 for F frames of K renders each, on the GPU.

    renders: (K,3,H,W) for one frame, or (F,K,3,H,W); gt: the frames' ground truth, (3,H,W), (1,3,H,W) or (F,3,H,W).
    The argument order of the metric is the script's (:70): x = the RENDER, y = the ground truth -- the other way round
    from prep.py:186 and from every other helper of this package, which pass x = the reference.  A-DISTS is asymmetric
    (its texture probabilities and channel weights come from x), so the order matters.

    The maps are `adists(renders, gt expanded to the renders, as_map=True)[:, 0]` for all F * K pairs as one batch, bit
    for bit, in adists.precision_for(H, W), through the module's own batched call (ADISTS._batched: where that splits a
    batch over two streams, the statistics' block partition follows the half-batch, 1e-7, as for the scores); rgb and
    logs are ops.score_maps of them (the arithmetic of :71-133: see include/nqa.h, nqa_score_maps).  Returns a ScoreMaps.

    share_gt=True (opt-in): the ground truth's pyramid runs once for its K renders -- one pyramid of F * (K + 1) images
    instead of 2 * F * K -- through the staged entry points of the loss path, always in f32s.  The maps then agree with
    the default's to a summation order, not bit for bit.

    ValueError for shapes that do not fit and images that require grad, NqaError for tensors off the GPU."""
    r5, g4, single = _checks(renders, gt)  # (in the caller's grad mode: images that require grad are refused)
    f, k, _, h, w = r5.shape
    with torch.no_grad():
        maps = (_shared_maps if share_gt else _pair_maps)(adists, r5, g4).contiguous()
        n = _frames_per_call(k, h, w)
        if n >= f:
            rgb, logs = ops.score_maps(maps, adists._ws)
        else:
            parts = [ops.score_maps(maps[i:i + n], adists._ws) for i in range(0, f, n)]
            rgb, logs = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
    return ScoreMaps(rgb, maps, logs, single)


class ScoreMapColumns:
    """The six CSV columns of nerf_nr_qa_prep_4.py:137-146 for one scene: add() every ScoreMaps of the scene in frame
    order (one frame or several at a time, all with the same K), then columns().  The extrema stay on the device until
    columns() reads them, once."""

    def __init__(self):
        self._logs: List[torch.Tensor] = []

    def add(self, result: ScoreMaps) -> None:
        logs = result.logs if result.logs.dim() == 2 else result.logs[None]
        if self._logs and logs.shape[1] != self._logs[0].shape[1]:
            raise ValueError(f"ScoreMapColumns: frames of {(self._logs[0].shape[1] - 4) // 2} renders so far, now "
                             f"{(logs.shape[1] - 4) // 2}")
        self._logs.append(logs)

    def columns(self) -> Dict[str, object]:
        """score_map_log_max / score_map_log_min: per render the to_str of its list over frames (:141-142, one row of the
        group per render); score_map_log_std_max / _std_min / _mean_max / _mean_min: one to_str per scene (:143-146)."""
        if not self._logs:
            raise ValueError("ScoreMapColumns: no frame added")
        logs = torch.cat(self._logs).cpu()
        k = (logs.shape[1] - 4) // 2
        per_scene = ("score_map_log_std_max", "score_map_log_std_min", "score_map_log_mean_max", "score_map_log_mean_min")
        out = {"score_map_log_max": [to_str(logs[:, i].tolist()) for i in range(k)],
               "score_map_log_min": [to_str(logs[:, k + i].tolist()) for i in range(k)]}
        out.update({name: to_str(logs[:, 2 * k + i].tolist()) for i, name in enumerate(per_scene)})
        return out
