"""Drop-in `DISTS` for nerf_qa.DISTS_pytorch.DISTS_pt.DISTS, computed by libnqa_hip.so.

Mirrors the reference's callable surface (nerf_qa/DISTS_pytorch/DISTS_pt.py):
  DISTS(load_weights=True, from_feats=False)                       :27-80
  .forward(x, y, require_grad=False, batch_average=False,
           warp=None, certainty=None)                              :105-148
  .forward_once(x) -> [x, relu1_2, relu2_2, relu3_3, relu4_3, relu5_3]   :91-103
  .forward_from_feats(feats0, feats1, batch_average=False)         :181-208
  .project_weights()                                               :82-89
  prepare_image(image, resize=True, keep_aspect_ratio=False)       :210-217
and keeps the attributes callers read: alpha, beta (nn.Parameter (1,1475,1,1)), chns,
stage1..stage5 (nn.Sequential holding the frozen fp32 Conv2d weights, same child names),
mean, std.

What runs where: the 13 conv3x3+ReLU, the 4 L2-pools and all statistics are HIP kernels
(ops.dists_forward).  PyTorch only holds memory and, when alpha/beta need gradients (the
fine-tuning loop, run_nerf_qa.py:433-461), evaluates the 2950-term weighted sum so that
autograd reaches alpha and beta without a custom backward.  CPU tensors are refused.
"""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.nn as nn

from .. import ops
from .._lib import NqaError, prec_id
from ..vgg_weights import load_vgg16_convs

_DATA = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data", "dists_alpha_beta.npz")
# "auto" (the default) picks, per frame size, the fastest precision mode that is KNOWN to hold the reference's scores
# to well inside 1e-4 with the VGG weights this module actually carries:
#   * frames below AUTO_MIN_PIXELS (128 x 128, A-DISTS' threshold too) always run in f32s (split-f16 products on float32
#     activations, <= 1e-6): the faster modes' |dscore| has a tail on small frames, whose deep-stage statistics run over
#     a handful of pixels (tools/gpu_stress_small.py: f16, 1 of 800 random frames up to 64x64 at 1.2e-4; f16w, the worst
#     of 6 000 random pairs from 96x96 up was a 76x135 frame at 5.4e-5), and such frames are launch-bound anyway;
#   * larger frames run in the FASTEST of six modes that a one-time calibration with these very weights admits:
#       f16    one MFMA per product, f16 activations and weights                      (~2.8x the throughput of f32s)
#       f16w   f16 activations x two-term (hi, lo) weights in ALL stages, 2 MFMAs per product       (~1.6x)
#       f32m4  the same in stages 1..4, stage 5 as f32s                                            (~1.55x)
#       f32m   ... stages 1..3, stages 4..5 as f32s                                                (~1.4x)
#       f32m2  ... stages 1..2                                                                     (~1.25x)
#       f32s   float activations, three-term split products, <= 1e-6                 (always admitted)
#     The first time a frame of a size class arrives (AUTO_CLASSES below), 256..384 synthetic pairs of that class's own
#     sizes (additive noise at two levels, 5x5 blur, independent content) go through all six on the GPU (0.15 s for the
#     smallest class, 4.3 s for the 1080p class).  A mode PASSES when its deviation from f32s has rms <= AUTO_F16_RMS
#     (2e-5) AND either max <= AUTO_SAFE_MAX (1.5e-5: seven times below the bar, whatever the tail looks like) or max <=
#     AUTO_F16_BUDGET (6e-5) with max / rms <= AUTO_TAIL (4.2: the deviations look like noise, not like outliers -- 384
#     Gaussian samples give 3.2 +- 0.3); it is ADMITTED when it and every more accurate mode pass.
# Why a measurement and not a rule: tools/cpu_prec_layers.py shows the 16-bit error is spread evenly over all 13
# layers and over both operands (weights and activations each ~2.3e-5 rms at stand-in gain 1.6), so no small set of
# "two-term" layers repairs it -- what decides whether 11-bit operands are enough is how the weights at hand grow
# the activations with depth, which one cheap comparison on the device answers.  Why the tail test: the deviations of
# the faster modes are outlier-driven once activations grow (nearly dead channels whose S2 is a quotient of two tiny
# moments): on 692 random pairs f32m at gain 1.3 has rms 7e-6 but a worst pair of 9.9e-5, f16 at gain 1.0 rms 1.1e-5
# and 4.8e-5 (profiles/r03_stress_modes_692.txt).  What the three pinned stand-in weight sets calibrate to
# (profiles/r03_cal_classes.txt): gain 1.0 -> f16w below 224x224 pixels (f16: max 6.5e-5, tail 4.8 -- refused) and plain
# f16 from there up (3.5e-5, tail 3.0); gain 1.3 -> f32m2 / f32m / f32m / f32m4 by class; gain 1.6 -> f32s everywhere.
DEFAULT_PRECISION = "auto"
# The precision of the GRADIENT chain of a loss step (autograd.pyramid_backward_device), apart from `precision`, which is
# the forward's: "f32s" (the default: split16 gradient records, three-term products, a second accumulator) or "f16" (plain
# half gradient maps, half weights, one MFMA per product; per-image power-of-two renormalisation into [8, 16)).  The
# forward of a loss step, its values, its ReLU masks and the statistics' / A-DISTS head's backward are the same in both.
DEFAULT_GRAD_PRECISION = "f32s"
GRAD_PRECISIONS = ("f32s", "f16")


def resolve_grad_precision(grad_precision=None) -> str:
    """The argument, else $NQA_GRAD_PRECISION, else "f32s"; ValueError for anything but "f32s" / "f16"."""
    v = grad_precision or os.environ.get("NQA_GRAD_PRECISION") or DEFAULT_GRAD_PRECISION
    if v not in GRAD_PRECISIONS:
        raise ValueError(f"grad_precision must be one of {GRAD_PRECISIONS}, got {v!r}")
    return v


# How forward_target(require_grad=True) issues its step: "python" (the default: autograd.DistsTargetSimilarities, about a
# hundred library calls from nerf_qa_amd/autograd.py) or "c" (autograd.DistsTargetStep: the library's two step calls,
# nqa_dists_target_step_forward / _backward, on one state tensor -- the same launches, the same bits, less host time).
DEFAULT_TARGET_STEP = "python"
TARGET_STEPS = ("python", "c")


def resolve_target_step(target_step=None) -> str:
    """The argument, else $NQA_TARGET_STEP, else "python"; ValueError for anything but "python" / "c"."""
    v = target_step or os.environ.get("NQA_TARGET_STEP") or DEFAULT_TARGET_STEP
    if v not in TARGET_STEPS:
        raise ValueError(f"target_step must be one of {TARGET_STEPS}, got {v!r}")
    return v
AUTO_MIN_PIXELS = 128 * 128
AUTO_F16_BUDGET = 6e-5  # on max |score_mode - score_f32s| over the calibration pairs ...
AUTO_TAIL = 4.2         # ... and then only if max / rms looks like noise (384 Gaussian samples: 3.2 +- 0.3), not outliers;
AUTO_SAFE_MAX = 1.5e-5  # a max this far below the bar is admitted whatever the shape of the tail (was 3e-5: a heavy-tailed
#                         rung admitted at 2.6e-5 over 384 pairs reached 5.5e-5 over 1 450 unseen ones; then 2e-5 -- and
#                         round 4's stress run on NeRF-like content took f32m4, admitted at 2.0e-5 on the gain-1.3 weights,
#                         to 6.9e-5 over 531 unseen 1-2 Mpx pairs: a factor of 3.5.  At 1.5e-5 that factor leaves 5e-5, and
#                         the gain-1.3 verdict no longer flips between f32m4 and f32m with the box)
AUTO_F16_RMS = 2e-5     # on the rms, always
# The content guard of `auto` (round 4): a pair whose reference OR rendered frame is nearly flat -- pixel variance (mean over
# the colour planes) below AUTO_FLAT_VAR, i.e. a standard deviation under ~4.5 % of the range: fog, a blank wall, an empty
# render -- is rescored in f32s whatever rung its size class calibrated to.  On such frames almost every VGG channel has a
# tiny variance and S2 is a quotient of two tiny moments in all 1 475 of them: tools/gpu_flat_frames.py has plain f16 at
# 6-9e-5 (once 1.45e-4) and f32m at 4-8e-5 from f32s for one colour +- 0 .. 10 % of smooth variation against a render with
# floaters, at 1.5 Mpx, where texture-rich content stays below 3.6e-5 / 1.5e-5; the 6 000-pair stress run's worst case
# (7.0e-5) is this family too.  No calibration family can stand for it without costing everyone the fast rungs; the guard
# costs two small reductions over a sixteenth of the pixels and one host look at the result per call (0 disables it:
# NQA_AUTO_FLAT_VAR=0).  Natural frames have a pixel variance of 0.02 .. 0.08.
AUTO_FLAT_VAR = float(os.environ.get("NQA_AUTO_FLAT_VAR", "2e-3"))
# The calibration is taken PER FRAME-SIZE CLASS, at the small end of the class: the outliers of the faster modes sit in
# single nearly-dead channels of tap 5, whose statistics run over H/16 x W/16 pixels (64 at 128x128, 8160 at 1080p), so
# what 128x128 frames refuse, 1080p frames may well allow (tools/gpu_size_study.py, tools/gpu_outlier_study.py).
# (first pixel count of the class, ((pairs, height, width, seed), ...)); frames below the first class run in f32s.
AUTO_CLASSES = (
    (128 * 128, ((256, 128, 128, 20261), (128, 160, 192, 20262))),
    (224 * 224, ((320, 256, 256, 20263), (64, 320, 448, 20264))),
    (640 * 640, ((192, 640, 640, 20265), (64, 600, 1000, 20266))),
    (900 * 1000, ((224, 720, 1280, 20267), (32, 1080, 1920, 20268))),
)


def walk_ladder(figures: dict, budget: float = AUTO_F16_BUDGET, rms_budget: float = AUTO_F16_RMS,
                tail_budget: float = AUTO_TAIL, safe_max: float = AUTO_SAFE_MAX):
    """figures = {mode: (max, rms) of mode - f32s over a class's calibration pairs} for every rung but f32s ->
    (choice, {mode: (passes its own test, admitted)}).  Most accurate rung first; a rung is admitted only if it and every
    more accurate one pass: a pass above a failure means the sample happened to miss the faster rung's outliers."""
    choice, chain, flags = "f32s", True, {}
    for prec in reversed(LADDER[:-1]):
        ok = admitted(*figures[prec], budget, rms_budget, tail_budget, safe_max)
        chain = chain and ok
        flags[prec] = (ok, chain)
        if chain:
            choice = prec
    return choice, flags


def size_class(h: int, w: int) -> int:
    """Index of the calibration class of an h x w frame (-1: below AUTO_MIN_PIXELS, always f32s)."""
    k = -1
    for i, (first, _) in enumerate(AUTO_CLASSES):
        if h * w >= first:
            k = i
    return k


# the ladder `auto` climbs, fastest first (two-term stages: f16w all five, f32m4 four, f32m three, f32m2 two)
LADDER = ("f16", "f16w", "f32m4", "f32m", "f32m2", "f32s")


def admitted(mx: float, rms: float, budget: float = AUTO_F16_BUDGET, rms_budget: float = AUTO_F16_RMS,
             tail_budget: float = AUTO_TAIL, safe_max: float = AUTO_SAFE_MAX) -> bool:
    """`auto`'s admission rule for one mode, from the max and rms of its deviation from f32s over the calibration
    pairs: the rms small, and the max either far below the bar or moderately below it with a noise-like tail."""
    if not (mx == mx and rms == rms) or mx == float("inf"):  # NaN / inf: never
        return False
    tail = mx / rms if rms > 0 else 0.0
    return rms <= rms_budget and (mx <= safe_max or (mx <= budget and tail <= tail_budget))


def calibration_pairs(dev, n=128, size=128, seed=20261, width=None):
    """An (x, y) batch `auto` calibrates on, generated on the device from a fixed seed (size x width pixels, square by
    default).  Five pairs of every eight are smooth-plus-noise frames (so that blur changes structure) under the four
    distortion families of SURVEY 8d; three of every eight are NeRF-render-like (round 4): a textured object on an exactly
    constant white or black background covering 40-70 % of the frame, and a smooth frame with a few small floaters --
    the content that produces exactly dead VGG channels, where the faster rungs' outliers live."""
    g = torch.Generator(device=dev).manual_seed(seed)
    h, w = size, (width or size)
    F = torch.nn.functional
    low = F.interpolate(torch.rand(n, 3, max(h // 16, 2), max(w // 16, 2), device=dev, generator=g),
                        size=(h, w), mode="bilinear", align_corners=False)
    x = 0.6 * torch.rand(n, 3, h, w, device=dev, generator=g) + 0.4 * low
    y = torch.empty_like(x)
    noise = torch.randn(n, 3, h, w, device=dev, generator=g)
    other = torch.rand(n, 3, h, w, device=dev, generator=g)
    # object masks / floaters: soft discs from a coarse random field (two thresholds give two slightly different silhouettes)
    field = F.interpolate(torch.rand(n, 1, 5, 5, device=dev, generator=g), size=(h, w), mode="bicubic", align_corners=False)
    par = torch.rand(n, 8, device=dev, generator=g)
    for i in range(n):
        k = i % 8
        if k in (0, 4):
            y[i] = (x[i] + (0.02 if k == 0 else 0.10) * noise[i]).clamp(0, 1)
        elif k == 1:
            y[i] = (x[i] + 0.10 * noise[i]).clamp(0, 1)
        elif k == 2:
            y[i] = F.avg_pool2d(x[i:i + 1], 5, 1, 2, count_include_pad=False)[0]
        elif k == 3:
            y[i] = other[i]
        elif k in (5, 6):  # constant background (white / black), object slightly blurred + noisy, silhouette a little off
            bg = 1.0 if k == 5 else 0.0
            thr = 0.5 + 0.15 * float(par[i, 0])  # roughly 40-70 % background
            m = ((field[i] - thr) * 40.0).clamp(0, 1)
            m2 = ((field[i] - thr - 0.01) * 40.0).clamp(0, 1)
            obj = 0.5 * x[i] + 0.5 * F.avg_pool2d(x[i:i + 1], 5, 1, 2, count_include_pad=False)[0] + 0.03 * noise[i]
            xi = m * x[i] + (1 - m) * bg
            y[i] = (m2 * obj + (1 - m2) * bg).clamp(0, 1)
            x[i] = xi
        else:  # k == 7: a smooth frame (no per-pixel noise) and a render with small floaters
            xi = low[i] * 0.5 + 0.25
            blob = ((field[i] - 0.86) * 60.0).clamp(0, 1)  # a few per cent of the frame
            y[i] = ((1 - blob) * F.avg_pool2d(xi[None], 5, 1, 2, count_include_pad=False)[0] + blob * par[i, 1:4].view(3, 1, 1)).clamp(0, 1)
            x[i] = xi
    return x, y


def cal_cache_path():
    """The calibration file: $NQA_CAL_CACHE (a path; "off" / "0" / "" disables it), default
    ~/.cache/nerf_qa_amd/dists_auto_calibration.json.  One JSON object {key: report}; a key names the VGG weights (by
    content), the device model, the library's source hash, the size class with its calibration sets and the thresholds,
    so a stale entry can never be picked up -- it is simply never looked for again."""
    v = os.environ.get("NQA_CAL_CACHE")
    if v is not None:
        return None if v.lower() in ("", "0", "off", "none") else v
    return os.path.join(os.path.expanduser("~"), ".cache", "nerf_qa_amd", "dists_auto_calibration.json")


def cal_cache_get(key: str):
    path = cal_cache_path()
    if not path:
        return None
    try:
        import json
        with open(path) as f:
            rep = json.load(f).get(key)
        return dict(rep) if isinstance(rep, dict) and rep.get("choice") in LADDER else None
    except (OSError, ValueError):
        return None


def cal_cache_put(key: str, report: dict) -> None:
    """Best effort (a read-only home directory must not break scoring): read-modify-write through a temporary file."""
    path = cal_cache_path()
    if not path:
        return
    try:
        import json
        os.makedirs(os.path.dirname(path), exist_ok=True)
        try:
            with open(path) as f:
                table = json.load(f)
        except (OSError, ValueError):
            table = {}
        table[key] = {k: v for k, v in report.items() if k != "source"}
        tmp = f"{path}.{os.getpid()}.tmp"
        with open(tmp, "w") as f:
            json.dump(table, f)
        os.replace(tmp, path)
    except OSError:
        pass


class L2pooling(nn.Module):
    """Parameter holder with the reference's buffer name/shape (DISTS_pt.py:11-25).

    The arithmetic is nqa_l2pool (HIP); this module exists so `stageN` keeps the same
    children and state_dict keys as the reference's.
    """

    def __init__(self, filter_size=5, stride=2, channels=None, pad_off=0):
        super().__init__()
        self.padding = (filter_size - 2) // 2
        self.stride = stride
        self.channels = channels
        a = np.hanning(filter_size)[1:-1]
        g = torch.Tensor(a[:, None] * a[None, :])
        g = g / torch.sum(g)
        self.register_buffer("filter", g[None, None, :, :].repeat((self.channels, 1, 1, 1)))

    def forward(self, input):
        raise NqaError("L2pooling runs inside the HIP pyramid (DISTS.forward / forward_once); "
                       "calling the stage modules directly is not supported")


def _build_stages(convs):
    """stage1..5 with torchvision's child indices (DISTS_pt.py:36-49)."""
    idx = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
    layers = {}
    for i, (w, b) in zip(idx, convs):
        m = nn.Conv2d(w.shape[1], w.shape[0], kernel_size=3, padding=1)
        m.weight.data = w.clone()
        m.bias.data = b.clone()
        layers[i] = m
        layers[i + 1] = nn.ReLU(inplace=True)
    stages = [nn.Sequential() for _ in range(5)]
    spans = ((0, 4), (5, 9), (10, 16), (17, 23), (24, 30))
    pools = (None, (4, 64), (9, 128), (16, 256), (23, 512))
    for s, (lo, hi) in enumerate(spans):
        if pools[s]:
            stages[s].add_module(str(pools[s][0]), L2pooling(channels=pools[s][1]))
        for i in range(lo, hi):
            stages[s].add_module(str(i), layers[i])
    return stages


class DISTS(torch.nn.Module):
    def __init__(self, load_weights=True, from_feats=False, precision=None, vgg16_path=None, grad_precision=None,
                 target_step=None):
        super().__init__()
        self.grad_precision = resolve_grad_precision(grad_precision)  # (refused before anything is loaded)
        self.target_step = resolve_target_step(target_step)
        convs, self.vgg_source = load_vgg16_convs(vgg16_path)
        self.stage1, self.stage2, self.stage3, self.stage4, self.stage5 = _build_stages(convs)
        for param in self.parameters():
            param.requires_grad = False

        self.register_buffer("mean", torch.tensor([0.485, 0.456, 0.406]).view(1, -1, 1, 1))
        self.register_buffer("std", torch.tensor([0.229, 0.224, 0.225]).view(1, -1, 1, 1))

        self.chns = [3, 64, 128, 256, 512, 512]
        self.register_parameter("alpha", nn.Parameter(torch.randn(1, sum(self.chns), 1, 1)))
        self.register_parameter("beta", nn.Parameter(torch.randn(1, sum(self.chns), 1, 1)))
        self.alpha.data.normal_(0.1, 0.01)
        self.beta.data.normal_(0.1, 0.01)
        if load_weights:
            # the published DISTS alpha/beta (the reference reads them from sys.prefix/weights.pt, :63,79-80)
            ab = np.load(_DATA)
            self.alpha.data = torch.from_numpy(ab["alpha"]).view(1, -1, 1, 1).clone()
            self.beta.data = torch.from_numpy(ab["beta"]).view(1, -1, 1, 1).clone()

        self.precision = precision or os.environ.get("NQA_PRECISION", DEFAULT_PRECISION)
        if self.precision != "auto":
            prec_id(self.precision)  # validate early
        self._packed = {}
        self._ws = ops.Workspace()
        self._guard_streams = {}
        self._auto = None  # (weights key, {size class: report}) once calibrated
        self._deltas = {}  # {size class: {mode: (dS1, dS2)}} similarity deviations, kept for _live_choice only
        self._agreed = {}  # {size class: (weights key, mode)} set by sharding.agree_precision under a process group

    # ---- plumbing -----------------------------------------------------------------
    def _conv_modules(self):
        return [m for st in (self.stage1, self.stage2, self.stage3, self.stage4, self.stage5)
                for m in st if isinstance(m, nn.Conv2d)]

    def _weights_key(self, dev):
        return (str(dev),) + tuple((m.weight._version, m.weight.data_ptr()) for m in self._conv_modules())

    # ---- `auto`: where the verdict comes from ----------------------------------------------
    # memory (self._auto, per weight set / device / size class)  ->  the calibration file (cal_cache_path(): written by
    # whichever process measured first; keyed by the VGG weights' content, the device model, the HIP sources' hash and
    # the thresholds)  ->  a measurement (calibrate()).  Under a process group sharding.agree_precision() has rank 0 do
    # that and broadcasts the report; the agreed choice lives in self._agreed, apart from the calibration cache.
    def precision_for(self, h: int, w: int, device=None) -> str:
        """The precision mode a frame size runs in.  "auto": f32s below AUTO_MIN_PIXELS; above, what the one-time
        calibration of these weights on `device` (default: where alpha lives) allows -- see the module header."""
        if self.precision != "auto":
            return self.precision
        if h * w < AUTO_MIN_PIXELS:
            return "f32s"
        device = torch.device(device if device is not None else self.alpha.device)
        cls = max(size_class(h, w), 0)
        hit = self._agreed.get(cls)
        if hit is not None and hit[0] == self._weights_key(device):
            return hit[1]
        report = self.calibrate(device, h, w)
        live = self._live_weights(device)
        if live is not None:  # alpha / beta are not the published ones: the verdict for THESE weights (see _live_choice)
            return self._live_choice(device, cls, h, w, live)
        return report["choice"]

    def calibrate_all(self, device) -> dict:
        """Calibrate every frame-size class now ({class index: report}): 0.15 + 0.4 + 1.9 + 4.3 s on an MI355X when
        nothing is cached, nothing when the calibration file already holds these weights on this device model and
        library build.  Call it once at start-up to keep the measurement out of the first forward() of each class."""
        return {cls: self.calibrate(device, *AUTO_CLASSES[cls][1][0][1:3]) for cls in range(len(AUTO_CLASSES))}

    def _vgg_digest(self) -> str:
        """sha256 over the thirteen conv layers' weights and biases (content, not identity): the calibration file's key."""
        key = tuple((m.weight._version, m.weight.data_ptr()) for m in self._conv_modules())
        hit = self.__dict__.get("_digest")
        if hit is None or hit[0] != key:
            import hashlib
            hh = hashlib.sha256()
            for m in self._conv_modules():
                hh.update(m.weight.detach().cpu().contiguous().numpy().tobytes())
                hh.update(m.bias.detach().cpu().contiguous().numpy().tobytes())
            hit = self.__dict__["_digest"] = (key, hh.hexdigest()[:32])
        return hit[1]

    def _cal_file_key(self, device, cls, thresholds) -> str:
        try:
            from .. import build as nqa_build
            lib = os.environ.get("NQA_LIB") or nqa_build.source_hash()
        except OSError:  # (sources not shipped beside the library: fall back to the library file itself)
            lib = "lib:%d" % os.path.getsize(os.path.join(os.path.dirname(_DATA), "..", "libnqa_hip.so"))
        devname = torch.cuda.get_device_name(device) if device.type == "cuda" else str(device)
        return "|".join([self._vgg_digest(), devname, str(lib), "class%d" % cls, repr(AUTO_CLASSES[cls]),
                         repr(LADDER), repr(thresholds)])

    @torch.no_grad()
    def calibrate(self, device, h: int = 128, w: int = 128, force: bool = False, keep_deltas: bool = False) -> dict:
        """Measure every faster rung of LADDER against f32s with this module's VGG weights on `device`, for the
        frame-size class of h x w (once per weight set, device model, library build and class: the report is kept in
        memory AND in the calibration file, cal_cache_path()), and decide what `auto` runs frames of that class in: the
        fastest mode whose deviation from f32s stays inside the budgets (module header).  Returns the report {"choice",
        "<mode>": {max_abs_diff, rms_diff, tail, ok} for every rung, "budget", "rms_budget", "tail_budget", "safe_max",
        "pairs", "sizes", "size_class", "source": "measured" | "file"}."""
        device = torch.device(device)
        if device.type != "cuda":
            raise NqaError("precision='auto' calibrates on the GPU: move the module to cuda first "
                           "(or name a precision: 'f32s' holds 1e-4 unconditionally, 'f16' is the fast mode)")
        cls = max(size_class(h, w), 0)
        key = self._weights_key(device)
        if self._auto is None or self._auto[0] != key:
            self._auto = (key, {})
            self._deltas = {}
        if not force and cls in self._auto[1] and not (keep_deltas and cls not in self._deltas):
            return self._auto[1][cls]
        cal_sets = AUTO_CLASSES[cls][1]
        budget = float(os.environ.get("NQA_AUTO_F16_BUDGET", AUTO_F16_BUDGET))
        rms_budget = float(os.environ.get("NQA_AUTO_F16_RMS", AUTO_F16_RMS))
        tail_budget = float(os.environ.get("NQA_AUTO_TAIL", AUTO_TAIL))
        safe_max = float(os.environ.get("NQA_AUTO_SAFE_MAX", AUTO_SAFE_MAX))
        thresholds = (budget, rms_budget, tail_budget, safe_max)
        fkey = self._cal_file_key(device, cls, thresholds)
        if not force and not keep_deltas:
            report = cal_cache_get(fkey)
            if report is not None:
                report["source"] = "file: " + str(cal_cache_path())
                self._auto[1][cls] = report
                return report
        ws = ops.Workspace()  # private scratch (a few GB for 256 pairs of 128x128 in f32s), released again below
        # weighted with the PUBLISHED alpha/beta: the verdict then depends on the VGG weights only; a module whose
        # alpha/beta have been trained away from them gets its own verdict from the kept similarity deltas (_live_choice)
        ab = np.load(_DATA)
        a, b = torch.from_numpy(ab["alpha"]).to(device), torch.from_numpy(ab["beta"]).to(device)
        modes = LADDER[:-1]
        dev_of = {m: [] for m in modes}
        deltas = {m: ([], []) for m in modes}
        npairs = 0
        for n, ch, cw, seed in cal_sets:
            bs = max(1, min(n, (64 * 128 * 128) // (ch * cw) * 4))  # batches of a few hundred MB of frames
            for i0 in range(0, n, bs):
                x, y = calibration_pairs(device, n=min(bs, n - i0), size=ch, seed=seed + 1000 * (i0 // bs), width=cw)
                score, sims = {}, {}
                for prec in modes + ("f32s",):
                    s1, s2 = ops.dists_forward(x, y, self._packed_weights(device, prec), prec, ws)
                    score[prec], sims[prec] = ops.dists_score(s1, s2, a, b), (s1, s2)
                for m in modes:
                    dev_of[m].append((score[m] - score["f32s"]).double())
                    if keep_deltas:
                        deltas[m][0].append(sims[m][0] - sims["f32s"][0])
                        deltas[m][1].append(sims[m][1] - sims["f32s"][1])
                del x, y
            npairs += n
        report = {"budget": budget, "rms_budget": rms_budget, "tail_budget": tail_budget, "safe_max": safe_max, "pairs": npairs,
                  "size_class": cls, "class_from_pixels": AUTO_CLASSES[cls][0],
                  "sizes": [f"{n}x {ch}x{cw}" for n, ch, cw, _ in cal_sets], "source": "measured"}
        figures = {}
        for prec in LADDER[:-1]:
            d = torch.cat(dev_of[prec])
            finite = bool(torch.isfinite(d).all())
            figures[prec] = (float(d.abs().max()), float(d.pow(2).mean().sqrt())) if finite else (float("inf"), float("inf"))
        choice, flags = walk_ladder(figures, budget, rms_budget, tail_budget, safe_max)
        for prec, (mx, rms) in figures.items():
            report[prec] = {"max_abs_diff": mx, "rms_diff": rms, "tail": mx / rms if 0 < rms < float("inf") else 0.0,
                            "ok": flags[prec][0], "admitted": flags[prec][1]}
        report["choice"] = choice
        # (kept for readers of earlier reports: the f16 comparison at top level)
        report["max_abs_diff"], report["rms_diff"] = report["f16"]["max_abs_diff"], report["f16"]["rms_diff"]
        del ws
        self._auto[1][cls] = report
        if keep_deltas:  # (pairs, 1475) per rung and similarity: 27 MB per class at 384 pairs
            self._deltas[cls] = {m: (torch.cat(deltas[m][0]), torch.cat(deltas[m][1])) for m in modes}
        cal_cache_put(fkey, report)
        return report

    # ---- alpha / beta that are not the published ones (fine-tuning: run_nerf_qa.py:454-462) -----------------------
    def _score_weights(self):
        """(alpha / w, beta / w) as this class's forward applies them to S1 / S2, flat float32 (1475,) tensors (the
        `_original` / `_softmax` variants override this with their own parametrisation)."""
        a, b = self.alpha.detach().reshape(-1).float(), self.beta.detach().reshape(-1).float()
        wsum = a.sum() + b.sum()
        return a / wsum, b / wsum

    def _live_weights(self, device):
        """None while alpha/beta still score like the published weights; else the (alpha/w, beta/w) in use.  Checked once
        per change of alpha/beta (their version counters), so an inference module pays for it once."""
        ver = (self.alpha._version, self.beta._version, self.alpha.data_ptr(), self.beta.data_ptr(), type(self).__name__)
        hit = self.__dict__.get("_live")
        if hit is None or hit[0] != ver:
            a, b = self._score_weights()
            ab = np.load(_DATA)
            pa, pb = torch.from_numpy(ab["alpha"]).to(a.device), torch.from_numpy(ab["beta"]).to(a.device)
            pw = pa.sum() + pb.sum()
            same = bool(((a - pa / pw).abs().max() <= 1e-7) & ((b - pb / pw).abs().max() <= 1e-7))
            hit = self.__dict__["_live"] = (ver, None if same else (a.to(device), b.to(device)), {})
        return hit[1]

    @torch.no_grad()
    def _live_choice(self, device, cls, h, w, live) -> str:
        """`auto` for a module whose alpha/beta have moved: the rungs' errors sit in a few nearly dead
        channels, so weights that lean on those channels can push a rung past 1e-4 that the published weights admit.  The
        calibration keeps each rung's similarity deviations (dS1, dS2 per pair and channel); the deviation of the SCORE
        under any alpha/beta is their weighted sum, so the ladder is walked again with the weights in use -- two small
        matrix-vector products per rung whenever alpha/beta change, no new measurement."""
        memo = self.__dict__["_live"][2]
        if cls in memo:
            return memo[cls]
        rep = self.calibrate(device, h, w, keep_deltas=True)
        a, b = live
        figures = {}
        for m, (d1, d2) in self._deltas[cls].items():
            d = -(d1.double() @ a.double() + d2.double() @ b.double())
            ok = bool(torch.isfinite(d).all())
            figures[m] = (float(d.abs().max()), float(d.pow(2).mean().sqrt())) if ok else (float("inf"), float("inf"))
        choice, _ = walk_ladder(figures, rep["budget"], rep["rms_budget"], rep["tail_budget"], rep["safe_max"])
        memo[cls] = choice
        return choice

    def _packed_weights(self, dev, prec=None):
        if prec is None:
            if self.precision == "auto":
                raise NqaError("auto precision depends on the frame size: name the mode (precision_for(h, w, device))")
            prec = self.precision
        key = self._weights_key(dev)
        convs = self._conv_modules()
        hit = self._packed.get(prec)
        if hit is None or hit[0] != key:
            blob = ops.pack_vgg_weights([(m.weight, m.bias) for m in convs], prec)
            hit = self._packed[prec] = (key, blob.to(dev))
        return hit[1]

    def __getstate__(self):  # torch.save(model) (run_nerf_qa.py:502): drop device scratch
        d = self.__dict__.copy()
        d.pop("_packed", None)
        d.pop("_ws", None)  # (__setstate__ rebuilds both)
        d.pop("_guard_streams", None)
        d["_auto"] = None
        for k in ("_deltas", "_agreed"):
            d[k] = {}
        for k in ("_bwd_blobs", "_live", "_digest"):  # device tensors / per-process memos (autograd.py's blobs: 60 MB of
            d.pop(k, None)                            # CUDA tensors that a CPU-only torch.load could not even open)
        return d

    def __setstate__(self, state):
        """Also accepts a module pickled by the REFERENCE's class of this name (loaded through
        nerf_qa_amd.install_alias(); reeval.py:83): its stage1..5 carry the Conv2d weights, the private fields
        of this build are filled in here."""
        super().__setstate__(state)
        d = self.__dict__
        d.setdefault("precision", os.environ.get("NQA_PRECISION", DEFAULT_PRECISION))
        d.setdefault("grad_precision", DEFAULT_GRAD_PRECISION)  # (a module pickled before the keyword existed)
        d.setdefault("target_step", DEFAULT_TARGET_STEP)        # (likewise)
        d.setdefault("vgg_source", "unpickled module (Conv2d weights of stage1..5)")
        d["_packed"], d["_ws"], d["_auto"], d["_deltas"], d["_agreed"] = {}, ops.Workspace(), None, {}, {}
        d["_guard_streams"] = {}

    def _similarities(self, x, y, require_grad=False):
        if x.shape != y.shape:
            raise ValueError(f"x and y differ in shape: {tuple(x.shape)} vs {tuple(y.shape)}")
        if require_grad and torch.is_grad_enabled() and (x.requires_grad or y.requires_grad):
            # DISTS_pt.py:106-108: the pyramids WITH autograd -- here a custom backward through the HIP pyramid
            from ..autograd import DistsSimilarities
            return DistsSimilarities.apply(x, y, self)
        prec = self.precision_for(x.shape[-2], x.shape[-1], x.device)
        if self.precision != "auto" or prec == "f32s" or AUTO_FLAT_VAR <= 0.0:
            return ops.dists_forward(x, y, self._packed_weights(x.device, prec), prec, self._ws)
        # `auto` on a fast rung: nearly FLAT frames are rescored in f32s (see AUTO_FLAT_VAR).  The flatness of the pairs is
        # measured on a SIDE stream (behind an event that says "x and y are ready") and copied to pinned host memory, the
        # fast forward is enqueued on the caller's stream meanwhile, and the host waits for the side stream only: the
        # caller's stream never drains, so the guard costs a few microseconds of host time per call.
        dev = x.device
        if torch.cuda.is_current_stream_capturing():
            raise NqaError("DISTS(precision='auto') on a fast rung looks at the frames on the host (nearly flat frames are "
                           "rescored in f32s) and cannot be captured into a hipGraph: name the precision "
                           f"(precision={prec!r} is what this frame size calibrated to) or set NQA_AUTO_FLAT_VAR=0")
        side = self._guard_streams.get(str(dev))
        if side is None:
            side = self._guard_streams[str(dev)] = torch.cuda.Stream(dev)
        main = torch.cuda.current_stream(dev)
        ready, done = torch.cuda.Event(), torch.cuda.Event()
        ready.record(main)
        flat_host = torch.empty(x.shape[0], dtype=torch.bool, pin_memory=True)
        with torch.no_grad(), torch.cuda.stream(side):
            side.wait_event(ready)
            # (every sixteenth row of both frames, whole rows so that the reduction reads contiguous memory: 1 / 16 of the
            # pixels tells flat from not)
            rows = torch.stack([x[:, :, ::16], y[:, :, ::16]]).float()
            flat = rows.var(dim=(3, 4)).mean(dim=2).amin(dim=0) < AUTO_FLAT_VAR
            flat_host.copy_(flat, non_blocking=True)
            done.record(side)
        s1, s2 = ops.dists_forward(x, y, self._packed_weights(x.device, prec), prec, self._ws)
        done.synchronize()
        idx = flat_host.nonzero().flatten().to(dev)
        if idx.numel():
            e1, e2 = ops.dists_forward(x[idx].contiguous(), y[idx].contiguous(), self._packed_weights(x.device, "f32s"), "f32s",
                                       self._ws)
            s1.index_copy_(0, idx, e1)
            s2.index_copy_(0, idx, e2)
        return s1, s2

    def _weighted(self, s1, s2, batch_average):
        """score from S1,S2; DISTS_pt.py:123-148."""
        if torch.is_grad_enabled() and (self.alpha.requires_grad or self.beta.requires_grad or s1.requires_grad):
            alpha, beta = self.alpha.view(1, -1), self.beta.view(1, -1)
            w_sum = alpha.sum() + beta.sum()
            dist1 = dist2 = 0
            o = 0
            for c in self.chns:
                dist1 = dist1 + ((alpha[:, o:o + c] / w_sum) * s1[:, o:o + c]).sum(1, keepdim=True)
                dist2 = dist2 + ((beta[:, o:o + c] / w_sum) * s2[:, o:o + c]).sum(1, keepdim=True)
                o += c
            score = 1 - (dist1 + dist2).squeeze(1)
        else:
            score = ops.dists_score(s1, s2, self.alpha, self.beta)
        return score.mean() if batch_average else score

    # ---- reference surface ------------------------------------------------------------
    def project_weights(self):
        lower_bound = torch.zeros_like(self.alpha.data)
        lower_bound[:, :3, :, :] = 0.02
        alpha = torch.max(self.alpha.data, lower_bound)
        beta = torch.max(self.beta.data, lower_bound)
        weight_sum = torch.cat([alpha, beta], dim=1).sum()
        self.alpha.data = alpha / weight_sum
        self.beta.data = beta / weight_sum

    def forward_once(self, x):
        prec = self.precision_for(x.shape[-2], x.shape[-1], x.device)
        taps = ops.vgg_pyramid(x, self._packed_weights(x.device, prec), prec, self._ws)
        return [x] + [ops.nhwc_to_nchw_f32(t, ops.tap_prec(prec, k)) for k, t in enumerate(taps)]

    def forward(self, x, y, require_grad=False, batch_average=False, warp=None, certainty=None):
        s1, s2 = self._similarities(x, y, require_grad)
        return self._weighted(s1, s2, batch_average)

    def prepare_target(self, x):
        """The fixed side of a loss, prepared once: x (B,3,H,W) on the GPU -> a target (nerf_qa_amd/target.py) holding x
        as float32 and its five float taps, detached, to be passed to forward_target at every step.  It supports
        .shape, .nbytes, len(), target[i:j] (views) and target.select(indices) (a gathered copy); it belongs to this
        module and to its VGG weights as they are now, and does not pickle.  ValueError for frames that require grad
        (the target takes no gradient), NqaError for tensors off the GPU."""
        from .. import target
        return target.prepare(self, x, "DISTS")

    def forward_target(self, target, y, require_grad=False, batch_average=False):
        """forward(x, y, require_grad, batch_average) for x = a prepared target: the same shapes and return.  With
        require_grad=True and a y that requires grad (grad mode on) a step is ONE kept pyramid of y plus the backward
        chain (autograd.DistsTargetSimilarities) -- nothing of x runs, nothing is computed twice, nothing is read back
        to the host -- and y.grad is forward's own bit for bit.  Otherwise y gives its taps and nothing is kept.  The
        forward always runs in f32s; the backward chain in the module's grad_precision ("f32s", or "f16": half gradient
        maps, the same values).  alpha / beta get their gradients as in forward.  A module built with target_step="c"
        runs that step as the library's two step calls on one state tensor (autograd.DistsTargetStep): the same launches
        and the same bits; the target is used whole, and a state beyond NQA_MAX_WORKSPACE_GB is an NqaError naming
        target[i:j].  ValueError for
        a target of another module, one prepared before the VGG weights changed, and a shape that does not fit;
        NqaError for tensors off the GPU."""
        from .. import autograd, target as tgt
        tgt.check(self, target, y, "DISTS")
        if require_grad and torch.is_grad_enabled() and y.requires_grad:
            step = (autograd.DistsTargetStep if getattr(self, "target_step", DEFAULT_TARGET_STEP) == "c"
                    else autograd.DistsTargetSimilarities)
            s1, s2 = step.apply(y, target, self)
        else:
            s1, s2 = autograd.dists_target_similarities(self, target, y)
        return self._weighted(s1, s2, batch_average)

    def _group_similarities(self, ref, renders):
        """(S1, S2), each (R*K, 1475), of renders (R,K,3,H,W) against ref (R,3,H,W) from one shared pyramid per group."""
        r, k = int(ref.shape[0]), int(renders.shape[1])
        dev = ref.device
        prec = self.precision_for(ref.shape[-2], ref.shape[-1], dev)
        s1, s2 = ops.dists_forward_group(ref, renders, self._packed_weights(dev, prec), prec, self._ws)
        if self.precision != "auto" or prec == "f32s" or AUTO_FLAT_VAR <= 0.0:
            return s1, s2
        # `auto` on a fast rung: the flat-frame guard of _similarities, per pair.  The flatness is measured once per FRAME
        # (R references, R * K renders; every sixteenth row), and a pair is flagged when either of its frames is flat;
        # flagged pairs are rescored through the pairwise f32s forward.  (One host look at R * K flags per call, behind
        # the group forward that is already enqueued.)
        if torch.cuda.is_current_stream_capturing():
            raise NqaError("DISTS(precision='auto') on a fast rung looks at the frames on the host (nearly flat frames are "
                           "rescored in f32s) and cannot be captured into a hipGraph: name the precision "
                           f"(precision={prec!r} is what this frame size calibrated to) or set NQA_AUTO_FLAT_VAR=0")
        flat_ref = ref[:, :, ::16].float().var(dim=(2, 3)).mean(dim=1) < AUTO_FLAT_VAR               # (R,)
        flat_ren = renders[:, :, :, ::16].float().var(dim=(3, 4)).mean(dim=2) < AUTO_FLAT_VAR        # (R, K)
        idx = (flat_ref[:, None] | flat_ren).flatten().nonzero().flatten()
        if idx.numel():
            x = ref[torch.div(idx, k, rounding_mode="floor")].contiguous()
            y = renders.flatten(0, 1)[idx].contiguous()
            e1, e2 = ops.dists_forward(x, y, self._packed_weights(dev, "f32s"), "f32s", self._ws)
            s1.index_copy_(0, idx, e1)
            s2.index_copy_(0, idx, e2)
        return s1, s2

    def forward_group(self, ref, renders, batch_average=False):
        """DISTS of K renders against ONE reference, for R such groups: ref (R,3,H,W), renders (R,K,3,H,W) -> scores
        (R,K), scores[r, k] = forward(ref[r:r+1], renders[r, k:k+1]) (the reference's tables hold several rows per
        reference_folder, test2_prep.py:89,201,304,404).  The reference frames go through the VGG pyramid once per group
        instead of once per render.  Precision: the module's named one, or `auto`'s verdict for the frame size (nearly
        flat pairs rescored in f32s as in forward).  alpha / beta receive gradients as in forward; the images do not:
        ValueError for images that require grad (use forward(require_grad=True) per pair) and for shapes that do not
        fit, NqaError for tensors off the GPU."""
        if not (torch.is_tensor(ref) and torch.is_tensor(renders)) or ref.dim() != 4 or renders.dim() != 5 \
                or ref.shape[1] != 3 or renders.shape[0] != ref.shape[0] or renders.shape[2:] != ref.shape[1:] \
                or ref.numel() == 0 or renders.numel() == 0:
            raise ValueError("forward_group expects references (R,3,H,W) and renders (R,K,3,H,W), got "
                             f"{tuple(getattr(ref, 'shape', ()))} / {tuple(getattr(renders, 'shape', ()))}")
        if torch.is_grad_enabled() and (ref.requires_grad or renders.requires_grad):
            raise ValueError("forward_group does not differentiate through the shared pyramid: detach the images, or call "
                             "forward(x, y, require_grad=True) per pair")
        if not (ref.is_cuda and renders.is_cuda):
            raise NqaError("nerf_qa_amd runs on the GPU only: got tensors on %s / %s (move inputs and the module to cuda; "
                           "there is no CPU fallback)" % (ref.device, renders.device))
        r, k = int(ref.shape[0]), int(renders.shape[1])
        s1, s2 = self._group_similarities(ref, renders)
        score = self._weighted(s1, s2, False).reshape(r, k)
        return score.mean() if batch_average else score

    def forward_from_feats(self, feats0, feats1, batch_average=False):
        if torch.is_grad_enabled() and any(f.requires_grad for f in list(feats0) + list(feats1)):
            # the NR models' training loss (model_nr_v8.py:258-265): the same statistics kernel, with a HIP backward
            # onto the maps (nerf_qa_amd/autograd.py); the weighted sum stays torch so alpha and beta get theirs too
            if len(feats0) != 6 or len(feats1) != 6:
                raise ValueError("expected six feature maps per image")
            from ..autograd import FeatsSimilarities
            s1, s2 = FeatsSimilarities.apply(*feats0, *feats1)
            return self._weighted(s1, s2, batch_average)
        s1, s2 = ops.dists_stats_nchw(feats0, feats1)
        return self._weighted(s1, s2, batch_average)


def prepare_image(image, resize=True, keep_aspect_ratio=False):
    """PIL image -> float32 (1,3,H,W) in [0,1]; DISTS_pt.py:210-217 without torchvision.

    torchvision's resize of a PIL image is PIL's own antialiased bilinear `Image.resize`;
    `resize(image, 256)` scales the short side to 256 keeping the aspect ratio.
    """
    from PIL import Image
    if resize and min(image.size) > 256:
        if keep_aspect_ratio:
            w, h = image.size
            if w <= h:
                nw, nh = 256, int(256 * h / w)
            else:
                nh, nw = 256, int(256 * w / h)
            image = image.resize((nw, nh), Image.BILINEAR)
        else:
            image = image.resize((256, 256), Image.BILINEAR)
    arr = np.array(image.convert("RGB"), dtype=np.uint8)
    return torch.from_numpy(arr).permute(2, 0, 1).float().div(255).unsqueeze(0)
