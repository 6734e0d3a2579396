"""CPU references of single layers of the mixed modes (f16 activations x two-term f16 weights): the float64 value of a
layer, the magnitude sum its rounding error scales with, and a float32 replay of the kernels' arithmetic whose own
distance from the float64 value is where the bars of tests/test_gpu_mixed_layers.py come from.  No GPU needed:
tests/test_mixed_refs.py recomputes every figure quoted there and shows that the checks catch a lost `lo` term."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

EPS24 = 2.0 ** -24

# (layer, n, H, W): ragged in both directions, maps below one tile, every tile form of the two-term kernels
CONV_CASES = [(1, 2, 13, 37), (2, 2, 11, 40), (3, 1, 8, 33), (3, 1, 24, 40), (4, 1, 7, 7), (5, 2, 9, 33), (6, 2, 12, 35),
              (8, 1, 8, 17), (9, 2, 9, 20), (10, 1, 5, 6), (12, 3, 4, 16), (12, 1, 1, 1)]
# the smallest map on which nqa_set_conv_variant 0 and 1 run different two-term kernels: an implicit-GEMM layer (5 = conv3_2)
# with >= 256 output channels, W > 16
# and 192 blocks of the 8-wave 256 ch x (8 x 32) px tile whose grid wastes no more than the 4-wave one's (13 rows = 2 | 4
# tile rows of 16 rows either way; 33 columns = 2 tile columns)
BIG_CASE = (5, 48, 13, 33)
STAGE1_SHAPES = [(2, 3, 37, 53), (1, 3, 16, 16), (3, 3, 5, 70), (2, 3, 1, 1)]
FUSED_SHAPES = [(1, 3, 16, 16), (2, 3, 9, 33), (3, 3, 37, 70), (1, 3, 64, 100)]
POOL_SHAPES = [(2, 9, 13, 256), (1, 1, 5, 256), (1, 7, 2, 512), (2, 16, 16, 128)]
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def to_half(t: torch.Tensor) -> torch.Tensor:
    """Round to IEEE half in ONE step from whatever precision t has (numpy converts float64 -> float16 directly; a
    detour through float32 would round twice), returned as float64."""
    return torch.from_numpy(t.detach().cpu().numpy().astype(np.float16).astype(np.float64))


@functools.lru_cache(maxsize=None)
def convs():
    from nerf_qa_amd import synth
    return [(torch.from_numpy(w), torch.from_numpy(b)) for w, b in synth.vgg16_weights(1234)]


def uniform(shape, seed, lo=0.0, hi=1.0) -> torch.Tensor:
    from nerf_qa_amd import synth
    n = int(np.prod(shape))
    return torch.from_numpy((synth.uniform(seed, n) * (hi - lo) + lo).astype(np.float32).reshape(shape))


def relu_like_input(layer, n, h, w) -> torch.Tensor:
    """Post-ReLU-like half NHWC input of conv `layer`: half zeros, the rest in [0, 2) (as tests/test_gpu_ops.py)."""
    from nerf_qa_amd import ops
    return uniform((n, h, w, ops.CONV_CIN[layer]), 100 + layer, -2.0, 2.0).clamp_min(0).half()


def split_terms(w32: torch.Tensor, scaled: bool = False):
    """(hi, lo, 1/s): the two f16 terms of float32 weights as float32 tensors.  scaled: times the power of two that puts
    the layer's largest |w| in [512, 1024), as nqa_pack_vgg_weights stores them (lo is then a normal half)."""
    s = 1.0
    if scaled:
        s = 2.0 ** np.floor(np.log2(1024.0 / float(w32.abs().max())))
    ws = w32 * s  # (exact: a power of two)
    hi = ws.half().float()
    lo = (ws - hi).half().float()
    return hi, lo, 1.0 / s


def conv_layer_ref(a16_nhwc: torch.Tensor, w32: torch.Tensor, b32: torch.Tensor, drop_lo=None):
    """One conv + bias of exact half inputs.  Returns float64 NCHW (pre, mag) -- the convolution with the UNROUNDED
    float32 weights and sum |a||w| + |b| -- and the float32 replay `acc` of the two-term arithmetic:
    conv2d(a, hi) + conv2d(a, lo) + b in float32.  drop_lo: None | "all" | (ky, kx): the replay of a FAULTY kernel that
    loses the lo term everywhere | in one of the nine taps (what the checks must catch)."""
    a = a16_nhwc.permute(0, 3, 1, 2).double()
    w, b = w32.double(), b32.double()
    pre = F.conv2d(a, w, b, padding=1)
    mag = F.conv2d(a.abs(), w.abs(), None, padding=1) + b.abs().view(1, -1, 1, 1)
    hi, lo, _ = split_terms(w32)
    if drop_lo == "all":
        lo = torch.zeros_like(lo)
    elif drop_lo is not None:
        lo = lo.clone()
        lo[:, :, drop_lo[0], drop_lo[1]] = 0
    a32 = a.float()
    acc = F.conv2d(a32, hi, None, padding=1) + F.conv2d(a32, lo, None, padding=1) + b32.view(1, -1, 1, 1)
    return pre, mag, acc


def half_envelope(pre, mag, c, relu=True):
    """[f16(relu(pre - tau)), f16(relu(pre + tau))], tau = c 2^-24 mag, as float64: rounding to half is monotone, so a
    value within tau of `pre` before the ReLU and the store lies in it, tiny outputs of cancelling sums included."""
    tau = c * EPS24 * mag
    lo, hi = pre - tau, pre + tau
    if relu:
        lo, hi = lo.clamp_min(0), hi.clamp_min(0)
    return to_half(lo), to_half(hi)


def replay_constant(pre, mag, acc) -> float:
    """max |acc - pre| / (2^-24 mag) of a float32 replay."""
    return float(((acc.double() - pre).abs() / (EPS24 * mag)).max())


def share_differing(got_half_f64, pre, relu=True) -> float:
    """Share of elements that differ at all from f16(relu(pre))."""
    want = to_half(pre.clamp_min(0) if relu else pre)
    return float((got_half_f64 != want).double().mean())


# ---- stage 1 --------------------------------------------------------------------------------------------------------
def image(shape, seed=11) -> torch.Tensor:
    return uniform(shape, seed)


def conv1_1_ref(x32: torch.Tensor):
    """The mixed conv1_1 (an exact float conv of the normalised pixels, half store): float64 (pre, mag) with the
    normalisation (x - mean) / std in float64, and the float32 replay of the same."""
    w32, b32 = convs()[0]
    mean, std = torch.tensor(MEAN, dtype=torch.float64).view(1, 3, 1, 1), torch.tensor(STD, dtype=torch.float64).view(1, 3, 1, 1)
    h = (x32.double() - mean) / std
    pre = F.conv2d(h, w32.double(), b32.double(), padding=1)
    mag = F.conv2d(h.abs(), w32.double().abs(), None, padding=1) + b32.double().abs().view(1, -1, 1, 1)
    h32 = (x32 - mean.float()) / std.float()
    acc = F.conv2d(h32, w32, b32, padding=1)
    return pre, mag, acc


def fused_stage1_ref(x32: torch.Tensor, dtype, drop_lo=()):
    """The fused mixed stage 1 with the kernel's rounding points (conv1_regw_kernel<.., 2>): the normalised pixels are
    rounded to half, relu1_1 is rounded to half, relu1_2 is stored as half; both convolutions on two-term weights with
    float accumulation.  dtype float64: unrounded float32 weights, everything else in float64; float32: the (hi, lo)
    terms and float32 arithmetic; drop_lo: the convolutions (0, 1) of a FAULTY float32 replay that lose their lo term.
    Returns relu1_2 before its half store, NCHW."""
    (w0, b0), (w1, b1) = convs()[0], convs()[1]
    mean, std = torch.tensor(MEAN, dtype=dtype).view(1, 3, 1, 1), torch.tensor(STD, dtype=dtype).view(1, 3, 1, 1)
    h = to_half((x32.to(dtype) - mean) / std).to(dtype)

    def conv(a, w32, b32, which):
        if dtype == torch.float64:
            return F.conv2d(a, w32.double(), b32.double(), padding=1)
        hi, lo, _ = split_terms(w32)
        if which in drop_lo:
            lo = torch.zeros_like(lo)
        return F.conv2d(a, hi, None, padding=1) + F.conv2d(a, lo, None, padding=1) + b32.view(1, -1, 1, 1)
    r11 = to_half(conv(h, w0, b0, 0).clamp_min(0)).to(dtype)
    return conv(r11, w1, b1, 1).clamp_min(0)


def share_of_halves_differing(got, ref64) -> float:
    """Share of elements of `got` (already half values) that differ at all from f16(ref64)."""
    return float((got.double() != to_half(ref64)).double().mean())


# ---- the boundary pool ----------------------------------------------------------------------------------------------
def pool_input(n, h, w, c) -> torch.Tensor:
    """Half NHWC tap in [0, 3) with channel 3 at 0 and channel 5 at 2^-15 (pooled values far below 2^-14)."""
    a = uniform((n, h, w, c), 7, 0.0, 3.0).half()
    a[..., 3] = 0.0
    a[..., 5] = 2.0 ** -15
    return a


def pool_refs(a16_nhwc: torch.Tensor):
    """(float64 oracle, float32 oracle) of the L2-pool of the same half values, NCHW."""
    from oracle import dists_oracle
    a = a16_nhwc.permute(0, 3, 1, 2)
    return dists_oracle.l2pool(a.double()), dists_oracle.l2pool(a.float())


def rel_to_max(got, ref) -> float:
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max())
