"""CPU side of tests/test_gpu_conv_split_exact.py and tests/test_gpu_conv_float_exact.py: operands on which the f32s
convolutions of nqa_conv.hip -- three MFMAs per product on (hi, lo) half pairs of weights and activations,
al*bh + ah*bl + ah*bh, no lo*lo -- must be BIT-EQUAL to a float64 restatement of that arithmetic, and a mirror of the
gates by which launch_conv picks a kernel instance.  No GPU needed: tests/test_split_refs.py checks everything here.

(a) Operand sets.  An activation is Ah + Al and a weight Wh + Wl such that the device encode (hi = half(v),
    lo = half(v - hi); store_split4 for activations, nqa_pack_vgg_weights / nqa_pack_conv_split for weights times the
    layer's power-of-two scale) gives back exactly (Ah, Al) and (s Wh, s Wl):
      "normal"  Ah in {0, 1, 2},        Al in {-1, 0, 1} 2^-13 where Ah > 0   (lo a normal half)
      "small"   Ah in {0, 2^-6, 2^-5},  Al in {-1, 0, 1} 2^-19 where Ah > 0   (lo a SUBNORMAL half: 32 units of 2^-24)
      weights   at most 400 non-zeros per output channel, Wh = +-1, Wl in {-1, 0, 1} 2^-13 with a sign of its own;
                the largest |w| is 1 + 2^-13, so weight_scale_exp gives s = 512: s Wh = +-512, s Wl = +-2^-4
      bias      integers in -3 .. 3 (VGG layers); nqa_pack_conv_split has none
    The signed sets put a random sign on the activations (the data-gradient convolutions, relu=False).
    Every product of the three terms is a multiple of the set's quantum q (2^-13 / 2^-19, times s in the accumulator), and
    sum |terms| + |bias| stays below q 2^24 (2048 / 32), so every partial sum in ANY order -- and in LOACC's two
    accumulators -- is a float32 number: the kernel has nothing to round.
(b) The reference: conv(s Wh, Ah) + conv(s Wh, Al) + conv(s Wl, Ah) in float64 on the encode model's halves, times 1/s,
    plus the bias, ReLU or not; rounded once to float32 (exact), or to the two halves of a split16 record.
(c) instance(): launch_conv's and conv3x3_split_generic's choices restated (narrow, big with eff_big / eff_small and
    blocks_big, wide, the forced plain / mixed grid), to assert in a test which kernel instance its shape reaches.  Never a
    reference for values.
(d) The dense integer operands of tests/persistent_refs.py (int_convs, int_base, conv_ref, round_to) extended to
    conv4_1 and conv4_2, for the f32 / bf16 / wide-tile cases."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

import persistent_refs as P

SETS = {"normal": dict(hi=(1.0, 2.0), q=2.0 ** -13, bound=2048.0), "small": dict(hi=(2.0 ** -6, 2.0 ** -5), q=2.0 ** -19, bound=32.0)}
WEIGHT_TERMS = 400
WQ = 2.0 ** -13
SCALE = 512.0
SPLIT_LAYERS = (1, 2, 7, 8, 9)            # conv1_2, conv2_1, conv4_1, conv4_2, conv4_3
GRAD_SHAPES = ((128, 128), (512, 256), (512, 512), (64, 64), (128, 64))  # (Cin, Cout) of the data-gradient convolutions
MIN_SUBNORMAL_HALF, MIN_NORMAL_HALF = 2.0 ** -24, 2.0 ** -14


# ---- (a) operands ---------------------------------------------------------------------------------------------------------
def weight_scale_exp(w: np.ndarray) -> int:
    """nqa_weights.hip weight_scale_exp: the power of two that puts the largest |w| in [512, 1024)."""
    wmax = float(np.abs(w).max())
    if not (wmax > 0.0 and math.isfinite(wmax)):
        return 0
    return max(-8, min(24, math.floor(math.log2(1024.0 / wmax))))


def encode_model(v64: torch.Tensor):
    """The device encode in float64: hi = half(v), lo = half(v - hi), both rounded to nearest even by torch's CPU
    conversion (which keeps subnormals); v must be a float32 number, v - hi is then exact in float32."""
    v32 = v64.to(torch.float32)
    assert torch.equal(v32.double(), v64)
    hi = v32.half()
    lo = (v32 - hi.float()).half()
    return hi.double(), lo.double()


@functools.lru_cache(maxsize=None)
def split_weights(cin: int, cout: int, seed: int):
    """(w float32 OIHW = Wh + Wl, Wh float64, Wl float64): WEIGHT_TERMS non-zeros per output channel at the positions of
    the smallest draws of its row (as persistent_refs.sparse_convs), Wh and Wl signed independently."""
    from nerf_qa_amd import synth
    k = cin * 9
    u = synth.uniform(seed, cout * k).reshape(cout, k)
    sh = np.where(synth.uniform(seed, cout * k, 1).reshape(cout, k) < 0.5, -1.0, 1.0)
    sl = (np.floor(synth.uniform(seed, cout * k, 2) * 3.0).clip(0, 2) - 1.0).reshape(cout, k) * WQ
    pick = np.argsort(u, axis=1)[:, :WEIGHT_TERMS]
    wh, wl = np.zeros((cout, k)), np.zeros((cout, k))
    np.put_along_axis(wh, pick, np.take_along_axis(sh, pick, axis=1), axis=1)
    np.put_along_axis(wl, pick, np.take_along_axis(sl, pick, axis=1), axis=1)
    wh, wl = (t.reshape(cout, cin, 3, 3) for t in (wh, wl))  # k = (cin, ky, kx): OIHW
    w = (wh + wl).astype(np.float32)
    assert np.array_equal(w.astype(np.float64), wh + wl)
    return w, torch.from_numpy(wh), torch.from_numpy(wl)


@functools.lru_cache(maxsize=None)
def split_convs():
    """The synthetic VGG weights with SPLIT_LAYERS replaced by split_weights and a bias in {-3 .. 3}."""
    from nerf_qa_amd import ops, synth
    convs = list(synth.vgg16_weights(1234))
    for layer in SPLIT_LAYERS:
        cout = ops.CONV_COUT[layer]
        b = np.floor(synth.uniform(2950 + layer, cout) * 7.0).clip(0, 6).astype(np.float32) - 3.0
        convs[layer] = (split_weights(ops.CONV_CIN[layer], cout, 2900 + layer)[0], b)
    return convs


def weights_of(wkey):
    """wkey = ("vgg", layer) | ("grad", Cin, Cout) -> (w float32 OIHW, Wh, Wl, bias float64 (Cout,)).  The data-gradient
    convolutions have weight tensors of their own, not slices of the VGG layers'."""
    if wkey[0] == "vgg":
        from nerf_qa_amd import ops
        layer = wkey[1]
        w, wh, wl = split_weights(ops.CONV_CIN[layer], ops.CONV_COUT[layer], 2900 + layer)
        return w, wh, wl, torch.from_numpy(split_convs()[layer][1]).double()
    _, cin, cout = wkey
    w, wh, wl = split_weights(cin, cout, 3100 + cin + 7 * cout)
    return w, wh, wl, torch.zeros(cout, dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def split_acts(name: str, cin: int, h: int, w: int, nb: int, signed: bool = False):
    """(a float32 NHWC (nb, h, w, cin) = Ah + Al, Ah float64, Al float64) of operand set `name`.  Never modified."""
    from nerf_qa_amd import synth
    s = SETS[name]
    seed = 3300 + (1 if name == "small" else 0) + 2 * cin + 7 * h + w + (100000 if signed else 0)
    n = nb * h * w * cin
    lvl = np.floor(synth.uniform(seed, n) * 3.0).clip(0, 2).astype(np.int64)
    ah = np.array([0.0, s["hi"][0], s["hi"][1]])[lvl]
    al = np.where(ah > 0, (np.floor(synth.uniform(seed, n, 1) * 3.0).clip(0, 2) - 1.0) * s["q"], 0.0)
    if signed:  # (+ 0.0: a zero keeps its +0, as the device's v - hi = +0 does)
        sign = np.where(synth.uniform(seed, n, 2) < 0.5, -1.0, 1.0)
        ah, al = np.where(ah > 0, sign * ah, 0.0), np.where(ah > 0, sign * al, 0.0) + 0.0
        assert not np.signbit(ah[ah == 0]).any() and not np.signbit(al[al == 0]).any()
    a = (ah + al).astype(np.float32)
    assert np.array_equal(a.astype(np.float64), ah + al)
    shape = (nb, h, w, cin)
    return torch.from_numpy(a.reshape(shape)), torch.from_numpy(ah.reshape(shape)), torch.from_numpy(al.reshape(shape))


# ---- (b) the reference ------------------------------------------------------------------------------------------------------
def _conv64(a_nhwc: torch.Tensor, w_oihw: torch.Tensor) -> torch.Tensor:
    """3 x 3, zero pad 1, float64, NHWC in and out."""
    return F.conv2d(a_nhwc.permute(0, 3, 1, 2), w_oihw, None, padding=1).permute(0, 2, 3, 1).contiguous()


def _halves(wkey, name, h, w, nb, signed):
    """The encode model's halves of the case's operands, asserted to be the intended ones; the weights' times SCALE."""
    w32, wh, wl, bias = weights_of(wkey)
    a32, ah, al = split_acts(name, w32.shape[1], h, w, nb, signed)
    k = weight_scale_exp(w32)
    assert 2.0 ** k == SCALE, f"weight_scale_exp gives 2^{k}, not {SCALE}"
    wh_m, wl_m = encode_model(torch.from_numpy(w32).double() * SCALE)
    ah_m, al_m = encode_model(a32.double())
    assert torch.equal(wh_m, wh * SCALE) and torch.equal(wl_m, wl * SCALE), "the weights' encode is not (s Wh, s Wl)"
    assert torch.equal(ah_m, ah) and torch.equal(al_m, al), "the activations' encode is not (Ah, Al)"
    return wh_m, wl_m, ah_m, al_m, bias


@functools.lru_cache(maxsize=None)
def pre_activation(wkey, name: str, h: int, w: int, nb: int, signed: bool = False) -> torch.Tensor:
    """(conv(s Wh, Ah) + conv(s Wh, Al) + conv(s Wl, Ah)) / s + bias in float64, NHWC (nb, h, w, Cout).  (The first two
    terms are one convolution with Ah + Al: every sum here is exact in float64, see analysis.)"""
    wh, wl, ah, al, bias = _halves(wkey, name, h, w, nb, signed)
    return (_conv64(ah + al, wh) + _conv64(ah, wl)) / SCALE + bias


def reference(wkey, name: str, h: int, w: int, nb: int, signed: bool = False, relu: bool = True) -> torch.Tensor:
    """The kernel's float output, float32 NHWC: exact, asserted.  (+ 0.0: a float64 sum of -0 terms is no -0 on the device,
    whose accumulators start at +0.)"""
    pre = pre_activation(wkey, name, h, w, nb, signed)
    v = (F.relu(pre) if relu else pre) + 0.0
    out = v.to(torch.float32)
    assert torch.equal(out.double(), v)
    return out


def records(v32: torch.Tensor):
    """The two halves (hi, lo) of the split16 records of a float32 map: hi = half(v), lo = half(v - hi)."""
    hi = v32.half()
    return hi, (v32 - hi.float()).half()


def record_halves(rec: torch.Tensor):
    """(hi, lo) half tensors (..., C) of split16 records held in a float32-typed tensor (..., C): per pixel and group of
    16 channels 64 bytes [hi 0-7 | hi 8-15 | lo 0-7 | lo 8-15] (include/nqa.h, Layouts)."""
    c = rec.shape[-1]
    r = rec.contiguous().view(torch.float16).reshape(*rec.shape[:-1], c // 16, 2, 16)
    return r[..., 0, :].reshape(rec.shape), r[..., 1, :].reshape(rec.shape)


def analysis(wkey, name: str, h: int, w: int, nb: int, signed: bool = False) -> dict:
    """The four products apart, with the conditions of (a) asserted, and what the mutants and the four-term product give:
    shares of the pre-activations whose float32 value differs from the reference's."""
    s = SETS[name]
    wh, wl, ah, al, bias = _halves(wkey, name, h, w, nb, signed)
    hh, hl, lh, ll = _conv64(ah, wh), _conv64(al, wh), _conv64(ah, wl), _conv64(al, wl)
    pre = pre_activation(wkey, name, h, w, nb, signed)
    assert torch.equal((hh + hl + lh) / SCALE + bias, pre)
    mag = float(((_conv64(ah.abs() + al.abs(), wh.abs()) + _conv64(ah.abs(), wl.abs())) / SCALE + bias.abs()).max())
    assert mag < s["bound"], f"sum |terms| + |bias| = {mag} is not below {s['bound']}"
    for t in (hh, hl, lh):  # every product, hence every partial sum, is a multiple of the quantum
        assert torch.equal(torch.round(t / (SCALE * s["q"])) * (SCALE * s["q"]), t)
    assert torch.equal(torch.round(pre / s["q"]) * s["q"], pre)
    ref = pre.to(torch.float32)
    assert torch.equal(ref.double(), pre)
    nz = al != 0
    sub = float(((al.abs() < MIN_NORMAL_HALF) & nz).sum()) / max(1.0, float((ah != 0).sum()))
    assert not nz.any() or float(al[nz].abs().min()) >= MIN_SUBNORMAL_HALF

    def share(terms):
        return float(((terms / SCALE + bias).to(torch.float32) != ref).double().mean())
    return dict(bound=mag, largest=float(pre.abs().max()), subnormal_lo=sub, positive=float((pre > 0).double().mean()),
                mutants={"hi*hi only": share(hh), "Wl*Ah dropped": share(hh + hl), "Wh*Al doubled": share(hh + 2 * hl + lh),
                         "operands swapped (al*bl + ah*bh)": share(hh + ll)},
                four_term=share(hh + hl + lh + ll))


def weight_coverage(wkey) -> dict:
    """Where the non-zero weights sit: kernel positions and 16-channel input chunks hit per output channel (the fewest over
    the channels), and the share of all (input channel, position) pairs some output channel of each 64-channel slab hits."""
    _, wh, wl, _ = weights_of(wkey)
    nz = wh != 0
    cout, cin = nz.shape[:2]
    taps = nz.reshape(cout, cin, 9).any(1).sum(1)
    chunks = nz.reshape(cout, cin // 16, 16 * 9).any(2).sum(1)
    slab = nz.reshape(cout // 64, 64, cin * 9).any(1)
    opposite = float(((wh * wl) < 0).sum()) / float((wl != 0).sum())
    return dict(per_channel=int(nz.reshape(cout, -1).sum(1).max()), taps=int(taps.min()), chunks=int(chunks.min()),
                of_chunks=cin // 16, slab_positions=float(slab.double().mean()), opposite_signs=opposite)


# ---- (c) launch_conv's gates --------------------------------------------------------------------------------------------------
def instance(cout: int, n: int, h: int, w: int, variant: int = 1, edge: int = 0, split: bool = False, cus: int = 256) -> dict:
    """The implicit-GEMM instance launch_conv gives a layer that no register-weights kernel takes: tile = its <WAVES_N,
    WAVES_M, WN_T, WM_T>, tw = its width, mixed = conv3x3_igemm_mixed_kernel.  variant: the conv variant's low two bits;
    edge: 0 (use_mixed_grid counts rounds of cus x blocks per CU), 256 (plain), 512 (mixed); split: f32s (no wide tile)."""
    cdiv = P.cdiv
    narrow = w <= 16
    big = variant >= 1 and cout >= 256 and not narrow
    eff_big = h * w / (cdiv(w, 32) * cdiv(h, 8) * 256.0)
    eff_small = h * w / (cdiv(w, 32) * cdiv(h, 4) * 128.0)
    blocks_big = cdiv(w, 32) * cdiv(h, 8) * n * (cout // 256)
    if big:
        big = eff_big * 1.05 >= eff_small and blocks_big >= 192
    out = dict(narrow=narrow, big=big, eff_big=eff_big, eff_small=eff_small, blocks_big=blocks_big, tw=16 if narrow else 32)
    if cout == 64:
        return dict(out, tile="<1,4,2,2>", mixed=False)
    eff_wide = h * w / (cdiv(w, 32) * cdiv(h, 16) * 512.0)
    if not split and variant >= 2 and cout >= 128 and not narrow and h >= 12 and eff_wide * 1.10 >= eff_small:
        return dict(out, tile="<2,4,2,4>", mixed=False, eff_wide=eff_wide)
    mixed = not narrow and edge != 256 and 1 <= w % 32 <= 16 and w >= 32
    if mixed and edge != 512:  # use_mixed_grid: taken where it needs fewer rounds
        mp, slots, per = (256, cus, n * (cout // 256)) if big else (128, 2 * cus, n * (cout // 128))
        plain = cdiv(w, 32) * cdiv(h, mp // 32) * per
        mix = ((w // 32) * cdiv(h, mp // 32) + cdiv(h, mp // 16)) * per
        mixed = cdiv(mix, slots) < cdiv(plain, slots)
    return dict(out, tile="<2,4,4,2>" if big else "<2,2,2,2>", mixed=mixed, eff_wide=eff_wide)


# ---- the cases of the GPU files ------------------------------------------------------------------------------------------------
# f32s on split operands: (layer, n, H, W), variant bits added to the default, the kernel, its tile width, mixed grids.
# Wherever 1 <= W % 32 <= 16 the grid is forced (+ 256 plain, + 512 mixed): left to use_mixed_grid it would depend on the
# device's CU count.
VGG_CASES = [((1, 2, 9, 40), 0, "<1,4,2,2>", 32, 0), ((1, 2, 5, 13), 0, "<1,4,2,2>", 16, 0),
             ((2, 2, 9, 40), 0, "regw_split", 32, 0), ((2, 2, 9, 40), 16 + 256, "<2,2,2,2>", 32, 0), ((2, 2, 7, 13), 0, "<2,2,2,2>", 16, 0),
             ((8, 2, 13, 80), 256, "<2,2,2,2>", 32, 0), ((8, 2, 13, 80), 512, "<2,2,2,2>", 32, 1), ((9, 2, 11, 13), 0, "<2,2,2,2>", 16, 0),
             ((7, 20, 24, 64), 0, "<2,4,4,2>", 32, 0), ((7, 20, 23, 40), 256, "<2,4,4,2>", 32, 0), ((7, 20, 24, 48), 512, "<2,4,4,2>", 32, 1)]
GRAD_MAPS = ((6, 21), (3, 13))  # n = 2; 32-wide and 16-wide LOACC instances
# integer operands in f32: the same columns
F32_CASES = [((1, 2, 9, 40), 0, "<1,4,2,2>", 32, 0), ((1, 2, 5, 13), 0, "<1,4,2,2>", 16, 0),
             ((3, 2, 9, 48), 256, "<2,2,2,2>", 32, 0), ((3, 2, 9, 48), 512, "<2,2,2,2>", 32, 1), ((8, 2, 13, 80), 256, "<2,2,2,2>", 32, 0),
             ((7, 2, 11, 13), 0, "<2,2,2,2>", 16, 0),
             ((7, 20, 24, 64), 0, "<2,4,4,2>", 32, 0), ((7, 20, 23, 40), 256, "<2,4,4,2>", 32, 0), ((7, 20, 24, 48), 512, "<2,4,4,2>", 32, 1)]
WIDE_CASES = [(3, 2, 16, 64), (3, 2, 29, 40), (7, 2, 32, 64)]  # conv variant 2: the 128 ch x 512 px tile <2,4,2,4>


def vgg_instance(layer: int, n: int, h: int, w: int, extra: int, split: bool, cus: int = 256):
    """(kernel, tile width, mixed grids) of one ops.conv3x3_relu call in f32s (split) or f32 under DEFAULT | extra --
    launch_conv read top to bottom: conv2_1 in f32s goes to conv3x3_regw_split_kernel unless + 16 (the first forms) or W < 16."""
    from nerf_qa_amd import ops
    if split and layer == 2 and not extra & 16 and w >= 16 and h >= 2:
        return "regw_split", 32, 0
    i = instance(ops.CONV_COUT[layer], n, h, w, 1, extra & 768, split, cus)
    return i["tile"], i["tw"], int(i["mixed"])


# ---- (d) dense integer operands ----------------------------------------------------------------------------------------------
int_convs, int_base, conv_ref, round_to, partial_sum_bound, batch_of = (P.int_convs, P.int_base, P.conv_ref, P.round_to,
                                                                        P.partial_sum_bound, P.batch_of)
