"""CPU side of tests/test_gpu_stage1_split_exact.py: raw frames and weights on which the f32s fused stage 1
(conv1_regw_split_kernel of nqa_conv.hip: normalisation in float split into (hi, lo) halves, conv1_1 on the MFMA as three
products w_hi*a_hi + w_lo*a_hi + w_hi*a_lo, relu1_1 re-split into halves in LDS, conv1_2 the same three products) must be
BIT-EQUAL to a float64 restatement of that arithmetic.  No GPU needed, nothing of nerf_qa_amd in the arithmetic (only its
deterministic draws, synth.uniform): tests/test_stage1_split_refs.py checks everything here.

(a) The pixel table.  The kernel normalises with fl(fl(raw - kMean[c]) / kStd[c]) in float32 (literals of csrc/nqa_regw.h,
    mirrored by persistent_refs.S1_MEAN / S1_STD).  pixel_table() replays that expression in numpy float32 on the few
    float32 numbers around float32(mean + std t) for every target t = hi + b q, q = 2^-13, hi a multiple of 1/2 in the
    normalised range of [0, 1] pixels, b in -3 .. 3, and keeps a raw pixel where the replay gives t EXACTLY and the device
    encode (hi = half(v), lo = half(v - hi)) gives back (hi, b q).  v = 0 is raw = mean itself.  (No tiny |v| other than 0
    is reachable: hi = 0 has b = 0 only.)  The one assumption -- that the device evaluates the expression as correctly
    rounded float32 -- has a GPU test of its own (test_the_device_normalises_as_the_replay_does).
(b) Frames draw from the table's levels -1 + b q and 2 + b q with |b| <= 1, and 0.
(c) conv1_1: one or two taps per output channel, Wh = +-1, Wl in {-1, 0, 1} q signed on its own, an integer bias chosen
    per sign pattern (C11_TYPES) so that over every combination of tap values in {-1, 0, 2} (0 is also what the zero
    padding gives) the integer part A of the pre-activation is <= -1 (dead), 0 with no lo term at all (a lone tap on a zero
    pixel), or >= 2 with the lo terms eps = sum Wh vl + Wl vh below half a half-ulp of A: relu1_1 is exactly 0 or A + eps
    and its re-split is (A, eps), a "normal"-type operand of tests/split_refs.py for conv1_2.  Every (channel, ky, kx) of
    the 27 positions is some output channel's tap.  The "wl0" set is the same with Wl = 0.
(d) conv1_2: C12_TERMS non-zeros per output channel, Wh = +-1, Wl in {-1, 0, 1} q, bias in -3 .. 3; relu1_1 <= 9, so
    sum |terms| + |bias| < 2048 = q 2^24.
(e) The reference, replay(): conv1_1's accumulator starts at bias x scale and takes the three products, is descaled, ReLU,
    zero outside the image, re-split by the encode model; conv1_2 the same three products, descaled, + bias, ReLU, rounded
    to float32 once -- exactly, asserted.  analysis() asserts per layer that every product is a multiple of the layer's
    quantum and sum |terms| + |bias| stays below quantum x 2^24 (every partial sum in any order is a float32 number) and
    that relu1_1's halves are the intended (A, eps); and gives, for each MUTANT (a wrong kernel restated on the
    reference; never compared with a kernel's output), the share of the outputs it changes."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

import persistent_refs as P
import split_refs as S

Q = 2.0 ** -13
SEARCH_ULPS = 8                       # float32 neighbours of float32(mean + std t) tried on either side
TABLE_B = tuple(range(-3, 4))         # lo = b q of the table
FRAME_HI, FRAME_B = (-1.0, 2.0), (-1, 0, 1)   # the levels frames draw from (and 0)
SHAPES = ((1, 1), (5, 7), (4, 32), (9, 33), (37, 70), (3, 200))  # the single-tile regime's frames, n = 3
RING_SHAPE = (P.S1_H, P.S1_W)         # the persistent regime's
PYRAMID_SHAPES = ((9, 33), (37, 70))
TH, TW = 4, 32                        # conv1_regw_split_kernel's output tile
C12_TERMS = 150
# conv1_1's output channel types: (Wh of its taps, bias).  Tap values are in {-1, 0, 2}:
#   (+1,)  b 0: {-1 dead, 0 (no lo term), 2}     (+1,)  b 3: {2, 3, 5}        (-1,)  b 4: {5, 4, 2}
#   (+1,+1) b 5: 5 + {-2 .. 4} >= 3              (+1,-1) b 6: 6 + {-3 .. 3} >= 3   (-1,-1) b 7: 7 - {-2 .. 4} >= 3
C11_TYPES = (((1.0,), 0.0), ((1.0,), 3.0), ((-1.0,), 4.0), ((1.0, 1.0), 5.0), ((1.0, -1.0), 6.0), ((-1.0, -1.0), 7.0))
MUTANTS = ("conv1_1: Wl*Ah dropped", "conv1_1: Wh*Al dropped", "relu1_1: lo = 0", "relu1_1: lo truncated toward zero",
           "conv1_2: Wl*Ah dropped", "conv1_2: Wh*Al dropped", "conv1_2: cross terms' activation halves swapped",
           "halo outside the image left at relu(bias)", "raw patch's pad channel not finite", "tile reads the previous tile's halo slot")


# ---- (a) the pixel table ------------------------------------------------------------------------------------------------
def normalise(raw: np.ndarray, c: int) -> np.ndarray:
    """fl(fl(raw - mean_c) / std_c) in float32, the kernels' source expression."""
    raw = np.asarray(raw, dtype=np.float32)
    return ((raw - P.S1_MEAN[c]).astype(np.float32) / P.S1_STD[c]).astype(np.float32)


def encode32(v: np.ndarray):
    """The device encode of float32 values in numpy: (hi, lo) as float64; v - hi is exact in float32 here."""
    v = np.asarray(v, dtype=np.float32)
    hi = v.astype(np.float16)
    lo = (v - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


@functools.lru_cache(maxsize=None)
def pixel_table():
    """Per channel {(hi, b): raw float32 pixel in [0, 1]} with normalise(raw) == hi + b q exactly and encode == (hi, b q).
    Deterministic: of the float32 numbers within SEARCH_ULPS of float32(mean + std t) the nearest, the lower one first."""
    table = []
    for c in range(3):
        mean, std = float(P.S1_MEAN[c]), float(P.S1_STD[c])
        found = {(0.0, 0): P.S1_MEAN[c]}
        assert float(normalise(P.S1_MEAN[c], c)) == 0.0
        for h2 in range(math.ceil(2.0 * (0.0 - mean) / std) - 1, math.floor(2.0 * (1.0 - mean) / std) + 2):
            for b in TABLE_B:
                hi = h2 / 2.0
                if hi == 0.0:
                    continue
                t = np.float32(hi + b * Q)
                assert float(t) == hi + b * Q
                below = above = np.float32(mean + std * float(t))
                cands = [below]
                for _ in range(SEARCH_ULPS):
                    below, above = np.nextafter(below, np.float32(-1.0)), np.nextafter(above, np.float32(2.0))
                    cands += [below, above]
                for raw in cands:
                    if 0.0 <= float(raw) <= 1.0 and normalise(raw, c) == t:
                        ehi, elo = encode32(t)
                        if float(ehi) == hi and float(elo) == b * Q:
                            found[(hi, b)] = raw
                        break
        table.append(found)
    return tuple(table)


def table_arrays(c: int):
    """(raw float32, hi float64, lo float64) of channel c's table, in sorted (hi, b) order."""
    keys = sorted(pixel_table()[c])
    return (np.array([pixel_table()[c][k] for k in keys], dtype=np.float32), np.array([k[0] for k in keys]),
            np.array([k[1] * Q for k in keys]))


def frame_levels(c: int):
    """{hi: [b, ...]} of the levels channel c's frame pixels draw from (besides 0)."""
    return {hi: [b for b in FRAME_B if (hi, b) in pixel_table()[c]] for hi in FRAME_HI}


# ---- (b) frames ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def frames(h: int, w: int, seed: int = 0):
    """Three base frames: (raw float32 NCHW (3, 3, h, w) in [0, 1], Vh float64, Vl float64 -- the intended halves of the
    normalised pixels).  About 0.42 / 0.10 / 0.48 of the pixels at -1 / 0 / 2.  Never modified."""
    from nerf_qa_amd import synth
    base = 5100 + 7 * h + w + 1000 * seed
    u = synth.uniform(base, 9 * h * w).reshape(3, 3, h, w)
    u2 = synth.uniform(base, 9 * h * w, 1).reshape(3, 3, h, w)
    raw, vh, vl = (np.zeros((3, 3, h, w), dtype=t) for t in (np.float32, np.float64, np.float64))
    for c in range(3):
        lv = frame_levels(c)
        raw[:, c] = pixel_table()[c][(0.0, 0)]
        for hi, pick in ((-1.0, u[:, c] < 0.42), (2.0, u[:, c] >= 0.52)):
            bs = np.array(lv[hi])
            b = bs[np.minimum((u2[:, c] * len(bs)).astype(np.int64), len(bs) - 1)]
            lut = np.array([pixel_table()[c][(hi, int(k))] for k in bs], dtype=np.float32)
            raw[:, c] = np.where(pick, lut[np.searchsorted(bs, b)], raw[:, c])
            vh[:, c] = np.where(pick, hi, vh[:, c])
            vl[:, c] = np.where(pick, b * Q, vl[:, c])
    assert 0.0 <= raw.min() and raw.max() <= 1.0
    return torch.from_numpy(raw), torch.from_numpy(vh), torch.from_numpy(vl)


def normalised_halves(h: int, w: int, seed: int = 0):
    """The encode model's halves of the float32 replay of the normalisation, asserted to be frames()'s (Vh, Vl)."""
    raw, vh, vl = frames(h, w, seed)
    v = np.stack([normalise(raw[:, c].numpy(), c) for c in range(3)], axis=1)
    assert v.dtype == np.float32
    mh, ml = encode32(v)
    assert np.array_equal(mh, vh.numpy()) and np.array_equal(ml, vl.numpy()), "the normalised pixels' encode is not (Vh, Vl)"
    assert np.array_equal(v.astype(np.float64), mh + ml)
    return torch.from_numpy(mh), torch.from_numpy(ml)


# ---- (c), (d) weights -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def conv1_1_weights(wl0: bool = False):
    """(w float32 OIHW (64, 3, 3, 3) = Wh + Wl, Wh, Wl float64, bias float64 (64,)): output channel o is of type
    C11_TYPES[o % 6], its first tap at position perm[o % 27] of the 27 (channel, ky, kx), a second one at another."""
    from nerf_qa_amd import synth
    perm = np.argsort(synth.uniform(6100, 27))
    other = synth.uniform(6101, 64)
    sl = np.floor(synth.uniform(6102, 128) * 3.0).clip(0, 2).reshape(64, 2) - 1.0
    wh, wl, bias = np.zeros((64, 27)), np.zeros((64, 27)), np.zeros(64)
    for o in range(64):
        signs, bias[o] = C11_TYPES[o % len(C11_TYPES)]
        first = int(perm[o % 27])
        pos = [first] + ([(first + 1 + int(other[o] * 26)) % 27] if len(signs) == 2 else [])
        assert len(set(pos)) == len(pos)
        for j, (p, s) in enumerate(zip(pos, signs)):
            wh[o, p], wl[o, p] = s, 0.0 if wl0 else sl[o, j] * Q
    wh, wl = wh.reshape(64, 3, 3, 3), wl.reshape(64, 3, 3, 3)
    w = (wh + wl).astype(np.float32)
    assert np.array_equal(w.astype(np.float64), wh + wl)
    return w, torch.from_numpy(wh), torch.from_numpy(wl), torch.from_numpy(bias)


@functools.lru_cache(maxsize=None)
def conv1_2_weights():
    """(w float32 OIHW (64, 64, 3, 3) = Wh + Wl, Wh, Wl float64, bias float64 (64,)) as split_refs.split_weights, with
    C12_TERMS non-zeros per output channel."""
    from nerf_qa_amd import synth
    cout, k, seed = 64, 576, 6200
    u = synth.uniform(seed, cout * k).reshape(cout, k)
    sh = np.where(synth.uniform(seed, cout * k, 1).reshape(cout, k) < 0.5, -1.0, 1.0)
    sl = (np.floor(synth.uniform(seed, cout * k, 2) * 3.0).clip(0, 2) - 1.0).reshape(cout, k) * Q
    pick = np.argsort(u, axis=1)[:, :C12_TERMS]
    wh, wl = np.zeros((cout, k)), np.zeros((cout, k))
    np.put_along_axis(wh, pick, np.take_along_axis(sh, pick, axis=1), axis=1)
    np.put_along_axis(wl, pick, np.take_along_axis(sl, pick, axis=1), axis=1)
    wh, wl = wh.reshape(cout, 64, 3, 3), wl.reshape(cout, 64, 3, 3)
    w = (wh + wl).astype(np.float32)
    assert np.array_equal(w.astype(np.float64), wh + wl)
    b = np.floor(synth.uniform(seed + 1, cout) * 7.0).clip(0, 6) - 3.0
    return w, torch.from_numpy(wh), torch.from_numpy(wl), torch.from_numpy(b)


@functools.lru_cache(maxsize=None)
def convs(key: str = "split"):
    """The synthetic VGG weights with conv1_1 and conv1_2 replaced; key "split" | "wl0" (conv1_1 with Wl = 0)."""
    from nerf_qa_amd import synth
    out = list(synth.vgg16_weights(1234))
    for layer, (w, _, _, b) in enumerate((conv1_1_weights(key == "wl0"), conv1_2_weights())):
        out[layer] = (w, b.numpy().astype(np.float32))
    return out


@functools.lru_cache(maxsize=None)
def copy_convs():
    """The diagnostic's weights: conv1_1's output channel c < 3 copies the centre tap of input channel c, bias 3."""
    from nerf_qa_amd import synth
    out = list(synth.vgg16_weights(1234))
    w = np.zeros((64, 3, 3, 3), dtype=np.float32)
    for c in range(3):
        w[c, c, 1, 1] = 1.0
    out[0] = (w, np.full(64, 3.0, dtype=np.float32))
    return out


@functools.lru_cache(maxsize=None)
def halves(key: str = "split") -> dict:
    """The encode model's halves of both layers' weights times the blob's scale, asserted to be (s Wh, s Wl)."""
    m = {}
    for name, (w32, wh, wl, bias) in (("1", conv1_1_weights(key == "wl0")), ("2", conv1_2_weights())):
        s = 2.0 ** S.weight_scale_exp(w32)
        assert s == (1024.0 if name == "1" and key == "wl0" else S.SCALE), f"conv1_{name}: weight_scale_exp gives {s}"
        mh, ml = S.encode_model(torch.from_numpy(w32).double() * s)
        assert torch.equal(mh, wh * s) and torch.equal(ml, wl * s), f"conv1_{name}: the weights' encode is not (s Wh, s Wl)"
        m.update({"h" + name: mh, "l" + name: ml, "s" + name: s, "b" + name: bias.view(1, -1, 1, 1)})
    return m


# ---- (e) the reference -----------------------------------------------------------------------------------------------------
def truncated_half(v64: torch.Tensor) -> torch.Tensor:
    """v as a half rounded TOWARD ZERO (a mutant's conversion), in float64."""
    v = v64.numpy()
    h = v.astype(np.float16)
    over = np.abs(h.astype(np.float64)) > np.abs(v)
    h[over] = np.nextafter(h[over], np.float16(0.0))
    return torch.from_numpy(h.astype(np.float64))


def _tiles(a: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """(n, C, h, w) -> the kernel's halo patches (n * tiles_y * tiles_x, C, TH + 2, TW + 2), zero outside the map."""
    ty, tx = P.cdiv(h, TH), P.cdiv(w, TW)
    a = F.pad(a, (1, tx * TW - w + 1, 1, ty * TH - h + 1))
    p = a.unfold(2, TH + 2, TH).unfold(3, TW + 2, TW)                 # (n, C, ty, tx, TH + 2, TW + 2)
    return p.permute(0, 2, 3, 1, 4, 5).reshape(-1, a.shape[1], TH + 2, TW + 2)


def _untile(t: torch.Tensor, n: int, h: int, w: int) -> torch.Tensor:
    ty, tx = P.cdiv(h, TH), P.cdiv(w, TW)
    t = t.reshape(n, ty, tx, t.shape[1], TH, TW).permute(0, 3, 1, 4, 2, 5).reshape(n, t.shape[1], ty * TH, tx * TW)
    return t[:, :, :h, :w]


def replay(key: str, h: int, w: int, seed: int = 0, mutant=None, parts: bool = False):
    """relu1_2 of the three base frames as the kernel computes it, in float64, NHWC (3, h, w, 64) (not yet rounded).
    mutant: one of MUTANTS.  parts: the intermediate terms as a dict instead."""
    assert mutant is None or mutant in MUTANTS
    m = halves(key)
    vh, vl = normalised_halves(h, w, seed)

    def conv(a, wq, pad=1):
        return F.conv2d(a, wq, None, padding=pad)
    t1 = dict(hh=conv(vh, m["h1"]), lh=conv(vh, m["l1"]), hl=conv(vl, m["h1"]))   # w_hi a_hi, w_lo a_hi, w_hi a_lo
    if mutant == MUTANTS[0]:
        t1["lh"] = torch.zeros_like(t1["lh"])
    if mutant == MUTANTS[1]:
        t1["hl"] = torch.zeros_like(t1["hl"])
    acc1 = m["b1"] * m["s1"] + t1["hh"] + t1["lh"] + t1["hl"]
    r11 = F.relu(acc1 / m["s1"]) + 0.0
    if mutant == MUTANTS[8]:
        # the pad channel's weights are zero in the blob: a finite value there changes nothing, a NaN or an infinity makes
        # every accumulator of conv1_1 a NaN (0 x NaN), which the kernel's fmaxf(., 0) turns into 0
        r11 = torch.zeros_like(r11)
    rh, rl = S.encode_model(r11)  # (asserts that relu1_1 is a float32 number)
    if mutant == MUTANTS[2]:
        rl = torch.zeros_like(rl)
    if mutant == MUTANTS[3]:
        rl = truncated_half(r11 - rh)
    if mutant == MUTANTS[7]:  # a ring of relu(bias) around the image instead of zeros
        ring = F.relu(m["b1"]).expand(3, 64, h + 2, w + 2).clone()
        gh, gl = S.encode_model(ring)
        gh[:, :, 1:-1, 1:-1], gl[:, :, 1:-1, 1:-1] = rh, rl
        rh, rl, pad = gh, gl, 0
    else:
        pad = 1
    if mutant == MUTANTS[9]:  # tile t's conv1_2 on the halo of tile t - 1 (in [image][row][column] order; tile 0: zeros)
        def conv2(a, wq):
            p = _tiles(a, h, w)
            return _untile(conv(torch.cat([torch.zeros_like(p[:1]), p[:-1]]), wq, 0), 3, h, w)
    else:
        def conv2(a, wq):
            return conv(a, wq, pad)
    t2 = dict(hh=conv2(rh, m["h2"]), lh=conv2(rh, m["l2"]), hl=conv2(rl, m["h2"]))
    if mutant == MUTANTS[4]:
        t2["lh"] = torch.zeros_like(t2["lh"])
    if mutant == MUTANTS[5]:
        t2["hl"] = torch.zeros_like(t2["hl"])
    if mutant == MUTANTS[6]:  # w_lo a_lo + w_hi a_hi
        t2["lh"], t2["hl"] = conv2(rl, m["l2"]), conv2(rh, m["h2"])
    pre = (t2["hh"] + t2["lh"] + t2["hl"]) / m["s2"] + m["b2"]
    if parts:
        return dict(vh=vh, vl=vl, t1=t1, r11=r11, rh=rh, rl=rl, t2=t2, pre=pre)
    return (F.relu(pre) + 0.0).permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def reference(key: str, h: int, w: int, seed: int = 0) -> torch.Tensor:
    """The kernel's output, float32 NHWC (3, h, w, 64): one rounding, exact (asserted).  Never modified."""
    v = replay(key, h, w, seed)
    out = v.to(torch.float32)
    assert torch.equal(out.double(), v)
    return out


@functools.lru_cache(maxsize=None)
def relu1_1_reference(key: str, h: int, w: int, seed: int = 0):
    """(hi, lo) halves of relu1_1's split16 records, NHWC (3, h, w, 64) half tensors."""
    p = replay(key, h, w, seed, parts=True)
    return tuple(t.permute(0, 2, 3, 1).contiguous().half() for t in (p["rh"], p["rl"]))


def tiled_replay_matches(key: str, h: int, w: int) -> bool:
    """The tile decomposition the slot mutant uses gives the plain convolution when every tile reads its own halo."""
    p = replay(key, h, w, parts=True)
    m = halves(key)
    own = _untile(F.conv2d(_tiles(p["rh"], h, w), m["h2"], None), 3, h, w)
    return torch.equal(own, p["t2"]["hh"])


def analysis(key: str, h: int, w: int, seed: int = 0) -> dict:
    """The conditions of (c) .. (e) asserted on the frames of one shape, and the share of the outputs each mutant changes."""
    m, p = halves(key), replay(key, h, w, seed, parts=True)
    vh, vl, r11, rh, rl = (p[k] for k in ("vh", "vl", "r11", "rh", "rl"))

    def aconv(a, wq):
        return F.conv2d(a.abs(), wq.abs(), None, padding=1)
    # conv1_1: multiples of s q, sum |terms| + |bias| s < s q 2^24
    q1 = m["s1"] * Q
    for t in p["t1"].values():
        assert torch.equal(torch.round(t / q1) * q1, t)
    mag1 = float((aconv(vh, m["h1"]) + aconv(vh, m["l1"]) + aconv(vl, m["h1"]) + m["b1"].abs() * m["s1"]).max()) / m["s1"]
    assert mag1 < Q * 2 ** 24, mag1
    # relu1_1 = 0 or A + eps, A an integer >= 2, |eps| below half of the half-ulp under A, re-split (A, eps)
    a = torch.round(r11)
    eps = r11 - a
    live = r11 > 0
    assert bool((a[live] >= 2).all()), "a relu1_1 below 2"
    ulp_under = 2.0 ** (torch.floor(torch.log2(a[live] - 0.5)) - 10)
    assert bool((eps[live].abs() < ulp_under / 2).all())
    assert torch.equal(rh, a) and torch.equal(rl, eps) and torch.equal(torch.round(eps / Q) * Q, eps)
    assert bool((eps[~live] == 0).all())
    # conv1_2
    q2 = m["s2"] * Q
    for t in p["t2"].values():
        assert torch.equal(torch.round(t / q2) * q2, t)
    mag2 = float(((aconv(rh, m["h2"]) + aconv(rh, m["l2"]) + aconv(rl, m["h2"])) / m["s2"] + m["b2"].abs()).max())
    assert mag2 < Q * 2 ** 24, mag2
    ref = reference(key, h, w, seed)

    def share(mutant):
        return float((replay(key, h, w, seed, mutant).to(torch.float32) != ref).double().mean())
    four = (F.conv2d(vl, m["l1"], None, padding=1) != 0).double().mean()
    return dict(bound1=mag1, bound2=mag2, largest1=float(r11.max()), largest=float(p["pre"].abs().max()),
                live1=float(live.double().mean()), lo1=float((rl != 0).double().mean()), positive=float((p["pre"] > 0).double().mean()),
                lolo1=float(four), mutants={mu: share(mu) for mu in MUTANTS})
