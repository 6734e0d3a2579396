"""The f32s fused stage 1 (conv1_regw_split_kernel of nqa_conv.hip) on frames whose normalised pixels, relu1_1 and
weights all have NON-ZERO lo halves, bit for bit (GPU box only).

f32s is the mode every other mode is calibrated against, and in the forward its stage 1 is this one kernel: the
normalisation in float split into (hi, lo) halves, conv1_1 on the MFMA as w_hi*a_hi + w_lo*a_hi + w_hi*a_lo, relu1_1
re-split into halves in LDS, conv1_2 the same three products, a persistent tile walk over a two-slot halo ring.  The 2e-6
of the largest activation it is held to elsewhere (test_gpu_ops.py::test_f32s_stage1_fused, the f32s row of
test_gpu_conv_persistent.py) is hundreds of ulps of a typical output: a truncated lo half, a dropped cross term or a
wrong value confined to small outputs passes.  Here the operands of tests/stage1_split_refs.py -- raw float32 pixels that
the kernel's (raw - mean) / std maps EXACTLY onto the levels -1 + b q, 0, 2 + b q (q = 2^-13), a sparse conv1_1 with
Wh = +-1, Wl in {-1, 0, 1} q whose relu1_1 is 0 or an integer A >= 2 plus a lo part eps, a split_refs-style conv1_2 --
make every product and every partial sum of either layer a float32 number in any order, so each output must be BIT-EQUAL
to the float64 restatement of that arithmetic (tests/test_stage1_split_refs.py: a dropped or mis-paired term, a zeroed
relu1_1 lo, a halo pixel left at relu(bias) or a stale halo slot each change up to half of the outputs).

Every output is passed in pre-filled with 0xFF bytes and searched for NaN first; every comparison is on bits.
  the diagnostic   ops.conv1_1(x, blob, "f32") = conv1_1_kernel<PrecF32>, which normalises by the same source expression:
                   with weights that copy the centre tap of channel c into output c and a bias of 3, output - 3 must be the
                   numpy float32 replay of fl(fl(raw - mean) / std) on the whole pixel table.  If THAT fails the device
                   does not evaluate the expression as correctly rounded float32 and the exact tests below are void.
  (a) one tile     ops.conv1_fused(x, blob, "f32s", out=), n = 3, at 1x1, 5x7 (inside one 4 x 32 tile), 4x32 (exactly one),
                   9x33 (partial tiles both ways), 37x70 and 3x200 (a wide strip): a block per tile, or two tiles where
                   the XCD-aware split deals them so (the regime is printed)
  (b) persistent   150 x 130, n = persistent_refs.batch_for("conv1_regw_split"): some block owns >= 4 tiles (both halo
                   slots and both raw patches reused, the counted vmcnt(4) behind a tile's stores), some fewer than
                   another; image k = base frame k % 3; a failure names block, step and ring slot
  (c) the forward  ops.vgg_pyramid(x, blob, "f32s")[0] gives the same bits at 9x33 and 37x70
  (d) two kernels  on the Wl = 0 conv1_1 set the first forms are the same exact function (conv1_1_kernel<PrecF32S> forms
                   Wh (vh + vl) in float -- the kernel's two terms; its only lo*lo product would be with Wl): the pyramid
                   under DEFAULT | 16, and ops.conv1_1 (relu1_1's split16 records compared half by half) followed by
                   ops.conv3x3_relu(., 1) (conv3x3_igemm_kernel<PrecF32S, 1,4,2,2>; what autograd.pyramid_keep /
                   pyramid_taps run in every loss step), both equal to the reference AND to the fused kernel's output
  (e) the y side   the kernel takes two image pointers (n < B from x, else y), but no ops entry that returns a map reaches
                   it with distinct x and y: ops.conv1_fused and ops.vgg_pyramid pass y = null with B = n, and the forwards
                   that pass both (nqa_dists_forward, the A-DISTS forward) return scores only.  Not tested here: a y image
                   goes through the same arithmetic as an x image, and a wrong y pointer is what every f32s score test
                   against the oracle sees."""
import numpy as np
import pytest
import torch

import persistent_refs as P
import split_refs as S
import stage1_split_refs as T
from test_gpu_conv_persistent import _nan_filled, _no_nan_left, _walk_report

pytestmark = pytest.mark.gpu

KERNEL = "conv1_regw_split"
_ID = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)  # noqa: E731


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


@pytest.fixture(scope="module")
def blob(dev):
    """blob("split" | "wl0"): the f32s blob of stage1_split_refs.convs; blob("copy"): the diagnostic's f32 blob."""
    made = {}

    def get(key):
        if key not in made:
            from nerf_qa_amd import ops
            made[key] = (ops.pack_vgg_weights(T.copy_convs(), "f32") if key == "copy"
                         else ops.pack_vgg_weights(T.convs(key), "f32s")).to(dev)
        return made[key]
    return get


def _assert_same_bits(got, ref, what, report=None):
    """got, ref: (n, h, w, C) CPU tensors of one dtype (float32 or half)."""
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype)
    bits = {torch.float16: torch.int16, torch.float32: torch.int32}[got.dtype]
    same = got.view(bits) == ref.view(bits)
    print(f"   {what}: {int((~same).sum())} of {same.numel()} values differ; largest expected value {ref.float().max().item():.6g}")
    if not bool(same.all()):
        elems = (~same).nonzero()
        bad = (~same).any(dim=3).nonzero()
        ch = sorted(set(elems[:, 3].tolist()))
        i, r, c, k = elems[0].tolist()
        raise AssertionError(f"{what}: {elems.shape[0]} values ({float((~same).double().mean()):.4f} of them) in {bad.shape[0]} pixels "
                             f"differ from the float64 reference; first (image, row, column) {bad[:6].tolist()}; rows hit "
                             f"{sorted(set(bad[:, 1].tolist()))[:24]}; columns hit {sorted(set(bad[:, 2].tolist()))[:24]}; channels "
                             f"hit {ch[:8]} .. {ch[-1]}; at {[i, r, c, k]} got {got[i, r, c, k].item()!r}, expected "
                             f"{ref[i, r, c, k].item()!r}" + ("; " + report(elems[:4096]) if report else ""))


def _fused(key, h, w, n, blob, cus, dev):
    """One launch of conv1_regw_split_kernel through ops.conv1_fused on image k = base frame k % 3 into a NaN-filled
    out=; the output on the CPU, searched for NaN."""
    from nerf_qa_amd import ops
    r = P.regime(KERNEL, n, h, w, cus)
    print(f"\n stage 1 [f32s, {key}] {KERNEL}_kernel: {n}x{h}x{w}, {r['total']} tiles on {r['grid']} blocks of {cus} CUs, "
          f"{r['least']}..{r['most']} tiles per block, halo ring of {r['ring']}")
    x = P.batch_of(T.frames(h, w)[0], n).to(dev)
    out = _nan_filled((n, h, w, 64), torch.float32, dev)
    assert ops.conv1_fused(x, blob(key), "f32s", out=out) is out
    _no_nan_left(out, f"stage 1 [f32s, {key}] {n}x{h}x{w}")
    return out.cpu(), r


def test_the_device_normalises_as_the_replay_does(blob, dev):
    """conv1_1_kernel<PrecF32> on the whole pixel table (channel c's pixels in plane c, the rest at the mean)."""
    from nerf_qa_amd import ops
    tabs = [T.table_arrays(c) for c in range(3)]
    h, w = 5, 7
    assert max(len(t[0]) for t in tabs) <= h * w
    raw = np.stack([np.full(h * w, P.S1_MEAN[c], dtype=np.float32) for c in range(3)])
    for c in range(3):
        raw[c, : len(tabs[c][0])] = tabs[c][0]
    replay = np.stack([T.normalise(raw[c], c) for c in range(3)], axis=1).reshape(h, w, 3)
    for c in range(3):
        assert np.array_equal(replay.reshape(-1, 3)[: len(tabs[c][0]), c].astype(np.float64), tabs[c][1] + tabs[c][2])
    out = ops.conv1_1(torch.from_numpy(raw.reshape(1, 3, h, w)).to(dev), blob("copy"), "f32")
    assert out.dtype == torch.float32 and out.shape == (1, h, w, 64)
    got = out.cpu()
    assert bool((got[..., 3:] == 3.0).all())
    print(f"\n conv1_1_kernel<PrecF32> on {[len(t[0]) for t in tabs]} table pixels of channels 0 / 1 / 2")
    _assert_same_bits((got[..., :3] - 3.0).contiguous(), torch.from_numpy(replay).view(1, h, w, 3).contiguous(),
                      "the device's (raw - mean) / std against the numpy float32 replay")


@pytest.mark.parametrize("shape", T.SHAPES, ids=_ID)
def test_one_tile_per_block_is_bit_exact(shape, blob, cus, dev):
    h, w = shape
    got, r = _fused("split", h, w, 3, blob, cus, dev)
    assert r["most"] <= (1 if r["total"] == 3 else 2) or cus < r["total"], r
    _assert_same_bits(got, T.reference("split", h, w), f"stage 1 [f32s] 3x{h}x{w}",
                      lambda e: _walk_report(KERNEL, e, 3, h, w, cus, 1, 64))


def test_the_persistent_walk_is_bit_exact(blob, cus, dev):
    h, w = T.RING_SHAPE
    n = P.batch_for(KERNEL, h, w, cus)
    r = P.regime(KERNEL, n, h, w, cus)
    assert P.in_regime(r) and r["most"] >= 4 and r["least"] < r["most"] and r["dummy_halo"], r
    got, _ = _fused("split", h, w, n, blob, cus, dev)
    ref = P.batch_of(T.reference("split", h, w), n)
    _assert_same_bits(got, ref, f"stage 1 [f32s] {n}x{h}x{w}", lambda e: _walk_report(KERNEL, e, n, h, w, cus, 1, 64))


@pytest.mark.parametrize("shape", T.PYRAMID_SHAPES, ids=_ID)
def test_the_forward_reaches_the_same_bits(shape, blob, cus, dev):
    """nqa_vgg_pyramid (run_stages: stage1_is_fused -> conv1_fused -> launch_conv1_regw_split) under the default variant."""
    from nerf_qa_amd import ops
    h, w = shape
    fused, _ = _fused("split", h, w, 3, blob, cus, dev)
    tap1 = ops.vgg_pyramid(T.frames(h, w)[0].to(dev), blob("split"), "f32s")[0].cpu()
    print(f"   vgg_pyramid [f32s] 3x{h}x{w}: tap 1 from {KERNEL}_kernel")
    _assert_same_bits(tap1, T.reference("split", h, w), f"vgg_pyramid [f32s] tap 1 3x{h}x{w}")
    _assert_same_bits(tap1, fused, f"vgg_pyramid [f32s] tap 1 against conv1_fused 3x{h}x{w}")


@pytest.mark.parametrize("shape", T.SHAPES, ids=_ID)
def test_the_two_kernel_forms_are_the_same_exact_function(shape, blob, cus, dev):
    from nerf_qa_amd import ops
    h, w = shape
    ref = T.reference("wl0", h, w)
    fused, _ = _fused("wl0", h, w, 3, blob, cus, dev)
    _assert_same_bits(fused, ref, f"stage 1 [f32s, wl0] 3x{h}x{w}")
    x = T.frames(h, w)[0].to(dev)
    ops.set_conv_variant(ops.DEFAULT_CONV_VARIANT | 16)
    try:
        tap1 = ops.vgg_pyramid(x, blob("wl0"), "f32s")[0].cpu()
    finally:
        ops.set_conv_variant(ops.DEFAULT_CONV_VARIANT)
    tile = S.vgg_instance(1, 3, h, w, 0, True, cus)
    print(f"   first forms: conv1_1_kernel<PrecF32S>, then conv3x3_igemm_kernel<PrecF32S, {tile[0][1:-1]}, {tile[1]}>")
    assert tile[0] == "<1,4,2,2>" and tile[1] == (16 if w <= 16 else 32)
    _assert_same_bits(tap1, ref, f"vgg_pyramid under DEFAULT | 16 [f32s, wl0] tap 1 3x{h}x{w}")
    _assert_same_bits(tap1, fused, f"vgg_pyramid under DEFAULT | 16 against the fused kernel 3x{h}x{w}")
    r11 = ops.conv1_1(x, blob("wl0"), "f32s")
    assert r11.dtype == torch.float32 and r11.shape == (3, h, w, 64)
    ghi, glo = S.record_halves(r11.cpu())
    rhi, rlo = T.relu1_1_reference("wl0", h, w)
    _assert_same_bits(ghi.contiguous(), rhi, f"ops.conv1_1 [f32s, wl0] 3x{h}x{w}: hi halves of relu1_1's split16 records")
    _assert_same_bits(glo.contiguous(), rlo, f"ops.conv1_1 [f32s, wl0] 3x{h}x{w}: lo halves of relu1_1's split16 records")
    out = _nan_filled((3, h, w, 64), torch.float32, dev)
    assert ops.conv3x3_relu(r11, 1, blob("wl0"), "f32s", out=out) is out
    _no_nan_left(out, f"conv1_1 + conv1_2 [f32s, wl0] 3x{h}x{w}")
    pair = out.cpu()
    _assert_same_bits(pair, ref, f"ops.conv1_1 + ops.conv3x3_relu(., 1) [f32s, wl0] 3x{h}x{w}")
    _assert_same_bits(pair, fused, f"ops.conv1_1 + ops.conv3x3_relu(., 1) against the fused kernel 3x{h}x{w}")
