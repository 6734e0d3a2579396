"""The f32s convolutions of nqa_conv.hip on operands whose lo halves are NOT zero, bit for bit (GPU box only).

f32s computes al*bh + ah*bl + ah*bh from (hi, lo) half pairs of weights and activations (the P::SPLIT branch of
conv3x3_igemm_tile, its LOACC form with a second accumulator for the cross terms, and conv3x3_regw_split_kernel).  The
cross terms are 2^-11 of the main one, so a dropped, doubled or mis-paired one moves the last bits of nearly every output
and stays far below the 2e-5 bar the mode is held to elsewhere; integer operands, whose lo halves are zero, never reach
them.  Here the operands of tests/split_refs.py make every product and every partial sum of the three terms a float32
number in any order, so each output must be BIT-EQUAL to the float64 restatement of that arithmetic
(tests/test_split_refs.py: such mutants differ in 96 .. 99 % of the outputs).  Two sets: "normal" (lo halves are normal
halves, 2^-13) and "small" (activations of 2^-6 and 2^-5 whose lo, 2^-19, is a SUBNORMAL half: the halves must survive
the encode, the MFMA operand path and the split16 epilogue).

Every case goes through ops.split16_encode, whose records are first asserted to hold exactly the intended halves, then
ops.conv3x3_relu(..., "f32s") into an out= pre-filled with 0xFF bytes, or ops.conv3x3_split (which takes none).  Tapped
layers (conv1_2, conv4_3) leave as float and are compared as float bits; the others leave as split16 records
(hi = half(v), lo = half(v - hi), staged through the swizzled LDS tile) and are compared half by half.  The instance each
case runs is read off launch_conv / conv3x3_split_generic by split_refs.vgg_instance / instance, asserted from the shape
before the launch, with ops.mixed_grid_launches() telling the grid:
  conv1_2 (layer 1)  2x9x40, 2x5x13        conv3x3_igemm_kernel<PrecF32S, 1,4,2,2, 32 | 16>: the 64-channel tile, float out
  conv2_1 (layer 2)  2x9x40                conv3x3_regw_split_kernel, one unit per block; and a batch sized by
                                           persistent_refs.batch_for so that the ring wraps on split operands ("normal")
  conv2_1            2x9x40 + 16 + 256     <2,2,2,2, 32>: the 4-wave tile (first forms: no register-weights kernel)
  conv2_1            2x7x13                <2,2,2,2, 16> (W < 16 keeps it off the register-weights kernel)
  conv4_2 (layer 8)  2x13x80 + 256, + 512  <2,2,2,2, 32>, Cin 512: 96 stages; plain grid, and conv3x3_igemm_mixed_kernel
  conv4_3 (layer 9)  2x11x13               <2,2,2,2, 16>, float out
  conv4_1 (layer 7)  20x24x64              <2,4,4,2, 32>: the 8-wave tile (240 blocks_big >= 192; images repeat three)
  conv4_1            20x23x40 + 256        8-wave, plain grid, ragged right and bottom
  conv4_1            20x24x48 + 512        8-wave, mixed grid
  data gradients     2x6x21, 2x3x13        <2,2,2,2, 32 | 16, LOACC> for (Cin, Cout) = (128,128), (512,256), (512,512) and
                                           <1,4,2,2, 32 | 16, LOACC> for (64,64), (128,64), through ops.pack_conv_split /
                                           ops.conv3x3_split on SIGNED activations: relu=False against the reference, and
                                           relu=True bit-equal to its clamp
Stage 1 fused (conv1_regw_split_kernel) has a file of its own, tests/test_gpu_stage1_split_exact.py: raw pixels that its
normalisation maps exactly onto (hi, lo) levels exist (tests/stage1_split_refs.py searches them)."""
import pytest
import torch

import persistent_refs as P
import split_refs as S

pytestmark = pytest.mark.gpu

BITS = {torch.float16: torch.int16, torch.float32: torch.int32}
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
    """blob("vgg"): the f32s blob of split_refs.split_convs; blob(("grad", Cin, Cout)): that layer by pack_conv_split."""
    made = {}

    def get(key):
        if key not in made:
            from nerf_qa_amd import ops
            made[key] = (ops.pack_vgg_weights(S.split_convs(), "f32s") if key == "vgg"
                         else ops.pack_conv_split(S.weights_of(key)[0])).to(dev)
        return made[key]
    return get


def _assert_same_bits(got, ref, what):
    """got, ref: (n, h, w, C) CPU tensors of one dtype."""
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype)
    same = got.view(BITS[got.dtype]) == ref.view(BITS[ref.dtype])
    print(f"   {what}: {int((~same).sum())} of {same.numel()} values differ; largest expected |value| {ref.float().abs().max().item():.6g}")
    if not bool(same.all()):
        elems = (~same).nonzero()
        bad = (~same).any(dim=3).nonzero()
        ch = sorted(set(elems[:, 3].tolist()))
        i, r, c, k = elems[0].tolist()
        raise AssertionError(f"{what}: {elems.shape[0]} values ({float((~same).double().mean()):.4f} of them) in {bad.shape[0]} pixels "
                             f"differ from the float64 reference, {int(torch.isnan(got.float()).sum())} of them never written; first "
                             f"(image, row, column) {bad[:6].tolist()}; rows hit {sorted(set(bad[:, 1].tolist()))[:24]}; columns hit "
                             f"{sorted(set(bad[:, 2].tolist()))[:24]}; channels hit {ch[:8]} .. {ch[-1]}; at {[i, r, c, k]} got "
                             f"{got[i, r, c, k].item()!r}, expected {ref[i, r, c, k].item()!r}")


def _encoded(a32, ah, al, idx, dev, what):
    """split16 records of image k = base[idx[k]] on the device, asserted to hold exactly the intended halves."""
    from nerf_qa_amd import ops
    enc = ops.split16_encode(a32[idx].contiguous().to(dev))
    ehi, elo = S.record_halves(enc.cpu())
    _assert_same_bits(ehi, ah[idx].half(), what + ": hi halves of the encoded input")
    _assert_same_bits(elo, al[idx].half(), what + ": lo halves of the encoded input")
    return enc


def _run_layer(layer, n, h, w, extra, want_mixed, name, blob, dev):
    """One ops.conv3x3_relu in f32s under DEFAULT | extra into an 0xFF-filled out=, against the reference."""
    from nerf_qa_amd import ops
    nb = min(n, 3)
    idx = torch.arange(n) % nb
    what = f"layer {layer} [f32s, {name}] {n}x{h}x{w} + {extra}"
    a32, ah, al = S.split_acts(name, ops.CONV_CIN[layer], h, w, nb)
    enc = _encoded(a32, ah, al, idx, dev, what)
    out = torch.empty((n, h, w, ops.CONV_COUT[layer]), dtype=torch.float32, device=dev)
    out.view(torch.uint8).fill_(0xFF)
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(out.view(torch.float16)).all())
    ops.set_conv_variant(ops.DEFAULT_CONV_VARIANT | extra)
    try:
        ops.mixed_grid_launches()
        res = ops.conv3x3_relu(enc, layer, blob("vgg"), "f32s", out=out)
        launched = ops.mixed_grid_launches()
    finally:
        ops.set_conv_variant(ops.DEFAULT_CONV_VARIANT)
    assert res is out and launched == want_mixed, f"{what}: mixed grids launched: {launched}, expected {want_mixed}"
    ref = S.reference(("vgg", layer), name, h, w, nb)[idx]
    if layer in ops.TAP_LAYERS:
        _assert_same_bits(out.cpu(), ref, what + ": float map")
    else:
        ghi, glo = S.record_halves(out.cpu())
        rhi, rlo = S.records(ref)
        _assert_same_bits(ghi, rhi, what + ": hi halves of the split16 records")
        _assert_same_bits(glo, rlo, what + ": lo halves of the split16 records")


@pytest.mark.parametrize("name", list(S.SETS))
@pytest.mark.parametrize("shape,extra,kernel,tw,want_mixed", S.VGG_CASES, ids=_ID)
def test_split_operands_are_bit_exact(shape, extra, kernel, tw, want_mixed, name, blob, cus, dev):
    """The instance is the case's `kernel` (<WAVES_N, WAVES_M, WN_T, WM_T> of conv3x3_igemm_kernel<PrecF32S, ...> or of the
    mixed kernel, or regw_split) at tile width `tw`; see the module's table."""
    from nerf_qa_amd import ops
    layer, n, h, w = shape
    assert S.vgg_instance(layer, n, h, w, extra, True, cus) == (kernel, tw, want_mixed)
    if kernel == "regw_split":
        assert layer == 2 and w >= 16 and h >= 2 and not extra & 16
        assert P.regime("regw_split", n, h, w, cus, 2)["most"] == 1 or cus < 24
    else:
        i = S.instance(ops.CONV_COUT[layer], n, h, w, 1, extra & 768, True, cus)
        assert i["narrow"] == (w <= 16) == (tw == 16)
        if kernel == "<1,4,2,2>":
            assert ops.CONV_COUT[layer] == 64
        elif kernel == "<2,4,4,2>":
            assert i["big"] and i["blocks_big"] >= 192 and i["eff_big"] * 1.05 >= i["eff_small"] and not i["narrow"]
        else:
            assert not i["big"] and (i["narrow"] or i["blocks_big"] < 192) and (layer != 2 or extra & 16 or w < 16)
        assert i["mixed"] == bool(want_mixed) and (not extra & 768 or 1 <= w % 32 <= 16)
    print(f"\n layer {layer} [f32s, {name}] {n}x{h}x{w} + {extra}: {kernel}, {tw} wide, {want_mixed} mixed grids")
    _run_layer(layer, n, h, w, extra, want_mixed, name, blob, dev)


def test_split_operands_are_bit_exact_past_one_tile_of_regw_split(blob, cus, dev):
    """conv3x3_regw_split_kernel with blocks that walk several tiles (the two-slot ring wraps), "normal" set."""
    n = P.batch_for("regw_split", P.H, P.W, cus, 2)
    r = P.regime("regw_split", n, P.H, P.W, cus, 2)
    print(f"\n layer 2 [f32s, normal] regw_split: {n}x{P.H}x{P.W}, {r['total']} tiles on {r['grid']} blocks of {cus} CUs, "
          f"{r['least']}..{r['most']} tiles per block, ring of {r['ring']}")
    assert P.in_regime(r) and r["most"] >= 4 and r["least"] < r["most"], r
    _run_layer(2, n, P.H, P.W, 0, 0, "normal", blob, dev)


@pytest.mark.parametrize("name", list(S.SETS))
@pytest.mark.parametrize("hw", S.GRAD_MAPS, ids=_ID)
@pytest.mark.parametrize("cin,cout", S.GRAD_SHAPES, ids=_ID)
def test_data_gradient_convs_are_bit_exact(cin, cout, hw, name, blob, dev):
    """conv3x3_split_generic: conv3x3_igemm_kernel<PrecF32S, 2,2,2,2, TW, false, 1, LOACC> where Cout % 128 == 0,
    <PrecF32S, 1,4,2,2, TW, false, 1, LOACC> otherwise; TW = 16 for W <= 16, else 32."""
    from nerf_qa_amd import ops
    h, w = hw
    assert (cout % 128 == 0) == ((cin, cout) in S.GRAD_SHAPES[:3]) and cout % 64 == 0 and (w <= 16) == (hw == S.GRAD_MAPS[1])
    what = f"conv {cin} -> {cout} [f32s LOACC, {name}, signed] 2x{h}x{w}"
    print(f"\n {what}: {'<2,2,2,2>' if cout % 128 == 0 else '<1,4,2,2>'}, {16 if w <= 16 else 32} wide")
    a32, ah, al = S.split_acts(name, cin, h, w, 2, True)
    enc = _encoded(a32, ah, al, torch.arange(2), dev, what)
    key = ("grad", cin, cout)
    ops.mixed_grid_launches()
    plain = ops.conv3x3_split(enc, blob(key), cout, relu=False).cpu()
    clamped = ops.conv3x3_split(enc, blob(key), cout, relu=True).cpu()
    assert ops.mixed_grid_launches() == 0
    _assert_same_bits(plain, S.reference(key, name, h, w, 2, True, relu=False), what + " relu=False")
    _assert_same_bits(clamped, plain.clamp_min(0), what + " relu=True against the clamp of relu=False")
    _assert_same_bits(clamped, S.reference(key, name, h, w, 2, True, relu=True), what + " relu=True")
