"""Integer operands, bit-equal, through the conv instances no exact test reached (GPU box only).

The operands of tests/persistent_refs.py (activations in {0, 1, 2}, weights in {-1, 0, 1}, a bias in {-3 .. 3}): every
partial sum is an integer below 2^24, exact in float32 in any order, so the output must be BIT-EQUAL to relu(conv2d)
taken in float64 and rounded ONCE to the storage type.  Batches of 20 repeat three base images (only to pass launch_conv's
`blocks_big >= 192`).  Every output goes into an out= pre-filled with 0xFF bytes.  The instance of each case is read off
launch_conv by split_refs.vgg_instance / instance and asserted from the shape; ops.mixed_grid_launches() tells the grid.

f32 -- conv3x3_igemm_kernel<PrecF32, ...> on the 32x32x2 MFMA (the M16 == false body that `auto` runs below 128 x 128 and
A-DISTS on its patches), cases of split_refs.F32_CASES:
  conv1_2 (layer 1)  2x9x40, 2x5x13              <1,4,2,2, 32 | 16>: the 64-channel tile
  conv2_2 (layer 3)  2x9x48 + 256, + 512         <2,2,2,2, 32>: the 4-wave tile, plain grid and mixed grid
  conv4_2 (layer 8)  2x13x80 + 256               4-wave, Cin 512 (24 blocks of the big tile < 192)
  conv4_1 (layer 7)  2x11x13                     <2,2,2,2, 16>
  conv4_1            20x24x64                    <2,4,4,2, 32>: the 8-wave tile
  conv4_1            20x23x40 + 256              8-wave, plain grid, ragged right and bottom
  conv4_1            20x24x48 + 512              8-wave, mixed grid
bf16 -- the M16 body it shares with f16, on the seven cases of tests/test_gpu_conv_igemm_addr.py (CASES: 8-wave plain,
ragged and mixed, 4-wave at Cin 512, conv2_2 on the implicit GEMM plain and mixed, the 16-wide 4-wave instance); the
reference is rounded once to bfloat16 (integers above 256 round; tests/test_split_refs.py prints their share).
Conv variant 2 -- conv3x3_igemm_kernel<P, 2,4,2,4, 32>, the 8-wave 128 ch x 512 px tile (16 rows x 32), in f16, bf16 and
f32 on conv2_2 2x16x64 (full tiles), 2x29x40 (ragged both ways) and conv4_1 2x32x64; each passes launch_conv's
`eff_wide * 1.10 >= eff_small` (asserted), and the output must also be bit-equal to the default variant's on the same
input (the register-weights kernel for conv2_2 in the 16-bit modes, the 4-wave tile otherwise)."""
import pytest
import torch

import split_refs as S
from test_gpu_conv_igemm_addr import CASES as M16_CASES

pytestmark = pytest.mark.gpu

DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
BITS = {torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32}
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
    """blob(mode): the integer layers of split_refs.int_convs packed for the mode, made on first use."""
    made = {}

    def get(prec):
        if prec not in made:
            from nerf_qa_amd import ops
            made[prec] = ops.pack_vgg_weights(S.int_convs(), prec).to(dev)
        return made[prec]
    return get


def _assert_same_bits(got, ref, what, against="the float64 convolution"):
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype)
    same = got.view(BITS[got.dtype]) == ref.view(BITS[ref.dtype])
    print(f"   {what}: {int((~same).sum())} of {same.numel()} values differ from {against}; largest expected value "
          f"{ref.float().max().item():.0f}")
    if not bool(same.all()):
        elems = (~same).nonzero()
        bad = (~same).any(dim=3).nonzero()
        ch = sorted(set(elems[:, 3].tolist()))
        raise AssertionError(f"{what}: {bad.shape[0]} pixels differ from {against}, {int(torch.isnan(got.float()).sum())} values "
                             f"never written; first (image, row, column) {bad[:6].tolist()}; rows hit "
                             f"{sorted(set(bad[:, 1].tolist()))}; columns hit {sorted(set(bad[:, 2].tolist()))}; channels hit "
                             f"{ch[:8]} .. {ch[-1]}")


def _run(layer, n, h, w, prec, variant, blob, dev):
    """One ops.conv3x3_relu on image k = base[k % 3] under conv variant `variant` into an 0xFF-filled out=;
    (output on the CPU, mixed grids launched)."""
    from nerf_qa_amd import ops
    a = S.batch_of(S.int_base(layer, h, w), n).to(DT[prec]).to(dev)
    out = torch.empty((n, h, w, ops.CONV_COUT[layer]), dtype=DT[prec], device=dev)
    out.view(torch.uint8).fill_(0xFF)
    assert bool(torch.isnan(out).all())
    ops.set_conv_variant(variant)
    try:
        ops.mixed_grid_launches()
        res = ops.conv3x3_relu(a, layer, blob(prec), prec, out=out)
        launched = ops.mixed_grid_launches()
    finally:
        ops.set_conv_variant(ops.DEFAULT_CONV_VARIANT)
    assert res is out
    return out.cpu(), launched


def _ref(layer, n, h, w, prec):
    return S.batch_of(S.round_to(S.conv_ref(layer, h, w), DT[prec]), n)


@pytest.mark.parametrize("shape,extra,kernel,tw,want_mixed", S.F32_CASES, ids=_ID)
def test_f32_integer_operands_are_bit_exact(shape, extra, kernel, tw, want_mixed, blob, cus, dev):
    """conv3x3_igemm_kernel<PrecF32, `kernel`, `tw`> (or the mixed kernel of that tile): M16 == false, 32x32x2 MFMA."""
    from nerf_qa_amd import ops
    layer, n, h, w = shape
    assert S.vgg_instance(layer, n, h, w, extra, False, cus) == (kernel, tw, want_mixed)
    i = S.instance(ops.CONV_COUT[layer], n, h, w, 1, extra & 768, False, cus)
    assert i["narrow"] == (w <= 16) == (tw == 16) and i["mixed"] == bool(want_mixed)
    if kernel == "<2,4,4,2>":
        assert i["big"] and i["blocks_big"] >= 192 and i["eff_big"] * 1.05 >= i["eff_small"]
    elif kernel == "<2,2,2,2>":
        assert not i["big"] and (i["narrow"] or i["blocks_big"] < 192)
    else:
        assert ops.CONV_COUT[layer] == 64
    what = f"layer {layer} [f32] {n}x{h}x{w} + {extra}"
    print(f"\n {what}: {kernel}, {tw} wide, {want_mixed} mixed grids")
    got, launched = _run(layer, n, h, w, "f32", ops.DEFAULT_CONV_VARIANT | extra, blob, dev)
    assert launched == want_mixed, f"{what}: mixed grids launched: {launched}, expected {want_mixed}"
    _assert_same_bits(got, _ref(layer, n, h, w, "f32"), what)


@pytest.mark.parametrize("shape,extra,want_mixed", M16_CASES, ids=_ID)
def test_bf16_integer_operands_are_bit_exact(shape, extra, want_mixed, blob, cus, dev):
    """conv3x3_igemm_kernel<PrecBF16, ..., M16 = true> / the mixed kernel, as the f16 cases of test_gpu_conv_igemm_addr.py:
    <2,4,4,2> for the batches of 20, <2,2,2,2> otherwise, 16 wide at W = 13; + 32 keeps conv2_2 off the register-weights
    kernel."""
    from nerf_qa_amd import ops
    layer, n, h, w = shape
    i = S.instance(ops.CONV_COUT[layer], n, h, w, 1, extra & 768, False, cus)
    assert i["tile"] == ("<2,4,4,2>" if n == 20 else "<2,2,2,2>") and i["big"] == (n == 20) and i["mixed"] == bool(want_mixed)
    assert layer not in (3, 4) or extra & 32
    what = f"layer {layer} [bf16] {n}x{h}x{w} + {extra}"
    print(f"\n {what}: {i['tile']}, {i['tw']} wide, {want_mixed} mixed grids")
    got, launched = _run(layer, n, h, w, "bf16", ops.DEFAULT_CONV_VARIANT | extra, blob, dev)
    assert launched == want_mixed, f"{what}: mixed grids launched: {launched}, expected {want_mixed}"
    ref = _ref(layer, n, h, w, "bf16")
    _assert_same_bits(got, ref, what)


@pytest.mark.parametrize("prec", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("shape", S.WIDE_CASES, ids=_ID)
def test_wide_tile_is_bit_exact_and_equals_the_default_variant(shape, prec, blob, cus, dev):
    """Conv variant 2: conv3x3_igemm_kernel<P, 2,4,2,4, 32> (M16 in f16 / bf16, the 32x32x2 body in f32)."""
    from nerf_qa_amd import ops
    layer, n, h, w = shape
    i = S.instance(ops.CONV_COUT[layer], n, h, w, variant=2, cus=cus)
    assert i["tile"] == "<2,4,2,4>" and i["eff_wide"] * 1.10 >= i["eff_small"] and h >= 12 and w > 16 and ops.CONV_COUT[layer] >= 128
    what = f"layer {layer} [{prec}] {n}x{h}x{w}, conv variant 2"
    print(f"\n {what}: eff_wide {i['eff_wide']:.3f} x 1.10 >= eff_small {i['eff_small']:.3f}")
    wide, launched = _run(layer, n, h, w, prec, 2, blob, dev)
    assert launched == 0
    _assert_same_bits(wide, _ref(layer, n, h, w, prec), what)
    default, _ = _run(layer, n, h, w, prec, ops.DEFAULT_CONV_VARIANT, blob, dev)
    _assert_same_bits(wide, default, what, against="the default variant's output")
