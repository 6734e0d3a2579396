"""The implicit-GEMM conv's mixed grid (conv3x3_igemm_mixed_kernel: 32-wide tiles plus 16-wide tiles down a right edge that
fills at most half a tile, 1 <= W % 32 <= 16, in one launch) against the plain grid of 32-wide tiles (GPU box only).

Each case is one layer through ops.conv3x3_relu, once with nqa_set_conv_variant + 256 (plain grids only) and once with
+ 512 (the mixed grid on every such map, whatever the block count), and asserts
  * that the second call did launch a mixed grid and the first did not (ops.mixed_grid_launches);
  * that the two outputs are BIT-EQUAL: both tile bodies contract in the same (chunk, tap) order into the same accumulator
    per pixel, so any difference is an indexing bug;
  * that the output agrees with F.conv2d + ReLU on the same rounded operands within the tolerance of
    tests/test_gpu_ops.py::test_conv3x3_relu for the mode (f16w: f16 activations, float weights -> the f16 bar).  The CPU
    reference of the 20-image cases is taken on the first and the last image only (the bit-equality covers every image).

Shapes (n, H, W, layer):
  20 x 24 x 48, conv4_1 (256 -> 512)   8-wave 256 x 256 tile (n = 20 passes its `blocks_big >= 192` gate); strip exactly full
  20 x 17 x 40, conv4_1                strip half outside the image, ragged bottom in both regions.  launch_conv's
                                       efficiency gate (eff_big * 1.05 >= eff_small) gives this map the 4-WAVE tile: 17 rows
                                       are 3 bands of 8 but 5 of 4, so the case runs the 4-wave form at 80 blocks per
                                       image; the next case puts the same edge through the 8-wave form
  20 x 23 x 40, conv4_1                8-wave form (23 rows: 3 bands of 8, 6 of 4), strip half outside, ragged bottom in both
   2 x  9 x 48, conv2_2 (128 -> 128)   4-wave 128 x 128 tile (edge form 8 rows x 16)
   2 x 13 x 80, conv4_2 (512 -> 512)   4-wave form, W % 32 == 16 behind two main columns
   2 x  7 x 33, conv2_2                one valid column in the strip
conv2_2 in f16 takes the register-weights kernel by default; + 32 puts it on the implicit GEMM (include/nqa.h).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DT = {"f16": torch.float16, "f32s": torch.float32, "f16w": torch.float16}
OUT_RTOL = {"f16": 1.2e-3, "f32s": 2e-5, "f16w": 1.2e-3}  # tests/test_gpu_ops.py OUT_RTOL (f16w stores f16)
BIG = [(7, 20, 24, 48), (7, 20, 17, 40), (7, 20, 23, 40)]   # (layer, n, H, W)
SMALL = [(3, 2, 9, 48), (8, 2, 13, 80), (3, 2, 7, 33)]
CASES = [(p, c) for c in BIG + SMALL for p in ("f16", "f32s")] + [("f16w", c) for c in BIG]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def packed(np_convs, dev):
    from nerf_qa_amd import ops
    return {p: ops.pack_vgg_weights(np_convs, p).to(dev) for p in DT}


_inputs, _refs = {}, {}


def _input(case):
    """Post-ReLU-like activations (half zeros, rest in [0, 2)), float32 NHWC; one array per case, shared by the modes."""
    if case not in _inputs:
        from nerf_qa_amd import ops, synth
        layer, n, h, w = case
        cin = ops.CONV_CIN[layer]
        a = synth.uniform(500 + layer + 7 * h + w, n * h * w * cin).astype(np.float32) * 4.0 - 2.0
        _inputs[case] = torch.from_numpy(a.reshape(n, h, w, cin)).clamp_min(0)
    return _inputs[case]


def _ref(case, prec, np_convs):
    """F.conv2d + ReLU of the rounded operands on images (0, n-1); computed once per (case, operand rounding)."""
    key = (case, "f16" if prec == "f16" else prec)
    if key not in _refs:
        layer, n = case[0], case[1]
        a = _input(case)[[0, n - 1]].to(DT[prec]).float()
        wq = torch.from_numpy(np_convs[layer][0])
        if prec == "f16":
            wq = wq.half().float()
        _refs[key] = F.relu(F.conv2d(a.permute(0, 3, 1, 2), wq, torch.from_numpy(np_convs[layer][1]), padding=1))
    return _refs[key]


def _run(a_dev, layer, blob, prec, variant, out=None):
    from nerf_qa_amd import ops
    ops.set_conv_variant(variant)
    try:
        ops.mixed_grid_launches()
        out = ops.conv3x3_relu(a_dev, layer, blob, prec, out=out)
        return out, ops.mixed_grid_launches()
    finally:
        ops.set_conv_variant(ops.DEFAULT_CONV_VARIANT)


@pytest.mark.parametrize("prec,case", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_mixed_grid_equals_plain_grid(prec, case, np_convs, packed, dev):
    from nerf_qa_amd import ops
    layer, n, h, w = case
    a = _input(case).to(DT[prec]).to(dev)
    inp = ops.split16_encode(a) if prec == "f32s" else a
    base = ops.DEFAULT_CONV_VARIANT | 32  # conv2_2 on the implicit GEMM in f16 too
    plain, n_plain = _run(inp, layer, packed[prec], prec, base | ops.CONV_PLAIN_GRID)
    # the second launch writes into an output of the caller's whose every byte is 0xFF (NaN in half, float and split16
    # records): it cannot be handed the block that still holds the first launch's result, so a skipped store shows
    fill = torch.empty_like(plain)
    fill.view(torch.uint8).fill_(0xFF)
    mixed, n_mixed = _run(inp, layer, packed[prec], prec, base | ops.CONV_MIXED_GRID, out=fill)
    records = prec == "f32s" and layer not in ops.TAP_LAYERS  # split16: NaN shows in the halves of a record
    assert mixed is fill and not torch.isnan(mixed.view(torch.float16) if records else mixed).any()
    assert (n_plain, n_mixed) == (0, 1), f"mixed grids launched: {n_plain} with + 256, {n_mixed} with + 512"
    assert plain.shape == mixed.shape and plain.dtype == mixed.dtype
    same = plain.view(torch.uint8).reshape(n, h, w, -1) == mixed.view(torch.uint8).reshape(n, h, w, -1)
    if not bool(same.all()):
        bad = (~same).any(dim=3).nonzero()
        raise AssertionError(f"layer {layer} [{prec}] {n}x{h}x{w}: {bad.shape[0]} pixels differ between the grids; first "
                             f"(image, row, column) {bad[:6].tolist()}; columns hit {sorted(set(bad[:, 2].tolist()))}")
    split = prec == "f32s" and layer not in ops.TAP_LAYERS
    got = (ops.split16_decode(mixed) if split else mixed.float())[[0, n - 1]].permute(0, 3, 1, 2).cpu()
    ref = _ref(case, prec, np_convs)
    scale = ref.abs().max().item() + 1e-30
    err = (got - ref).abs().max().item()
    print(f"\n layer {layer} [{prec}] {n}x{h}x{w}: max |mixed - conv2d| = {err / scale:.2e} of the map's scale")
    assert err <= OUT_RTOL[prec] * scale, f"max abs err {err:.3e} vs scale {scale:.3e} (rtol {OUT_RTOL[prec]})"


def test_stage4_of_a_1080p_batch_takes_the_mixed_grid_by_default(packed, dev):
    """conv4_2 on the 16 images of 135 x 240 that 8 pairs of 1080p leave at stage 4: 4352 blocks = 17 rounds of the chip
    on the plain grid, 3808 + 288 = 4096 = 16 rounds mixed (given at least 241 compute units), so the default rule takes
    the mixed grid; + 256 keeps the plain one.  Nothing is timed."""
    from nerf_qa_amd import ops
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert -(-4096 // cus) < -(-4352 // cus), f"{cus} compute units: the mixed grid saves no round on this device"
    a = torch.zeros(16, 135, 240, 512, dtype=torch.float16, device=dev)
    out, launched = _run(a, 8, packed["f16"], "f16", ops.DEFAULT_CONV_VARIANT)
    assert launched == 1 and out.shape == (16, 135, 240, 512)
    _, launched = _run(a, 8, packed["f16"], "f16", ops.DEFAULT_CONV_VARIANT | ops.CONV_PLAIN_GRID)
    assert launched == 0
    # a map whose last tile column is full has no edge strip
    _, launched = _run(a[:, :, :224].contiguous(), 8, packed["f16"], "f16", ops.DEFAULT_CONV_VARIANT)
    assert launched == 0
