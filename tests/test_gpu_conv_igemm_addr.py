"""The 16x16x32 stage loop of the implicit-GEMM conv (nqa_conv.hip conv3x3_igemm_tile) reads every fragment at a per-tile
lane address plus a constant: the halo rows are padded to a pitch of 8 pixels so that the LDS swizzle is the same under
every step the loop takes (kernel row, pixel group, buffer parity).  An error in that address algebra, in the padded halo's
DMA plan or in a buffer size is an indexing bug, so it is looked for where rounding cannot hide it (GPU box only).

Exact-integer cases.  The layer under test has weights in {-1, 0, 1} and a bias in {-3 .. 3}; the activations are in
{0, 1, 2}.  Every product and every partial sum is then an integer below 2^24 (at most 4608 terms of magnitude <= 2), exact
in float32 in ANY order, in one-term (f16) and in two-term (f16w: lo = 0, hi exact, a power-of-two scale) weights alike, so
the kernel's output must be BIT-EQUAL to relu(conv2d) taken in float64 and rounded to half once.  A batch of 20 exists
only to pass launch_conv's `blocks_big >= 192` gate to the 8-wave tile: its images repeat three distinct ones (image k =
base[k % 3]), so three float64 convolutions are the reference of all twenty.

Random-operand cases.  The same shapes and grids with the operands of tests/test_gpu_conv_edge_tiles.py (its _input, the
synthetic VGG weights) against F.conv2d + ReLU on the same rounded operands within that file's OUT_RTOL.

Shapes (layer, n, H, W) and the conv variant added to the default, as in tests/test_gpu_conv_edge_tiles.py:
  (7, 20, 24, 64)          8-wave 256 x 256 tile, 32 wide: two tile columns, three tile rows -- interior and all four borders
  (7, 20, 23, 40)  + 256   the plain grid: right tile column half outside the image, ragged bottom
  (7, 20, 24, 48)  + 512   the mixed grid: the 32-wide and the 16-wide 8-wave body in one launch
  (8,  2, 13, 80)          4-wave 128 x 128 tile (24 blocks of the big tile < 192), Cin 512: 48 stages in f16, 96 in f16w,
                           both parities of both buffers many times over; ragged bottom, right column half outside
  (3,  2,  9, 48)  + 32    conv2_2 on the implicit GEMM (by default it takes the register-weights kernel), 4-wave tile
  (3,  2,  9, 48)  + 32 + 512   ... and its mixed grid: the 16-wide 4-wave body as the edge strip
  (7,  2, 11, 13)          a map at most 16 wide: launch_conv gives it the 16-wide 4-WAVE instance (8 rows x 16).  No map
                           reaches the 16-wide 8-wave instance through launch_conv's plain grid: `big` requires W > 16, so
                           that body runs as the edge strip of the mixed grid only -- the + 512 case above.
Every case runs in f16 (NTERM = 1) and in f16w (f16 activations on two-term weights, NTERM = 2).
ops.mixed_grid_launches() tells which grid ran.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_conv_edge_tiles import DT, OUT_RTOL, _input as _random_input, _ref as _random_ref

pytestmark = pytest.mark.gpu

# (layer, n, H, W), variant bits added to the default, mixed grids expected
CASES = [((7, 20, 24, 64), 0, 0), ((7, 20, 23, 40), 256, 0), ((7, 20, 24, 48), 512, 1), ((8, 2, 13, 80), 0, 0),
         ((3, 2, 9, 48), 32, 0), ((3, 2, 9, 48), 32 + 512, 1), ((7, 2, 11, 13), 0, 0)]
PRECS = ("f16", "f16w")
INT_LAYERS = (3, 7, 8)
_ID = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)  # noqa: E731


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def int_convs(np_convs):
    """The synthetic VGG weights with integer layers 3, 7 and 8: weights in {-1, 0, 1}, bias in {-3 .. 3}."""
    from nerf_qa_amd import ops, synth
    convs = list(np_convs)
    for layer in INT_LAYERS:
        cout, cin = ops.CONV_COUT[layer], ops.CONV_CIN[layer]
        w = np.floor(synth.uniform(900 + layer, cout * cin * 9) * 3.0).clip(0, 2).astype(np.float32) - 1.0
        b = np.floor(synth.uniform(950 + layer, cout) * 7.0).clip(0, 6).astype(np.float32) - 3.0
        convs[layer] = (w.reshape(cout, cin, 3, 3), b)
    return convs


@pytest.fixture(scope="module")
def packed(np_convs, int_convs, dev):
    from nerf_qa_amd import ops
    return {(kind, p): ops.pack_vgg_weights(convs, p).to(dev)
            for kind, convs in (("int", int_convs), ("random", np_convs)) for p in PRECS}


_int_inputs, _int_refs = {}, {}


def _int_input(shape):
    """Activations in {0, 1, 2}, float32 NHWC; image k repeats base image k % 3."""
    if shape not in _int_inputs:
        from nerf_qa_amd import ops, synth
        layer, n, h, w = shape
        cin, nb = ops.CONV_CIN[layer], min(n, 3)
        a = np.floor(synth.uniform(700 + layer + 7 * h + w, nb * h * w * cin) * 3.0).clip(0, 2).astype(np.float32)
        _int_inputs[shape] = torch.from_numpy(a.reshape(nb, h, w, cin))[torch.arange(n) % nb].contiguous()
    return _int_inputs[shape]


def _int_ref(shape, int_convs):
    """relu(conv2d) in float64 of the distinct base images, rounded to half once; NHWC, expanded to the batch."""
    if shape not in _int_refs:
        layer, n = shape[0], shape[1]
        nb = min(n, 3)
        a = _int_input(shape)[:nb].double().permute(0, 3, 1, 2)
        wq, b = (torch.from_numpy(t).double() for t in int_convs[layer])
        ref = F.relu(F.conv2d(a, wq, b, padding=1))
        assert ref.max().item() < 2 ** 24 and bool((ref == ref.round()).all())
        _int_refs[shape] = ref.permute(0, 2, 3, 1).to(torch.float16)[torch.arange(n) % nb].contiguous()
    return _int_refs[shape]


def _run(a_dev, layer, blob, prec, extra, want_mixed):
    from nerf_qa_amd import ops
    ops.set_conv_variant(ops.DEFAULT_CONV_VARIANT | extra)
    try:
        ops.mixed_grid_launches()
        out = ops.conv3x3_relu(a_dev, layer, blob, prec)
        launched = ops.mixed_grid_launches()
    finally:
        ops.set_conv_variant(ops.DEFAULT_CONV_VARIANT)
    assert launched == want_mixed, f"mixed grids launched: {launched}, expected {want_mixed} (variant + {extra})"
    return out


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape,extra,want_mixed", CASES, ids=_ID)
def test_integer_operands_are_bit_exact(shape, extra, want_mixed, prec, int_convs, packed, dev):
    layer, n, h, w = shape
    out = _run(_int_input(shape).to(DT[prec]).to(dev), layer, packed["int", prec], prec, extra, want_mixed)
    ref = _int_ref(shape, int_convs)
    assert out.shape == ref.shape and out.dtype == torch.float16
    same = out.cpu().view(torch.int16) == ref.view(torch.int16)
    print(f"\n layer {layer} [{prec}] {n}x{h}x{w} + {extra}: {int((~same).sum())} of {same.numel()} values differ; "
          f"largest expected value {ref.max().item():.0f}")
    if not bool(same.all()):
        bad = (~same).any(dim=3).nonzero()
        ch = sorted(set((~same).nonzero()[:, 3].tolist()))
        raise AssertionError(f"layer {layer} [{prec}] {n}x{h}x{w} + {extra}: {bad.shape[0]} pixels differ from the float64 "
                             f"convolution; first (image, row, column) {bad[:6].tolist()}; rows hit "
                             f"{sorted(set(bad[:, 1].tolist()))}; columns hit {sorted(set(bad[:, 2].tolist()))}; channels "
                             f"hit {ch[:8]} .. {ch[-1]}")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape,extra,want_mixed", CASES, ids=_ID)
def test_random_operands_match_conv2d(shape, extra, want_mixed, prec, np_convs, packed, dev):
    layer, n, h, w = shape
    out = _run(_random_input(shape).to(DT[prec]).to(dev), layer, packed["random", prec], prec, extra, want_mixed)
    got = out.float()[[0, n - 1]].permute(0, 3, 1, 2).cpu()
    ref = _random_ref(shape, prec, np_convs)
    scale = ref.abs().max().item() + 1e-30
    err = (got - ref).abs().max().item()
    print(f"\n layer {layer} [{prec}] {n}x{h}x{w} + {extra}: max |out - conv2d| = {err / scale:.2e} of the map's scale")
    assert err <= OUT_RTOL[prec] * scale, f"max abs err {err:.3e} vs scale {scale:.3e} (rtol {OUT_RTOL[prec]})"
