"""tests/split_refs.py without a GPU: for every case of tests/test_gpu_conv_split_exact.py the operands encode to exactly
the intended (hi, lo) halves, every output is a multiple of the set's quantum and sum |terms| + |bias| stays below
quantum x 2^24 -- so the float64 reference IS the kernel's float32 arithmetic in any order -- and the reference has power:
a kernel that keeps hi*hi only, drops a cross term, doubles one or pairs the halves wrongly (al*bl + ah*bh) differs from it
in nearly every output.  The share in which the full four-term product differs is printed, not bounded: the reference is
the kernel's three-term arithmetic, not a better one.  Every figure is printed."""
import pytest
import torch

import persistent_refs as P
import split_refs as S

_ID = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)  # noqa: E731
VGG_KEYS = sorted({(("vgg", c[0][0]), name, c[0][2], c[0][3], min(c[0][1], 3), False) for c in S.VGG_CASES for name in S.SETS})
RING_KEY = (("vgg", 2), "normal", P.H, P.W, 3, False)  # the persistent-regime case of conv3x3_regw_split_kernel
GRAD_KEYS = [(("grad", cin, cout), name, h, w, 2, True) for cin, cout in S.GRAD_SHAPES for h, w in S.GRAD_MAPS for name in S.SETS]


def test_weights_hit_every_position_and_scale_by_512():
    from nerf_qa_amd import ops
    keys = [("vgg", layer) for layer in S.SPLIT_LAYERS] + [("grad", cin, cout) for cin, cout in S.GRAD_SHAPES]
    for key in keys:
        w32, wh, wl, bias = S.weights_of(key)
        cov = S.weight_coverage(key)
        print(f"\n {key}: {cov}")
        assert 2.0 ** S.weight_scale_exp(w32) == S.SCALE and float(abs(w32).max()) == 1.0 + S.WQ
        assert cov["per_channel"] <= S.WEIGHT_TERMS and cov["taps"] == 9 and cov["chunks"] == cov["of_chunks"]
        assert cov["slab_positions"] > 0.99 and 0.3 < cov["opposite_signs"] < 0.7  # sign(hi) != sign(lo) does occur
        assert set(wh.unique().tolist()) == {-1.0, 0.0, 1.0} and set((wl / S.WQ).unique().tolist()) == {-1.0, 0.0, 1.0}
        assert set(bias.unique().tolist()) <= set(range(-3, 4))
        if key[0] == "vgg":
            assert w32.shape[:2] == (ops.CONV_COUT[key[1]], ops.CONV_CIN[key[1]])
    a = {k: S.weights_of(("grad",) + k)[0] for k in S.GRAD_SHAPES}
    assert not (a[128, 128][:64] == a[128, 64]).all()  # tensors of their own, not slices of one another


@pytest.mark.parametrize("key", VGG_KEYS + [RING_KEY] + GRAD_KEYS, ids=lambda k: "-".join(_ID(v) for v in k))
def test_the_reference_is_exact_and_has_power(key):
    wkey, name, h, w, nb, signed = key
    a = S.analysis(*key)  # asserts the encode model, the quantum and the bound
    print(f"\n {wkey} [{name}{', signed' if signed else ''}] {nb}x{h}x{w}: sum |terms| + |bias| <= {a['bound']:.2f} < "
          f"{S.SETS[name]['bound']:.0f}, largest |pre-activation| {a['largest']:.4f}, {a['positive']:.2f} of them positive; "
          f"{a['subnormal_lo']:.2f} of the non-zero activations have a subnormal lo")
    for mutant, share in a["mutants"].items():
        print(f"   {mutant}: {share:.4f} of the outputs differ")
        assert share >= 0.5, (mutant, share)
    print(f"   the full four-term product: {a['four_term']:.4f} of the outputs differ")
    assert (a["subnormal_lo"] > 0.3) if name == "small" else (a["subnormal_lo"] == 0.0)
    assert 0.3 < a["positive"] < 0.7  # a ReLU leaves about half of them: no map of zeros
    a32, ah, al = S.split_acts(name, S.weights_of(wkey)[0].shape[1], h, w, nb, signed)
    assert bool((ah < 0).any()) == signed and (not signed or bool(((ah > 0) & (al < 0)).any()))
    ref = S.reference(wkey, name, h, w, nb, signed, relu=True)
    assert torch.equal(ref, S.reference(wkey, name, h, w, nb, signed, relu=False).clamp_min(0))
    hi, lo = S.records(ref)
    err = (hi.double() + lo.double() - ref.double()).abs().max().item()
    print(f"   split16 records of the output: |hi + lo - v| <= {err:.3e}; {float((lo.float().abs() < S.MIN_NORMAL_HALF)[lo != 0].float().mean()):.2f} "
          f"of the non-zero lo halves are subnormal")
    assert err <= 2.0 ** -22 * max(1.0, ref.abs().max().item())  # (lo rounds a 13-bit residual to 11 bits)


@pytest.mark.parametrize("cus", P.CU_COUNTS)
def test_every_case_reaches_the_instance_it_names(cus):
    for cases, split in ((S.VGG_CASES, True), (S.F32_CASES, False)):
        for (layer, n, h, w), extra, kernel, tw, mixed in cases:
            assert S.vgg_instance(layer, n, h, w, extra, split, cus) == (kernel, tw, mixed), (layer, n, h, w, extra, split)
    from nerf_qa_amd import ops
    for layer, n, h, w in S.WIDE_CASES:
        i = S.instance(ops.CONV_COUT[layer], n, h, w, variant=2, cus=cus)
        assert i["tile"] == "<2,4,2,4>" and i["eff_wide"] * 1.10 >= i["eff_small"], i
    i = S.instance(512, 3, 40, 70, cus=cus, edge=256)  # what the operator tests reach: 90 blocks of the 8-wave tile
    assert i["blocks_big"] == 90 and not i["big"]
    r = P.regime("regw_split", 2, 9, 40, cus, 2)
    assert r["most"] == 1 or cus < 24, r  # one unit per block wherever the 24 units find 24 CUs


def test_integer_layers_of_the_float_cases_are_exact():
    from nerf_qa_amd import ops
    shapes = sorted({c[0][:1] + c[0][2:] for c in S.F32_CASES} | {(c[0], c[2], c[3]) for c in S.WIDE_CASES} | {(3, 9, 48), (7, 24, 64)})
    for layer, h, w in shapes:
        bound, ref = S.partial_sum_bound(layer, h, w), S.conv_ref(layer, h, w)
        print(f"\n layer {layer} {h}x{w}: partial sums <= {bound:.0f} < 2^24, largest output {ref.max().item():.0f}")
        assert bound < 2 ** 24 and ref.shape == (3, h, w, ops.CONV_COUT[layer]) and float((ref > 0).double().mean()) > 0.2
        assert torch.equal(S.round_to(ref, torch.float32).double(), ref)
        rounds = float((S.round_to(ref, torch.bfloat16).double() != ref).double().mean())
        print(f"   {rounds:.4f} of the outputs round in bfloat16 (integers above 256)")
