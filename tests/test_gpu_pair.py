"""DISTS and A-DISTS of a batch from ONE VGG pyramid (nqa_adists_dists_forward, ops.adists_dists_forward,
pair.score_pair, video.score_video(shared_pyramid=True)) on the GPU.

The A-DISTS half must be bit-identical to the standalone call (the same launches in the same order); the DISTS half is
held to the reference's goldens, to the CPU oracle and to the standalone DISTS in the same precision.  In "f32" and
"f32s" -- the only modes the pair runs in under A-DISTS' `auto` -- nqa_dists_forward fuses no tap into a conv kernel
(conv1_pool_fusable / conv_pool_fusable ask for 16-bit kernels), so both paths run stats_nchw, conv1_1 / the fused
stage 1, conv3x3, pool_stats, stats_nhwc and finalize with the same partial-sum plans in the same order: there the
DISTS half is bit-identical to the standalone too, and the tests assert that wherever nqa_dists_fused_taps confirms it.
"""
import glob
import os
import warnings

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
SCORE_TOL = 1e-4      # the project's bar (tests/test_gpu_adists.py SCORE_TOL, tests/test_gpu_dists.py SCORE_TOL)
S_TOL = 5e-4          # tests/test_gpu_dists.py::test_dists_vs_golden, max |S - golden S| for "f32" and "f32s"
PRECS = ("f32", "f32s")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def packed(np_convs, dev):
    from nerf_qa_amd import ops
    return {p: ops.pack_vgg_weights(np_convs, p).to(dev) for p in PRECS}


def _case(path, dev):
    from nerf_qa_amd import synth
    g = np.load(path)
    x, y = synth.frame_batch([int(s) for s in g["seeds"]], int(g["h"]), int(g["w"]), [str(k) for k in g["kinds"]])
    return g, torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)


def _golden(prefix, sizes):
    paths = [os.path.join(GOLDEN, f"{prefix}_{s}.npz") for s in sizes]
    return pytest.mark.parametrize("path", paths, ids=[os.path.basename(p)[:-4] for p in paths])


def _models(dev, dists_cls=None, **kw):
    from nerf_qa_amd.ADISTS import ADISTS
    from nerf_qa_amd.DISTS_pytorch import DISTS
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return (dists_cls or DISTS)(**kw).to(dev).eval(), ADISTS().to(dev).eval()


def _frames(seeds, h, w, dev):
    from nerf_qa_amd import synth
    x, y = synth.frame_batch(list(seeds), h, w)
    return torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)


# ---- the C entry point through ops ------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@_golden("adists", ("20x20", "64x64", "97x131", "256x256", "352x336"))
def test_adists_half_bit_exact_and_vs_golden(path, prec, packed, dev):
    from nerf_qa_amd import ops
    g, x, y = _case(path, dev)
    d, s1, s2 = ops.adists_dists_forward(x, y, packed[prec], prec)
    d0 = ops.adists_forward(x, y, packed[prec], prec)
    assert s1.shape == s2.shape == (x.shape[0], 1475)
    err = np.abs((1 - d).cpu().numpy() - g["score"]).max()
    print(f"\n{os.path.basename(path)} [{prec}] A-DISTS half |d golden|={err:.2e} equal={torch.equal(d, d0)}")
    assert torch.equal(d, d0)
    assert err <= SCORE_TOL


@pytest.mark.parametrize("prec", PRECS)
@_golden("amap", ("20x20", "64x64", "97x131"))
def test_adists_map_bit_exact_and_vs_golden(path, prec, packed, dev):
    from nerf_qa_amd import ops
    g, x, y = _case(path, dev)
    d, s1, s2, m = ops.adists_dists_forward(x, y, packed[prec], prec, with_map=True)
    d0, m0 = ops.adists_forward(x, y, packed[prec], prec, with_map=True)
    err = np.abs(m.cpu().numpy() - g["map"]).max()
    print(f"\n{os.path.basename(path)} [{prec}] map |d golden|={err:.2e}")
    assert torch.equal(d, d0) and torch.equal(m, m0)
    assert m.shape == g["map"].shape and err <= 1e-4
    # asking for the map changes neither half
    d1, t1, t2 = ops.adists_dists_forward(x, y, packed[prec], prec)
    assert torch.equal(d, d1) and torch.equal(s1, t1) and torch.equal(s2, t2)


@pytest.mark.parametrize("prec", PRECS)
@_golden("dists", ("20x20", "64x64", "97x131", "256x256", "256x341"))
def test_dists_half_vs_golden(path, prec, packed, alpha_beta, dev):
    from nerf_qa_amd import ops
    g, x, y = _case(path, dev)
    _, s1, s2 = ops.adists_dists_forward(x, y, packed[prec], prec)
    alpha, beta = alpha_beta
    score = ops.dists_score(s1, s2, alpha.to(dev), beta.to(dev)).cpu().numpy()
    d = np.abs(score - g["score"]).max()
    e1 = np.abs(s1.cpu().numpy() - g["s1"]).max()
    e2 = np.abs(s2.cpu().numpy() - g["s2"]).max()
    print(f"\n{os.path.basename(path)} [{prec}] DISTS half |dscore|={d:.2e} |dS1|={e1:.2e} |dS2|={e2:.2e}")
    assert d <= SCORE_TOL
    assert e1 <= S_TOL and e2 <= S_TOL


@pytest.mark.parametrize("prec", PRECS)
def test_both_halves_against_the_cpu_oracle_on_an_odd_size(prec, packed, oracle_convs, alpha_beta, dev):
    """75x118, B=3, three distortion kinds: a size no golden covers (every stage ragged, stages 3-5 on the global branch)."""
    from nerf_qa_amd import ops, synth
    from oracle import adists_oracle, dists_oracle
    xn, yn = synth.frame_batch([21, 22, 23], 75, 118, list(synth.KINDS[1:4]))
    x, y = torch.from_numpy(xn), torch.from_numpy(yn)
    alpha, beta = alpha_beta
    want = dists_oracle.dists(x, y, oracle_convs, alpha, beta)
    awant = adists_oracle.adists(x, y, oracle_convs)
    d, s1, s2 = ops.adists_dists_forward(x.to(dev), y.to(dev), packed[prec], prec)
    got = ops.dists_score(s1, s2, alpha.to(dev), beta.to(dev)).cpu()
    err, aerr = (got - want).abs().max().item(), ((1 - d).cpu() - awant).abs().max().item()
    print(f"\n75x118 [{prec}] vs oracle: DISTS half |d|={err:.2e}  A-DISTS half |d|={aerr:.2e}")
    assert err <= SCORE_TOL and aerr <= SCORE_TOL


@pytest.mark.parametrize("prec", PRECS)
def test_dists_half_against_the_standalone_dists(prec, packed, alpha_beta, dev):
    """256x256 B=8 against ops.dists_forward in the same precision.  nqa_dists_forward fuses no tap in f32 / f32s (see the
    module docstring; confirmed here through nqa_dists_fused_taps), so the sums come from the same kernels in the same
    order and the similarities are bit-identical, not merely within the bar."""
    from nerf_qa_amd import ops
    x, y = _frames(range(30, 38), 256, 256, dev)
    alpha, beta = (t.to(dev) for t in alpha_beta)
    _, s1, s2 = ops.adists_dists_forward(x, y, packed[prec], prec)
    t1, t2 = ops.dists_forward(x, y, packed[prec], prec)
    diff = (ops.dists_score(s1, s2, alpha, beta) - ops.dists_score(t1, t2, alpha, beta)).abs().max().item()
    ds = max((s1 - t1).abs().max().item(), (s2 - t2).abs().max().item())
    fused = ops.dists_fused_taps(8, 256, 256, prec)
    print(f"\n256x256 B=8 [{prec}] pair vs standalone DISTS: max |dscore|={diff:.3e} max |dS|={ds:.3e} fused taps={fused}")
    assert diff <= SCORE_TOL
    if fused == ():
        assert torch.equal(s1, t1) and torch.equal(s2, t2)


def test_bit_repeatable(packed, dev):
    from nerf_qa_amd import ops
    x, y = _frames(range(5), 97, 131, dev)
    first = ops.adists_dists_forward(x, y, packed["f32s"], "f32s")
    for _ in range(9):
        again = ops.adists_dists_forward(x, y, packed["f32s"], "f32s")
        assert all(torch.equal(a, b) for a, b in zip(first, again))


# ---- pair.score_pair ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,h,w", [(3, 64, 72), (2, 160, 144), (4, 512, 512)], ids=["3x64x72", "2x160x144", "4x512x512_two_streams"])
def test_score_pair_against_the_modules(b, h, w, dev):
    import nerf_qa_amd
    from nerf_qa_amd.ADISTS.ADISTS import TWO_STREAM_MIN_PAIRS, TWO_STREAM_MIN_PIXELS
    from nerf_qa_amd.DISTS_pytorch import DISTS
    dm, am = _models(dev)
    x, y = _frames(range(40, 40 + b), h, w, dev)
    if b == 4:
        assert b >= TWO_STREAM_MIN_PAIRS and h * w >= TWO_STREAM_MIN_PIXELS  # the two-stream route of ADISTS._score
    prec = am.precision_for(h, w)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = DISTS(precision=prec).to(dev).eval()
    with torch.no_grad():
        ds, ad = nerf_qa_amd.score_pair(dm, am, x, y)
        want_a, want_d = am(x, y, as_loss=False), ref(x, y)
        assert ad.shape == want_a.shape == (b,) and ad.dtype == want_a.dtype and torch.equal(ad, want_a)
        assert ds.shape == want_d.shape and ds.dtype == want_d.dtype
        err = (ds - want_d).abs().max().item()
        ds_avg, loss = nerf_qa_amd.score_pair(dm, am, x, y, batch_average=True, as_loss=True)
        assert loss.shape == () and torch.equal(loss, am(x, y))
        err_avg = (ds_avg - ref(x, y, batch_average=True)).abs().item()
        assert ds_avg.shape == ()
        print(f"\nscore_pair {b}x{h}x{w} [{prec}]: DISTS half vs DISTS(precision={prec!r}) |d|={err:.2e} (mean {err_avg:.2e})")
        assert err <= SCORE_TOL and err_avg <= SCORE_TOL
        if b <= 3:
            _, amap = nerf_qa_amd.score_pair(dm, am, x, y, as_map=True)
            want_m = am(x, y, as_loss=False, as_map=True)
            assert amap.shape == (b, b, h, w) and torch.equal(amap, want_m)


@pytest.mark.parametrize("variant,flags", [("original", "off"), ("original", "relu+w_sum_detach"), ("softmax", "off")])
def test_variants_and_alpha_beta_gradients(variant, flags, dev):
    """DISTS_pt_original / DISTS_pt_softmax through score_pair: the value of their own forward in the pair's precision and
    the same gradients on alpha and beta (relative tolerance of tests/test_gpu_module.py::test_alpha_beta_gradients:
    1e-4 * max(1, |g|))."""
    import importlib
    import nerf_qa_amd
    from nerf_qa_amd.config import config
    mod = importlib.import_module(f"nerf_qa_amd.DISTS_pytorch.DISTS_pt_{variant}")
    old = config().dists_weight_norm
    config().dists_weight_norm = flags
    try:
        dm, am = _models(dev, mod.DISTS)
        x, y = _frames((7, 8, 9), 48, 56, dev)
        prec = am.precision_for(48, 56)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ref = mod.DISTS(precision=prec).to(dev).eval()
        ds, _ = nerf_qa_amd.score_pair(dm, am, x, y)
        want = ref(x, y)
        assert ds.requires_grad and ds.shape == want.shape
        err = (ds - want).abs().max().item()
        ds.sum().backward()
        want.sum().backward()
        worst = 0.0
        for got_g, ref_g in ((dm.alpha.grad, ref.alpha.grad), (dm.beta.grad, ref.beta.grad)):
            assert got_g is not None and ref_g is not None
            rel = ((got_g - ref_g).abs() / ref_g.abs().clamp(min=1.0)).max().item()
            worst = max(worst, rel)
        print(f"\nDISTS_pt_{variant} [{flags}] pair vs forward |d|={err:.2e}  alpha/beta grad rel err={worst:.2e}")
        assert err <= SCORE_TOL
        assert worst <= 1e-4
        one, _ = nerf_qa_amd.score_pair(dm, am, x[:1], y[:1])  # the variants' squeeze(): 0-d for one pair
        assert one.shape == ref(x[:1], y[:1]).shape == ()
    finally:
        config().dists_weight_norm = old


def test_base_module_alpha_beta_gradients(dev):
    import nerf_qa_amd
    from nerf_qa_amd.DISTS_pytorch import DISTS
    dm, am = _models(dev)
    x, y = _frames((7, 8), 48, 48, dev)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = DISTS(precision=am.precision_for(48, 48)).to(dev).eval()
    ds, _ = nerf_qa_amd.score_pair(dm, am, x, y)
    want = ref(x, y)
    assert ds.requires_grad
    ds.sum().backward()
    want.sum().backward()
    for got_g, ref_g in ((dm.alpha.grad, ref.alpha.grad), (dm.beta.grad, ref.beta.grad)):
        assert ((got_g - ref_g).abs() / ref_g.abs().clamp(min=1.0)).max().item() <= 1e-4


def test_refusals(dev):
    import nerf_qa_amd
    from nerf_qa_amd.ADISTS import ADISTS
    from nerf_qa_amd.DISTS_pytorch import DISTS
    x, y = _frames((1, 2), 64, 64, dev)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        dm, am = DISTS(vgg16_path="synth:1234").to(dev).eval(), ADISTS(vgg16_path="synth:7").to(dev).eval()
        named = DISTS(vgg16_path="synth:7", precision="f16").to(dev).eval()
    for _ in range(2):  # (the verdict is remembered: the second call refuses as well)
        with pytest.raises(nerf_qa_amd.NqaError, match="different VGG-16 weights"):
            nerf_qa_amd.score_pair(dm, am, x, y)
    with pytest.raises(ValueError, match=r"'f32'.*'f16'"):
        nerf_qa_amd.score_pair(named, am, x, y)
    good = DISTS(vgg16_path="synth:7").to(dev).eval()
    with pytest.raises(ValueError, match="separately"):
        nerf_qa_amd.score_pair(good, am, x.clone().requires_grad_(True), y)
    with torch.no_grad():
        ds, ad = nerf_qa_amd.score_pair(good, am, x, y)
        assert torch.equal(ad, am(x, y, as_loss=False))


def test_score_pair_captures_into_a_hip_graph_and_replays(dev):
    import nerf_qa_amd
    dm, am = _models(dev)
    gen = torch.Generator(device=dev).manual_seed(11)
    frames = [torch.rand(2, 3, 128, 160, device=dev, generator=gen) for _ in range(4)]
    x, y = frames[0].clone(), frames[1].clone()  # the graph's static inputs
    with torch.no_grad():
        nerf_qa_amd.score_pair(dm, am, x, y)  # the one eager call: weights compared and packed
        torch.cuda.synchronize(dev)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):  # warm-up on a side stream, as torch asks before a capture (workspace of that stream)
            nerf_qa_amd.score_pair(dm, am, x, y)
        torch.cuda.current_stream(dev).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out_d, out_a = nerf_qa_amd.score_pair(dm, am, x, y)
        for a, b in ((frames[0], frames[1]), (frames[2], frames[3]), (frames[3], frames[0])):
            x.copy_(a)
            y.copy_(b)
            graph.replay()
            torch.cuda.synchronize(dev)
            got_d, got_a = out_d.clone(), out_a.clone()
            want_d, want_a = nerf_qa_amd.score_pair(dm, am, a, b)
            assert torch.equal(got_d, want_d) and torch.equal(got_a, want_a)


# ---- video.score_video(shared_pyramid=True) ------------------------------------------------------------------------
def test_video_shared_pyramid_64x96(dev):
    """20 frames of 64x96 in batches of 8 (the last batch is ragged): the A-DISTS columns are those of the two-pass call to
    the character, the DISTS columns agree per frame with the two-pass call in the pair's precision, and both agree with
    the CPU oracle as tests/test_gpu_video10k.py::test_video_64x96_against_the_oracle asks."""
    from nerf_qa_amd import synth, video
    from nerf_qa_amd.DISTS_pytorch import DISTS
    from oracle import adists_oracle, dists_oracle
    H, W, B, N = 64, 96, 8, 20
    dm, am = _models(dev)
    prec = am.precision_for(H, W)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        named = DISTS(precision=prec).to(dev).eval()
    ref, ren = video.synthetic_frames(range(N), H, W, dev)
    two = video.score_video(ref, ren, named, am, batch_size=B, return_frame_scores=True)
    one = video.score_video(ref, ren, dm, am, batch_size=B, return_frame_scores=True, shared_pyramid=True)
    assert list(one) == list(two)  # the same columns in the same order
    for col in two:
        if "A-DISTS" in col or col in ("frame_count", "frame_bias_adists"):
            assert str(one[col]) == str(two[col]), col
    fa, fd = one["_frame_scores"]["A-DISTS"], one["_frame_scores"]["DISTS"]
    assert fa.dtype == fd.dtype == np.float32 and fa.shape == fd.shape == (N,)
    assert np.array_equal(fa, two["_frame_scores"]["A-DISTS"])
    err = np.abs(fd - two["_frame_scores"]["DISTS"]).max()
    convs = dists_oracle.convs_from_numpy(synth.vgg16_weights(1234))
    want = dists_oracle.dists(ref.cpu(), ren.cpu(), convs, dm.alpha.detach().cpu(), dm.beta.detach().cpu()).numpy()
    awant = adists_oracle.adists(ref.cpu(), ren.cpu(), convs).numpy()
    oerr, aerr = np.abs(fd - want).max(), np.abs(fa - awant).max()
    print(f"\nvideo 64x96 x{N} shared pyramid [{prec}]: DISTS vs two-pass |d|={err:.2e}; vs oracle DISTS {oerr:.2e} A-DISTS {aerr:.2e}")
    assert err <= SCORE_TOL and oerr <= SCORE_TOL and aerr <= SCORE_TOL
    for col in ("DISTS", "DISTS_std", "DISTS_min", "DISTS_max"):
        assert abs(float(one[col]) - float(two[col])) <= SCORE_TOL


def test_video_shared_pyramid_with_a_policy_on_uint8_frames(dev):
    from nerf_qa_amd import video
    from nerf_qa_amd.DISTS_pytorch import DISTS
    N, B = 11, 4
    gen = torch.Generator(device=dev).manual_seed(3)
    ref = torch.randint(0, 256, (N, 120, 200, 3), dtype=torch.uint8, device=dev, generator=gen)
    noise = torch.randint(-20, 21, ref.shape, device=dev, generator=gen)
    ren = (ref.int() + noise).clamp_(0, 255).to(torch.uint8)
    dm, am = _models(dev)
    prec = am.precision_for(256, 256)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        named = DISTS(precision=prec).to(dev).eval()
    two = video.score_video(ref, ren, named, am, batch_size=B, policy="interp256", return_frame_scores=True)
    one = video.score_video(ref, ren, dm, am, batch_size=B, policy="interp256", return_frame_scores=True,
                            shared_pyramid=True)
    assert list(one) == list(two)
    for col in two:
        if "A-DISTS" in col or col in ("frame_count", "frame_bias_adists"):
            assert str(one[col]) == str(two[col]), col
    err = np.abs(one["_frame_scores"]["DISTS"] - two["_frame_scores"]["DISTS"]).max()
    print(f"\nvideo interp256 x{N} shared pyramid [{prec}]: DISTS vs two-pass |d|={err:.2e}")
    assert err <= SCORE_TOL
