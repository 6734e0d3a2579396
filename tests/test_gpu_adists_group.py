"""A-DISTS of K renders against one reference from ONE shared pyramid per group (nqa_adists_forward_group through
ADISTS.forward_group, pair.score_group and video.score_videos) on the GPU.

Bounds.  Pair by pair against the CPU oracle (oracle/adists_oracle.py): |d(1 - D)| <= SCORE_TOL = 1e-4, the bar of
tests/test_gpu_adists.py -- after the PAIRWISE module of the same precision has been held to the same bar on the same
inputs (a pair it misses would be a knife-edge pair, DESIGN.md 4.4, that the group path cannot be judged by; none of the
pairs below is one: every shape runs on its first seed).  Against the pairwise module of the same precision the group
path runs the same convolutions on the same images and the same window and chain arithmetic; what differs is the split of
the fp64 statistics and entropy sums into blocks, so D agrees to NAMED_TOL = 5e-6, the project's named-mode bound
(tests/test_gpu_fullsize_golden.py).  The DISTS half of score_group is held as tests/test_gpu_group.py holds
DISTS.forward_group: against float64 similarities of the module's own taps, at most twice the pairwise path's distance,
floored at 2^-22.
"""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SCORE_TOL = 1e-4      # tests/test_gpu_adists.py SCORE_TOL for "f32" and "f32s"
NAMED_TOL = 5e-6      # tests/test_gpu_fullsize_golden.py: explicitly named "f32s" / "f32" scores
FLOOR = 2.0 ** -22
# (R, K, H, W) per precision; f32s only where the default runs it (frames of at least 128 x 128 pixels)
CASES = [("f32", (1, 1, 17, 23)), ("f32", (2, 3, 33, 47)), ("f32", (1, 5, 130, 95)),
         ("f32s", (2, 2, 144, 128)), ("f32s", (1, 3, 130, 160))]
_ids = lambda c: "%s_R%dK%d_%dx%d" % ((c[0],) + c[1])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def models(dev):
    from nerf_qa_amd.ADISTS import ADISTS
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return {p: ADISTS(precision=p).to(dev).eval() for p in ("f32", "f32s")}


@pytest.fixture(scope="module")
def dists_models(dev):
    from nerf_qa_amd.DISTS_pytorch import DISTS
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return {p: DISTS(precision=p).to(dev).eval() for p in ("f32", "f32s")}


def _group(R, K, h, w):
    """ref (R,3,h,w) and renders (R,K,3,h,w) as tests/test_gpu_group.py::_group builds them: noise, blur and one
    synth.NERF_KINDS kind in every group (K = 1: noise; K = 2: blur and a NeRF-like frame)."""
    from nerf_qa_amd import synth
    kinds = {1: ("noise10",), 2: ("blur", "nerf_white"), 3: ("noise10", "blur", "nerf_float"),
             5: ("noise02", "noise10", "blur", "nerf_black", "nerf_grad")}[K]
    refs, rens = [], []
    for r in range(R):
        seed = 300 + 17 * r + h
        refs.append(synth.frame_pair(seed, h, w, "noise10")[0])
        rens.append(np.stack([synth.frame_pair(seed, h, w, k)[1][0] for k in kinds]))
    return torch.from_numpy(np.concatenate(refs)), torch.from_numpy(np.stack(rens))


_ORACLE = {}


def _oracle(shape, oracle_convs):
    """(ref, renders, 1 - D (R,K)) of the CPU oracle, pair by pair; computed once per shape and left unchanged."""
    if shape not in _ORACLE:
        from oracle import adists_oracle
        R, K, h, w = shape
        ref, ren = _group(*shape)
        want = adists_oracle.adists(ref.repeat_interleave(K, 0), ren.flatten(0, 1), oracle_convs, as_loss=False)
        _ORACLE[shape] = (ref, ren, want.view(R, K))
    return _ORACLE[shape]


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_forward_group_against_the_cpu_oracle(case, models, oracle_convs, dev):
    prec, shape = case
    R, K, h, w = shape
    ref, ren, want = _oracle(shape, oracle_convs)
    m = models[prec]
    assert m.precision_for(h, w) == prec
    with torch.no_grad():
        pairwise = m(ref.repeat_interleave(K, 0).to(dev), ren.flatten(0, 1).to(dev), as_loss=False).view(R, K)
        got = m.forward_group(ref.to(dev), ren.to(dev))
    dp = (pairwise.cpu() - want).abs().max().item()
    dg = (got.cpu() - want).abs().max().item()
    print(f"\nadists forward_group {shape} [{prec}] vs oracle: pairwise {dp:.2e} group {dg:.2e}")
    assert dp <= SCORE_TOL, "a knife-edge pair (DESIGN.md 4.4): the pairwise module misses the oracle; take the next seed"
    assert got.shape == (R, K) and got.dtype == torch.float32
    assert dg <= SCORE_TOL


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_forward_group_agrees_with_the_pairwise_module(case, models, dev):
    prec, shape = case
    R, K, h, w = shape
    ref, ren = (t.to(dev) for t in _group(*shape))
    m = models[prec]
    with torch.no_grad():
        pairwise = m(ref.repeat_interleave(K, 0), ren.flatten(0, 1), as_loss=False)
        got = m.forward_group(ref, ren)
        again = m.forward_group(ref, ren)
    d = (got.flatten() - pairwise).abs().max().item()
    print(f"\nadists forward_group {shape} [{prec}] vs the pairwise module: max |dD| = {d:.2e}")
    assert d <= NAMED_TOL
    assert torch.equal(got, again)  # no atomics on any sum


@pytest.mark.parametrize("prec,h,w", [("f32", 33, 47), ("f32s", 144, 128)])
def test_identity_duplicates_and_permutations(prec, h, w, models, dev):
    """Render 0 is the reference itself, renders 2 and 3 are one frame; then the same group with its renders permuted."""
    ref, ren = (t.to(dev) for t in _group(2, 3, h, w))
    ren = torch.stack([ref, ren[:, 0], ren[:, 1], ren[:, 1], ren[:, 2]], dim=1).contiguous()  # (2, 5, 3, h, w)
    m = models[prec]
    perm = [3, 0, 4, 2, 1]
    with torch.no_grad():
        got = m.forward_group(ref, ren)
        same = m(ref, ref.clone(), as_loss=False)
        permuted = m.forward_group(ref, ren[:, perm].contiguous())
    assert (got[:, 0] - same).abs().max().item() <= NAMED_TOL
    assert torch.equal(got[:, 2], got[:, 3])
    assert torch.equal(permuted, got[:, perm])
    assert (got[:, 1:] > got[:, :1]).all()  # every distorted render lies farther from the reference than the reference


@pytest.mark.parametrize("prec,shape", [("f32", (2, 3, 33, 47)), ("f32s", (2, 2, 144, 128))], ids=str)
def test_score_group_gives_both_metrics_from_one_pyramid(prec, shape, models, dists_models, dev):
    from nerf_qa_amd import ops, pair
    from oracle import dists_oracle
    R, K, h, w = shape
    ref, ren = (t.to(dev) for t in _group(*shape))
    am, dm = models[prec], dists_models[prec]
    x, y = ref.repeat_interleave(K, 0), ren.flatten(0, 1)
    with torch.no_grad():
        ds, ad = pair.score_group(dm, am, ref, ren)
        assert ds.shape == ad.shape == (R, K) and ds.dtype == ad.dtype == torch.float32
        assert torch.equal(ad, am.forward_group(ref, ren))
        packed = am._packed_weights(dev, prec)
        dg, g1, g2 = ops.adists_forward_group(ref, ren, packed, prec, with_dists=True)
        assert torch.equal(dg, ops.adists_forward_group(ref, ren, packed, prec))  # the similarities change nothing
        _, p1, p2 = ops.adists_dists_forward(x, y, packed, prec)
        # float64 similarities of the module's own taps
        fr = [f.double().repeat_interleave(K, 0) for f in am.forward_once(ref)]
        fy = [f.double() for f in am.forward_once(y)]
        w1, w2 = dists_oracle.dists_stats(fr, fy)
        want = dm.forward_group(ref, ren)
    eg = max((g1.double() - w1).abs().max().item(), (g2.double() - w2).abs().max().item())
    ep = max((p1.double() - w1).abs().max().item(), (p2.double() - w2).abs().max().item())
    dsc = (ds - want).abs().max().item()
    print(f"\nscore_group {shape} [{prec}] S vs float64 S of its taps: group {eg:.2e} pairwise {ep:.2e}; "
          f"|dscore vs DISTS.forward_group| = {dsc:.2e}")
    assert eg <= max(2 * ep, FLOOR)
    assert dsc <= NAMED_TOL


def test_surface(models, dev):
    m = models["f32"]
    ref, ren = (t.to(dev) for t in _group(2, 3, 33, 47))
    with torch.no_grad():
        s = m.forward_group(ref, ren)
        loss = m.forward_group(ref, ren, as_loss=True)
        one = m.forward_group(ref[:1], ren[:1, :1])
        fwd = m(ref[:1], ren[:1, 0], as_loss=False)
        t = m.forward_group(ref, ren.transpose(0, 1).contiguous().transpose(0, 1))  # a non-contiguous view
    assert s.shape == (2, 3) and s.dtype == torch.float32
    assert loss.dim() == 0 and abs(loss.item() - (1 - (1 - s).mean().item())) <= 1e-6
    assert one.shape == (1, 1) and abs(one.item() - fwd.item()) <= NAMED_TOL
    assert torch.equal(t, s)
    for a, b in ((ref, ren[:1]), (ref, ren[..., :40]), (ref, ren[:, 0]), (ref[0], ren)):
        with pytest.raises(ValueError):
            m.forward_group(a, b)
    with pytest.raises(ValueError, match="forward"):
        m.forward_group(ref.clone().requires_grad_(True), ren)
    with pytest.raises(ValueError, match="forward"):
        m.forward_group(ref, ren.clone().requires_grad_(True))


def test_score_videos_equals_k_score_video_calls(dev):
    from nerf_qa_amd import video
    from nerf_qa_amd.ADISTS import ADISTS
    from nerf_qa_amd.DISTS_pytorch import DISTS
    N, K, H, W = 5, 2, 64, 96
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        dm, am = DISTS().to(dev).eval(), ADISTS().to(dev).eval()  # (auto: frames this small run in f32s / f32)
    ref, ren = (t.to(dev) for t in _group(N, K, H, W))
    rens = ren.transpose(0, 1).contiguous()  # (K, N, 3, H, W)
    today = video.score_videos(ref, rens, dm, batch_size=2, return_frame_scores=True)
    assert [list(d) for d in today] == [["DISTS", "DISTS_std", "DISTS_min", "DISTS_max", "frame_count", "frame_bias_dists",
                                         "_frame_scores"]] * K and list(today[0]["_frame_scores"]) == ["DISTS"]
    for shared in (False, True):
        cols = video.score_videos(ref, rens, dm, batch_size=2, return_frame_scores=True, adists_model=am,
                                  shared_pyramid=shared)
        assert len(cols) == K
        for k in range(K):
            one = video.score_video(ref, rens[k], dm, am, batch_size=2, return_frame_scores=True, shared_pyramid=shared)
            assert list(cols[k]) == list(one) and cols[k]["frame_count"] == one["frame_count"] == 3
            assert list(cols[k]["_frame_scores"]) == list(one["_frame_scores"]) == ["A-DISTS", "DISTS"]
            for name in ("A-DISTS", "DISTS"):
                a, b = cols[k]["_frame_scores"][name], one["_frame_scores"][name]
                assert a.shape == b.shape == (N,) and a.dtype == b.dtype == np.float32
                err = np.abs(a - b).max()
                print(f"\nscore_videos shared={shared} column {k} {name}: |d frame scores| = {err:.2e}")
                assert err <= NAMED_TOL
                for key in (name, name + "_std", name + "_min", name + "_max"):
                    assert type(cols[k][key]) is type(one[key]) and abs(float(cols[k][key]) - float(one[key])) <= NAMED_TOL
            if not shared:  # the DISTS half is the DISTS-only call's, bit for bit
                assert np.array_equal(cols[k]["_frame_scores"]["DISTS"], today[k]["_frame_scores"]["DISTS"])
