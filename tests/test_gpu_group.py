"""DISTS of K renders against one reference from ONE shared pyramid per group (nqa_dists_forward_group through
DISTS.forward_group and video.score_videos) on the GPU.

Bounds: pair by pair against the CPU oracle -- scores within the project's SCORE_TOL in every mode tried, and in "f32" /
"f32s" the similarities within S_TOL and the scores within 5e-6 (the named-mode bound of test_gpu_fullsize_golden.py).
Against the pairwise module of the same named precision the group path is the same arithmetic on another split of the
sums: both are measured against float64 similarities computed from the module's own taps (forward_once), and the group
path gets twice the pairwise path's distance, floored at 2^-22.
"""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SCORE_TOL = 1e-4      # the project's bar (tests/test_gpu_dists.py SCORE_TOL)
S_TOL = 5e-4          # tests/test_gpu_dists.py::test_dists_vs_golden, max |S - golden S| for "f32" and "f32s"
NAMED_TOL = 5e-6      # tests/test_gpu_fullsize_golden.py: explicitly named "f32s" / "f32" scores
FLOOR = 2.0 ** -22
SHAPES = [(1, 1, 17, 23), (2, 3, 33, 47), (3, 2, 64, 96), (1, 5, 130, 95)]
PRECS = ("f32", "f32s", "f16", "f32m")
_ids = lambda s: "R%dK%d_%dx%d" % s


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def models(dev):
    from nerf_qa_amd.DISTS_pytorch import DISTS
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return {p: DISTS(precision=p).to(dev).eval() for p in PRECS}


def _group(R, K, h, w):
    """ref (R,3,h,w) and renders (R,K,3,h,w): noise, blur and one synth.NERF_KINDS kind in every group (K = 1: noise; K = 2:
    blur and a NeRF-like frame)."""
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


def _oracle(shape, oracle_convs, alpha_beta):
    """(ref, renders, S1, S2, score) of the CPU oracle, pair by pair; computed once per shape."""
    if shape not in _ORACLE:
        from oracle import dists_oracle
        R, K, h, w = shape
        ref, ren = _group(*shape)
        with torch.no_grad():
            f0 = [f.repeat_interleave(K, 0) for f in dists_oracle.vgg_pyramid(ref, oracle_convs)]
            f1 = dists_oracle.vgg_pyramid(ren.flatten(0, 1), oracle_convs)
            s1, s2 = dists_oracle.dists_stats(f0, f1)
            score = dists_oracle.dists_score(s1, s2, *alpha_beta)
        _ORACLE[shape] = (ref, ren, s1, s2, score.view(R, K))
    return _ORACLE[shape]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_forward_group_against_the_cpu_oracle(shape, prec, models, oracle_convs, alpha_beta, dev):
    R, K, h, w = shape
    ref, ren, w1, w2, want = _oracle(shape, oracle_convs, alpha_beta)
    m = models[prec]
    with torch.no_grad():
        got = m.forward_group(ref.to(dev), ren.to(dev))
        s1, s2 = m._group_similarities(ref.to(dev), ren.to(dev))
    assert got.shape == (R, K) and got.dtype == torch.float32 and s1.shape == s2.shape == (R * K, 1475)
    d = (got.cpu() - want).abs().max().item()
    e1, e2 = (s1.cpu() - w1).abs().max().item(), (s2.cpu() - w2).abs().max().item()
    print(f"\nforward_group {shape} [{prec}] vs oracle: |dscore|={d:.2e} |dS1|={e1:.2e} |dS2|={e2:.2e}")
    assert d <= SCORE_TOL
    if prec in ("f32", "f32s"):
        assert e1 <= S_TOL and e2 <= S_TOL
        assert d <= NAMED_TOL


@pytest.mark.parametrize("prec", ("f32", "f32s"))
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_forward_group_agrees_with_the_pairwise_module(shape, prec, models, dev):
    from oracle import dists_oracle
    R, K, h, w = shape
    ref, ren = (t.to(dev) for t in _group(*shape))
    m = models[prec]
    x, y = ref.repeat_interleave(K, 0), ren.flatten(0, 1)
    with torch.no_grad():
        g1, g2 = m._group_similarities(ref, ren)
        p1, p2 = m._similarities(x, y)
        gs, ps = m.forward_group(ref, ren), m(x, y)
        # float64 similarities of the module's own taps
        fr = [f.double().repeat_interleave(K, 0) for f in m.forward_once(ref)]
        fy = [f.double() for f in m.forward_once(y)]
        w1, w2 = dists_oracle.dists_stats(fr, fy)
    dg = max((g1.double() - w1).abs().max().item(), (g2.double() - w2).abs().max().item())
    dp = max((p1.double() - w1).abs().max().item(), (p2.double() - w2).abs().max().item())
    ds = (gs.flatten() - ps).abs().max().item()
    print(f"\nforward_group {shape} [{prec}] vs float64 S of its taps: group {dg:.2e} pairwise {dp:.2e}; |dscore group - pairwise|={ds:.2e}")
    assert dg <= max(2 * dp, FLOOR)
    assert ds <= NAMED_TOL


def test_batch_average_and_k1(models, dev):
    m = models["f32s"]
    ref, ren = (t.to(dev) for t in _group(2, 3, 33, 47))
    with torch.no_grad():
        s = m.forward_group(ref, ren)
        avg = m.forward_group(ref, ren, batch_average=True)
        one = m.forward_group(ref[:1], ren[:1, :1])
        again = m.forward_group(ref, ren)
    assert avg.dim() == 0 and abs(avg.item() - s.mean().item()) <= 1e-7
    assert one.shape == (1, 1) and abs(one.item() - s[0, 0].item()) <= NAMED_TOL
    assert torch.equal(again, s)
    # the renders may arrive as a non-contiguous view
    with torch.no_grad():
        t = m.forward_group(ref, ren.transpose(0, 1).contiguous().transpose(0, 1))
    assert torch.equal(t, s)


def test_alpha_gradient(models, dev):
    """alpha / beta receive gradients through forward_group as through forward (run_nerf_qa.py:433-461)."""
    m = models["f32s"]
    ref, ren = (t.to(dev) for t in _group(2, 3, 33, 47))
    m.zero_grad()
    score = m.forward_group(ref, ren)
    assert score.requires_grad and score.shape == (2, 3)
    score.sum().backward()
    assert m.alpha.grad is not None and m.beta.grad is not None
    with torch.no_grad():
        fused = m.forward_group(ref, ren)
        s1, s2 = m._group_similarities(ref, ren)
    assert (fused - score.detach()).abs().max().item() < 2e-6
    a, b_ = m.alpha.detach().view(-1).double(), m.beta.detach().view(-1).double()
    w = a.sum() + b_.sum()
    for j in (1, 10, 700):
        d = (-(s1[:, j].double()) / w + ((a * s1.double()).sum(1) + (b_ * s2.double()).sum(1)) / w ** 2).sum()
        assert abs(m.alpha.grad.view(-1)[j].item() - d.item()) < 1e-4 * max(1.0, abs(d.item()))
    m.zero_grad()


def test_flat_reference_is_rescored_under_auto(models, dev):
    """`auto` on a fast rung: a pair whose reference OR render is nearly flat carries the pairwise f32s result, the other
    pairs the fast rung's.  (The rung is pinned the way sharding.agree_precision pins it, so nothing is calibrated.)"""
    from nerf_qa_amd.DISTS_pytorch import DISTS
    from nerf_qa_amd.DISTS_pytorch import DISTS_pt as dp
    H, W, R, K = 128, 160, 2, 3
    ref, ren = (t.to(dev) for t in _group(R, K, H, W))
    low = torch.nn.functional.interpolate(torch.rand(1, 3, 8, 10, generator=torch.Generator().manual_seed(3)), size=(H, W),
                                          mode="bilinear").to(dev)
    ref[1] = 0.4 + 0.02 * (low[0] - 0.5)   # a nearly flat reference: its whole group is flagged
    ren[0, 2] = 0.6 + 0.01 * (low[0] - 0.5)  # a nearly flat render: that pair alone
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        auto = DISTS().to(dev).eval()
    auto._agreed[max(dp.size_class(H, W), 0)] = (auto._weights_key(dev), "f16")
    assert auto.precision_for(H, W, dev) == "f16" and dp.AUTO_FLAT_VAR == 2e-3
    flagged = torch.tensor([[False, False, True], [True, True, True]], device=dev)
    with torch.no_grad():
        got = auto.forward_group(ref, ren)
        fast = models["f16"].forward_group(ref, ren)
        idx = flagged.flatten().nonzero().flatten()
        exact = models["f32s"](ref.repeat_interleave(K, 0)[idx], ren.flatten(0, 1)[idx])
    assert torch.equal(got[~flagged], fast[~flagged])
    assert torch.equal(got[flagged], exact)
    assert not torch.equal(fast[flagged], exact)


def test_score_videos_equals_k_score_video_calls(dev):
    from nerf_qa_amd import video
    from nerf_qa_amd.DISTS_pytorch import DISTS
    N, K, H, W = 5, 3, 64, 96
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = DISTS().to(dev).eval()  # (auto: frames this small always run in f32s)
    ref, ren = (t.to(dev) for t in _group(N, K, H, W))
    rens = ren.transpose(0, 1).contiguous()  # (K, N, 3, H, W)
    cols = video.score_videos(ref, rens, m, batch_size=2, return_frame_scores=True)
    listed = video.score_videos(ref, [rens[k] for k in range(K)], m, batch_size=2, return_frame_scores=True)
    assert len(cols) == K == len(listed)
    for k in range(K):
        one = video.score_video(ref, rens[k], m, batch_size=2, return_frame_scores=True)
        assert list(cols[k]) == list(one) and cols[k]["frame_count"] == one["frame_count"] == 3
        a, b = cols[k]["_frame_scores"]["DISTS"], one["_frame_scores"]["DISTS"]
        assert a.shape == b.shape == (N,) and a.dtype == b.dtype == np.float32
        err = np.abs(a - b).max()
        print(f"\nscore_videos column {k}: |d frame scores|={err:.2e}")
        assert err <= SCORE_TOL
        for key in ("DISTS", "DISTS_std", "DISTS_min", "DISTS_max"):
            assert type(cols[k][key]) is type(one[key]) and abs(float(cols[k][key]) - float(one[key])) <= SCORE_TOL
        assert np.array_equal(listed[k]["_frame_scores"]["DISTS"], a)
