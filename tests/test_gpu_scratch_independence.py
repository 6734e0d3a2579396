"""Every entry point's results must not depend on what its scratch held when the call started.

The kernels are each held to exact or float64 references on their own; the memory they pass to one another is not.  A
workspace is carved into activation buffers, statistics partials, seam planes, coefficient records, window moments and
exponent partials, outputs and stage-level scratch come from torch.empty, and ops.Workspace hands the second call of a
module the first call's bytes back -- so a partial slot, seam row or coefficient record that is read but not written
reads the right number from one call earlier, and every "bit-repeatable" test passes.

Here every case runs three times (tests/poison.py): with every workspace buffer and every torch.empty CUDA tensor
filled with 0x00 first, then with 0xFF (NaN in half, bfloat16, float, double and split16 records, 255 in uint8, -1 in
int32), then unpoisoned.  Asserted per case:

  * every returned tensor is bit-equal across the three runs (compared as byte views);
  * no returned value is NaN (the shapes are ones where the reference is finite: no 1x1 or 21x21 A-DISTS);
  * the helper's counters show that a poisoned workspace was asked (where the entry point has one) and at least one
    torch.empty tensor was filled: a refactor that allocates past the hooks fails instead of passing unpoisoned.  The
    counters are printed per case (run with -s);
  * the module-level forwards also compare their 0xFF run with the CPU oracle at the existing bar of that path: DISTS
    at test_gpu_fuzz.py::test_random_shape's per-mode bars ("f32": test_gpu_dists.py's SCORE_TOL), A-DISTS f32s at the
    same test's 2e-5.

What a 0xFF fill cannot do here: no workspace region holds an integer that a kernel uses as an index, a count or a
loop bound before a kernel of the same call has written it ("Workspace regions"): the resize pass' bounds
are written by its coefficient kernel, the chain's accumulators by chain_init_kernel, the exponents by
exponent_finish_kernel for every image.  The 0x00 run of a case comes before its 0xFF run.

Graph capture is out of scope: a fill inside a capture would become part of the graph.
"""
import sys

import numpy as np
import pytest
import torch

import poison

pytestmark = pytest.mark.gpu

SPEC = "synth:1234"
# tests/test_gpu_fuzz.py::test_random_shape (small odd frames, every mode); "f32": tests/test_gpu_dists.py SCORE_TOL
DISTS_BAR = {"f32s": 1e-5, "f32m2": 1e-4, "f32m": 1e-4, "f16w": 1e-4, "f16": 1e-4, "bf16": 1e-3, "f32": 1e-4}
ADISTS_BAR = 2e-5  # tests/test_gpu_fuzz.py::test_random_shape, "a32s"
DISTS_MODES = ("f16", "f16w", "f32m", "f32m2", "f32s", "f32", "bf16")
CHNS = (3, 64, 128, 256, 512, 512)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def blobs(np_convs, dev):
    from nerf_qa_amd import ops
    cache = {}

    def get(prec):
        if prec not in cache:
            cache[prec] = ops.pack_vgg_weights(np_convs, prec).to(dev)
        return cache[prec]
    return get


@pytest.fixture(scope="module")
def dists(dev):
    from nerf_qa_amd.DISTS_pytorch import DISTS
    return DISTS(vgg16_path=SPEC, precision="f32s").to(dev).eval()


@pytest.fixture(scope="module")
def adists(dev):
    from nerf_qa_amd.ADISTS import ADISTS
    return ADISTS(vgg16_path=SPEC, precision="f32s", loss_head="auto").to(dev).eval()


_FRAMES, _ORACLE = {}, {}


def _frames(b, h, w):
    """(x, y) CPU float32 (b,3,h,w): synthetic pairs, one seed per pair, the distortion kinds cycling."""
    from nerf_qa_amd import synth
    key = (b, h, w)
    if key not in _FRAMES:
        xn, yn = synth.frame_batch([300 + 17 * h + w + i for i in range(b)], h, w)
        _FRAMES[key] = (torch.from_numpy(xn), torch.from_numpy(yn))
    return _FRAMES[key]


def _oracle(kind, b, h, w, convs, model=None):
    """The CPU oracle's scores of _frames(b, h, w), computed once per shape and shared."""
    from oracle import adists_oracle, dists_oracle
    key = (kind, b, h, w)
    if key not in _ORACLE:
        x, y = _frames(b, h, w)
        if kind == "dists":
            _ORACLE[key] = dists_oracle.dists(x, y, convs, model.alpha.detach().cpu(), model.beta.detach().cpu())
        else:
            _ORACLE[key] = adists_oracle.adists(x, y, convs)
    return _ORACLE[key]


def _relu_maps(shape, seed, dtype=torch.float32):
    """Non-negative maps with zeros, like taps behind a ReLU (CPU)."""
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g).sub_(0.3).clamp_(min=0).to(dtype)


# ---- the three runs ---------------------------------------------------------------------------------------------------
def _flat(out):
    if out is None:
        return []
    if torch.is_tensor(out):
        return [out]
    return [t for o in out for t in _flat(o)]


def _bytes(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def _ws(p):
    """The ws= argument of a run: a poisoned workspace of the run's byte, or None (the entry point's own) unpoisoned."""
    return None if p is None else p.workspace()


def three_runs(name, call, monkeypatch, modules=(), need_ws=True, need_empty=True):
    """call(p) under fill 0x00, under fill 0xFF (p: the poison.Poison of the run) and unpoisoned (p None), in that order;
    returns {0x00 | 0xFF | None: [returned tensors]} after the assertions of the module docstring."""
    runs = {}
    for byte in poison.FILLS:
        with poison.poisoned(byte, *modules, monkeypatch=monkeypatch) as p:
            out = call(p)
            torch.cuda.synchronize()
        print(f"  {name}: {p.report()}")
        p.require(workspace=need_ws, empty=need_empty)
        runs[byte] = [t.detach() for t in _flat(out)]
    assert torch.empty.__name__ == "empty" and not hasattr(torch.empty, "__wrapped__")
    out = call(None)
    torch.cuda.synchronize()
    runs[None] = [t.detach() for t in _flat(out)]
    same_results(name, runs)
    return runs


def same_results(name, runs, ref_key=None):
    ref = runs[ref_key]
    assert ref, f"{name}: the case returned nothing to compare"
    for key, got in runs.items():
        assert len(got) == len(ref), (name, key)
        for i, (a, b) in enumerate(zip(got, ref)):
            assert a.shape == b.shape and a.dtype == b.dtype, (name, key, i, a.shape, b.shape, a.dtype, b.dtype)
            if a.is_floating_point():
                nans = int(torch.isnan(a).sum())
                assert nans == 0, f"{name}: output {i} {tuple(a.shape)} holds {nans} NaN under {_label(key)}"
            if key == ref_key:
                continue
            if not torch.equal(_bytes(a), _bytes(b)):
                diff = int((a != b).sum())
                far = float((a.double() - b.double()).abs().max()) if a.numel() else 0.0
                raise AssertionError(f"{name}: output {i} {tuple(a.shape)} {a.dtype} under {_label(key)} differs from "
                                     f"{_label(ref_key)} in {diff} of {a.numel()} elements (max |d| {far:.3e})")


def _label(key):
    return "the unpoisoned run" if key is None else (f"fill 0x{key:02X}" if isinstance(key, int) else str(key))


# ---- 1. the DISTS pyramid: ops.dists_forward, ops.vgg_pyramid, module DISTS -----------------------------------------
# 37x70: fused stage 1 and fused conv2_2, ragged both ways; 36x64: their full-tile instances; 7x9: W < 16, nothing
# fused and only 16-wide tiles
DISTS_SHAPES = [(37, 70), (36, 64), (7, 9)]


@pytest.mark.parametrize("h,w", DISTS_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("prec", DISTS_MODES)
def test_dists_pyramid_entries(prec, h, w, blobs, dists, oracle_convs, dev, monkeypatch):
    from nerf_qa_amd import ops
    packed = blobs(prec)
    monkeypatch.setattr(dists, "precision", prec)
    print()
    for b in (2, 3):
        xc, yc = _frames(b, h, w)
        x, y = xc.to(dev), yc.to(dev)
        tag = f"{prec} {h}x{w} B={b}"
        if prec in ("f16", "f16w") and w >= 16:  # (the shape list's promise: stage 1 fused in f16, conv2_2 in both)
            assert 2 in ops.dists_fused_taps(b, h, w, prec) and (prec != "f16" or 1 in ops.dists_fused_taps(b, h, w, prec))
        if w < 16:
            assert ops.dists_fused_taps(b, h, w, prec) == ()
        three_runs(f"dists_forward {tag}", lambda p: ops.dists_forward(x, y, packed, prec, _ws(p)), monkeypatch)
        three_runs(f"vgg_pyramid {tag}", lambda p: ops.vgg_pyramid(x, packed, prec, _ws(p)), monkeypatch)

        def module(p):
            with torch.no_grad():
                return dists(x, y)
        runs = three_runs(f"DISTS module {tag}", module, monkeypatch, modules=(dists,))
        ref = _oracle("dists", b, h, w, oracle_convs, dists)
        err = (runs[0xFF][0].cpu() - ref).abs().max().item()
        print(f"  DISTS module {tag}: |score - oracle| under fill 0xFF = {err:.2e} (bar {DISTS_BAR[prec]:.0e})")
        assert err <= DISTS_BAR[prec], (tag, err)


def test_dists_forward_unfused_taps_in_the_same_layout(blobs, dev, monkeypatch):
    """set_conv_variant(DEFAULT + 64): tap 2 through the unfused conv + pool_stats, inside a workspace that is sized
    for the fused and the unfused form alike."""
    from nerf_qa_amd import ops
    xc, yc = _frames(2, 37, 70)
    x, y = xc.to(dev), yc.to(dev)
    print()
    for prec in ("f16", "f16w"):
        fused = ops.dists_forward(x, y, blobs(prec), prec)
        ops.set_conv_variant(ops.DEFAULT_CONV_VARIANT + 64)
        try:
            assert 2 not in ops.dists_fused_taps(2, 37, 70, prec)
            runs = three_runs(f"dists_forward {prec} 37x70 variant+64",
                              lambda p: ops.dists_forward(x, y, blobs(prec), prec, _ws(p)), monkeypatch)
        finally:
            ops.set_conv_variant(ops.DEFAULT_CONV_VARIANT)
        # (taps 0 and 1 do not know about the switch: test_gpu_conv_pool.py::test_dists_forward_fused_tap_equals_unfused)
        assert torch.equal(runs[None][0][:, :67], fused[0][:, :67])


# ---- 2. A-DISTS: ops.adists_forward, ops.adists_dists_forward, module ADISTS on two streams ----------------------
# 44x52: stages 0 to 2 windowed (44x52, 44x52, 22x26), the deeper ones global; 20x50: all global
ADISTS_SHAPES = [(44, 52), (20, 50)]


@pytest.mark.parametrize("h,w", ADISTS_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("prec", ["f32s", "f16"])
def test_adists_entries(prec, h, w, blobs, dev, monkeypatch):
    from nerf_qa_amd import ops
    assert ops.adists_chain_dims(h, w)[1] == (3 if h == 44 else 0)
    xc, yc = _frames(2, h, w)
    x, y = xc.to(dev), yc.to(dev)
    packed, tag = blobs(prec), f"{prec} {h}x{w} B=2"
    print()
    plain = three_runs(f"adists_forward {tag}", lambda p: ops.adists_forward(x, y, packed, prec, _ws(p)), monkeypatch)
    maps = three_runs(f"adists_forward with_map {tag}",
                      lambda p: ops.adists_forward(x, y, packed, prec, _ws(p), with_map=True), monkeypatch)
    both = three_runs(f"adists_dists_forward {tag}", lambda p: ops.adists_dists_forward(x, y, packed, prec, _ws(p)),
                      monkeypatch)
    bothm = three_runs(f"adists_dists_forward with_map {tag}",
                       lambda p: ops.adists_dists_forward(x, y, packed, prec, _ws(p), with_map=True), monkeypatch)
    # (asking for the map or for S1 / S2 changes nothing of D: the entry points' own contract)
    assert all(torch.equal(r[0xFF][0], plain[0xFF][0]) for r in (maps, both, bothm))
    assert torch.equal(bothm[0xFF][3], maps[0xFF][1])


def test_adists_module_two_stream_halves(adists, oracle_convs, dev, monkeypatch):
    """ADISTS._batched's two half-batches on two HIP streams, forced at a small shape by lowering the module's pixel
    threshold (tests/test_gpu_adists.py reaches it with five 520x600 frames): a buffer per side stream, each filled on
    its own stream."""
    from nerf_qa_amd.ADISTS import ADISTS
    A = sys.modules[ADISTS.__module__]
    monkeypatch.setattr(A, "TWO_STREAM_MIN_PIXELS", 0)
    monkeypatch.delenv("NQA_ADISTS_STREAMS", raising=False)
    b, h, w = 5, 44, 52
    assert b >= A.TWO_STREAM_MIN_PAIRS
    xc, yc = _frames(b, h, w)
    x, y = xc.to(dev), yc.to(dev)

    def module(p):
        with torch.no_grad():
            out = adists(x, y, as_loss=False)
        assert len(adists._ws.bufs) == 2  # one scratch buffer per side stream
        return out
    print()
    runs = three_runs(f"ADISTS module f32s {h}x{w} B={b}, two streams", module, monkeypatch, modules=(adists,))
    ref = _oracle("adists", b, h, w, oracle_convs)
    err = (runs[0xFF][0].cpu() - ref).abs().max().item()
    print(f"  ADISTS module two streams: |score - oracle| under fill 0xFF = {err:.2e} (bar {ADISTS_BAR:.0e})")
    assert err <= ADISTS_BAR, err
    monkeypatch.setenv("NQA_ADISTS_STREAMS", "1")
    with torch.no_grad():
        one = adists(x, y, as_loss=False)
    assert (one - runs[None][0]).abs().max().item() <= 3e-7  # (test_adists_two_stream_halves_equal_one_call's bound)


# ---- 3. one reference against K renders -----------------------------------------------------------------------------
GROUP_SHAPES = [(37, 70), (44, 52)]
R, K = 2, 3


def _group_frames(h, w, dev):
    xc, yc = _frames(R * K, h, w)
    ref = xc[::K].contiguous()
    renders = yc.reshape(R, K, 3, h, w).clone()
    renders[:, 0] = 0.5 * (ref + renders[:, 0])  # (so that a group's renders belong to its reference)
    return ref.to(dev), renders.contiguous().to(dev)


@pytest.mark.parametrize("h,w", GROUP_SHAPES, ids=lambda v: str(v))
def test_group_entries(h, w, blobs, dev, monkeypatch):
    from nerf_qa_amd import ops
    ref, renders = _group_frames(h, w, dev)
    print()
    for prec in ("f16", "f32s"):
        three_runs(f"dists_forward_group {prec} {h}x{w} R={R} K={K}",
                   lambda p: ops.dists_forward_group(ref, renders, blobs(prec), prec, _ws(p)), monkeypatch)
    for prec in ("f32s", "f16"):
        d = three_runs(f"adists_forward_group {prec} {h}x{w}",
                       lambda p: ops.adists_forward_group(ref, renders, blobs(prec), prec, _ws(p)), monkeypatch)
        ds = three_runs(f"adists_forward_group with_dists {prec} {h}x{w}",
                        lambda p: ops.adists_forward_group(ref, renders, blobs(prec), prec, _ws(p), with_dists=True),
                        monkeypatch)
        assert torch.equal(d[0xFF][0], ds[0xFF][0])
    # one map's group statistics on their own (scratch from torch.empty: there is no ops.Workspace to ask)
    n, hw = R + R * K, h * w
    for c in (64, 512):
        planes = _relu_maps((n, c, hw), 7 * c + h).to(dev)
        three_runs(f"dists_group_stats planar C={c} HW={hw}",
                   lambda p: ops.dists_group_stats(planes, R, K, "f32", nchw=True), monkeypatch, need_ws=False)
        for prec, dt in (("f32", torch.float32), ("f16", torch.float16)):
            feat = _relu_maps((n, hw, c), 11 * c + h, dt).to(dev)
            three_runs(f"dists_group_stats NHWC {prec} C={c} HW={hw}",
                       lambda p: ops.dists_group_stats(feat, R, K, prec), monkeypatch, need_ws=False)


# ---- 4. the staged A-DISTS entries at the 44x52 pyramid ---------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32s", "f16"])
def test_staged_adists_entries(prec, blobs, dev, monkeypatch):
    from nerf_qa_amd import ops
    h, w = 44, 52
    b = R * K
    ref, renders = _group_frames(h, w, dev)
    x, y = ref.repeat_interleave(K, 0).contiguous(), renders.flatten(0, 1).contiguous()
    storage = prec
    taps = ops.vgg_pyramid(torch.cat([x, y]), blobs(prec), prec)
    print()
    front = three_runs(f"adists_front {prec} {h}x{w} B={b}", lambda p: ops.adists_front(x, y, taps, storage, _ws(p)),
                       monkeypatch)
    q, wgt = front[None]
    gamma, tw, sw, ggam, off = [], [], [], [], 0
    for k, c in enumerate(CHNS):
        fx, fy = (x, y) if k == 0 else (taps[k - 1][:b].contiguous(), taps[k - 1][b:].contiguous())
        qk, wk = q[:, :, off:off + c].contiguous(), wgt[:, off:off + c].contiguous()
        st = three_runs(f"adists_window_stage {prec} stage {k} {tuple(fx.shape[1:])}",
                        lambda p: ops.adists_window_stage(fx, fy, qk, wk, storage), monkeypatch, need_ws=False)
        fxr, wkr = fx[::K].contiguous(), wk[::K].contiguous()
        sg = three_runs(f"adists_window_stage_group {prec} stage {k}",
                        lambda p: ops.adists_window_stage_group(fxr, fy, qk, wkr, storage), monkeypatch, need_ws=False)
        # (the group form is the pairwise one bit for bit: tests/test_gpu_adists_group_stage.py)
        assert torch.equal(sg[0xFF][1], st[0xFF][1]) and torch.equal(sg[0xFF][0], st[0xFF][0][::K])
        gamma.append(st[None][0]), tw.append(st[None][1]), sw.append(st[None][2]), ggam.append(sg[None][0])
        off += c
    for with_map in (True, False):
        three_runs(f"adists_chain {prec} with_map={with_map}",
                   lambda p: ops.adists_chain(gamma, tw, sw, h, w, with_map, _ws(p)), monkeypatch)
    three_runs(f"adists_chain_group {prec}", lambda p: ops.adists_chain_group(ggam, tw, sw, h, w, _ws(p)), monkeypatch)


# ---- 5. one stage of the A-DISTS head's backward --------------------------------------------------------------------
# windowed on the scalar path; windowed on the 16-byte path with two blocks of the dot product (65 * 64 > 4096); global
TS_SHAPES = [(1, 64, 22, 37), (1, 64, 65, 64), (2, 512, 13, 17)]


@pytest.mark.parametrize("b,c,h,w", TS_SHAPES, ids=lambda v: str(v))
def test_adists_ts_backward(b, c, h, w, dev, monkeypatch):
    from nerf_qa_amd import ops
    X, Y = _relu_maps((b, c, h, w), 1000 + c + h), _relu_maps((b, c, h, w), 2000 + c + h)
    Y[:, 1] = 0  # a dead channel of y: F.normalize's clamp
    xd, yd = X.double().flatten(2), Y.double().flatten(2)
    mx, my = xd.mean(2), yd.mean(2)
    q = torch.stack([1 / xd.norm(dim=2).clamp_min(1e-12), 1 / yd.norm(dim=2).clamp_min(1e-12), xd.sum(2), mx, my,
                     (xd * xd).mean(2) - mx * mx, (yd * yd).mean(2) - my * my, (xd * yd).mean(2) - mx * my]).float()
    g = torch.Generator().manual_seed(c + w)
    windowed = h >= 21 and w >= 21
    ps = torch.rand((b, h - 20, w - 20) if windowed else (b, 1, 1), generator=g)
    wgt = (torch.rand((b, c), generator=g) + 0.5) / 1475
    u = torch.full((b,), -1.0 / b)
    args = [t.contiguous().to(dev) for t in (X, Y, q, wgt, ps, u)]
    print()
    planar = three_runs(f"adists_ts_backward planar {b}x{c}x{h}x{w}",
                        lambda p: ops.adists_ts_backward(*args, mask=True, ws=_ws(p)), monkeypatch)
    nhwc = three_runs(f"adists_ts_backward NHWC {b}x{c}x{h}x{w}",
                      lambda p: ops.adists_ts_backward(*args, mask=True, nhwc=True, ws=_ws(p)), monkeypatch)
    assert torch.equal(nhwc[0xFF][0].permute(0, 3, 1, 2), planar[0xFF][0])
    assert planar[0xFF][0].abs().max().item() > 0 and (planar[0xFF][0][:, 1] == 0).all()


# ---- 6. statistics and their gradients --------------------------------------------------------------------------------
# six planar maps of one call (forward_from_feats takes any sizes): C = 64 and 512 over 33 * 47 pixels and over one pixel,
# and the image's three channels
NCHW_MAPS = [(64, 33, 47), (512, 33, 47), (64, 1, 1), (512, 1, 1), (3, 33, 47), (128, 5, 6)]


def test_nchw_statistics_and_backward(dev, monkeypatch):
    """forward_from_feats' kernels: the sums kept as scratch, then the coefficient records and the gradients."""
    from nerf_qa_amd import ops
    b = 2
    f0 = [_relu_maps((b, c, h, w), 50 + k).to(dev) for k, (c, h, w) in enumerate(NCHW_MAPS)]
    f1 = [_relu_maps((b, c, h, w), 80 + k).to(dev) for k, (c, h, w) in enumerate(NCHW_MAPS)]
    g = torch.Generator().manual_seed(7)
    g1, g2 = (torch.randn(b, sum(c for c, _, _ in NCHW_MAPS), generator=g).to(dev) for _ in range(2))

    def call(p):
        s1, s2, scratch = ops.dists_stats_nchw(f0, f1, keep_scratch=True)
        gx, gy = ops.dists_stats_nchw_backward(f0, f1, scratch, g1, g2, [True] * 6, [True, True, False, True, True, False])
        return s1, s2, gx, gy
    print()
    runs = three_runs("dists_stats_nchw + backward, C = 64 / 512 over 33x47 and 1x1", call, monkeypatch, need_ws=False)
    assert len(runs[0xFF]) == 2 + 6 + 4


@pytest.mark.parametrize("h,w", [(1, 1), (33, 47)], ids=lambda v: str(v))
@pytest.mark.parametrize("c", [64, 512])
def test_nhwc_statistics_and_their_gradients(c, h, w, dev, monkeypatch):
    """33 * 47 pixels are 13 blocks per pair of the sums kernel at C = 64 and 97 at C = 512; one pixel is one."""
    from nerf_qa_amd import ops
    b, ctot, col = 2, c + 8, 5
    tx, ty = _relu_maps((b, h, w, c), 3 * c + h).to(dev), _relu_maps((b, h, w, c), 5 * c + h).to(dev)
    g = torch.Generator().manual_seed(c + h)
    g1, g2 = (torch.randn(b, ctot, generator=g).to(dev) for _ in range(2))
    other = torch.randn(tx.shape, generator=g).to(dev)
    print()
    three_runs(f"dists_stats_nhwc_backward C={c} {h}x{w}",
               lambda p: ops.dists_stats_nhwc_backward(tx, ty, g1, g2, col), monkeypatch, need_ws=False)

    def target(p):
        s1 = torch.zeros(b, ctot, device=dev)
        s2 = torch.zeros(b, ctot, device=dev)
        part = ops.dists_stats_target(tx, ty, s1, s2, col)
        gx, gy = ops.dists_stats_nhwc_backward_from(tx, ty, part, g1, g2, col)
        acc = ops.dists_stats_nhwc_grad_y_add(tx, ty, part, g1, g2, col, other.clone())
        return s1, s2, gx, gy, acc
    runs = three_runs(f"dists_stats_target + backward_from + grad_y_add C={c} {h}x{w}", target, monkeypatch, need_ws=False)
    s1 = runs[0xFF][0]
    assert (s1[:, :col] == 0).all() and (s1[:, col + c:] == 0).all() and s1[:, col:col + c].abs().max().item() > 0

    def exponents(p):
        out = []
        for gmap in (tx, tx.half()):
            for fn in ((ops.grad_exponent, ops.grad_exponent_half) if gmap.dtype == torch.float32 else (ops.grad_exponent_half,)):
                k = torch.empty(b, dtype=torch.int32, device=dev)
                total = torch.full((b,), 3, dtype=torch.int32, device=dev)
                fn(gmap, k, total)
                out += [k, total]
        return out
    runs = three_runs(f"grad_exponent / grad_exponent_half C={c} {h}x{w}", exponents, monkeypatch, need_ws=False)
    assert all(torch.equal(runs[0xFF][i + 1], runs[0xFF][i] + 3) for i in (0, 2, 4))


# ---- 7. the fused stage-closing kernels on their own: partials and seam planes ----------------------------------------
@pytest.mark.parametrize("h,w", [(36, 64), (37, 70)], ids=lambda v: str(v))
def test_fused_conv_pool_entries(h, w, blobs, dev, monkeypatch):
    from nerf_qa_amd import ops
    print()
    for b in (2, 3):
        xc, yc = _frames(b, h, w)
        x, y = xc.to(dev), yc.to(dev)
        three_runs(f"conv1_pool_stats f16 {h}x{w} B={b}", lambda p: ops.conv1_pool_stats(x, y, blobs("f16"), "f16"),
                   monkeypatch, need_ws=False)
        inp = _relu_maps((2 * b, h, w, 128), 9 * h + w + b, torch.float16).to(dev)
        for prec in ("f16", "f16w"):
            three_runs(f"conv_pool_stats {prec} {h}x{w} B={b}", lambda p: ops.conv_pool_stats(inp, 3, blobs(prec), prec),
                       monkeypatch, need_ws=False)


# ---- 8. PIL's resize: an intermediate frame and two tables of bounds and weights in the workspace -------------------
@pytest.mark.parametrize("hin,win,hout,wout", [(37, 53, 64, 80), (90, 61, 45, 61)], ids=lambda v: str(v))
def test_resize_pil(hin, win, hout, wout, dev, monkeypatch):
    from PIL import Image
    from nerf_qa_amd import ops, synth
    img = (synth.uniform(hin * 1000 + win, 2 * hin * win * 3) * 256).astype(np.uint8).reshape(2, hin, win, 3)
    d = torch.from_numpy(img).to(dev)
    print()
    runs = three_runs(f"resize_pil_bilinear_u8 {hin}x{win} -> {hout}x{wout}",
                      lambda p: ops.resize_pil_bilinear_u8(d, (hout, wout), _ws(p)), monkeypatch)
    want = np.stack([np.asarray(Image.fromarray(f).resize((wout, hout), Image.BILINEAR)) for f in img])
    assert np.array_equal(runs[0xFF][0].cpu().numpy(), want)  # (bit-exact with Pillow: test_gpu_fuzz.py::test_random_resize)


# ---- 9. loss steps: forward plus backward() ---------------------------------------------------------------------------
STEP_SHAPES = [(40, 56, 2), (33, 47, 1)]
STEPS = ("dists_one_sided", "dists_target", "adists_auto", "adists_target", "pair_target")


@pytest.mark.parametrize("gp", ["f32s", "f16"])
@pytest.mark.parametrize("h,w,b", STEP_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("step", STEPS)
def test_loss_steps(step, h, w, b, gp, dists, adists, dev, monkeypatch):
    """The loss and y.grad of one optimisation step, bit-equal across the fills.  The target is prepared inside the run,
    so its taps come out of poisoned tensors too."""
    from nerf_qa_amd import pair
    monkeypatch.setattr(dists, "grad_precision", gp)
    monkeypatch.setattr(adists, "grad_precision", gp)
    xc, yc = _frames(b, h, w)
    x, y = xc.to(dev), yc.to(dev)

    def call(p):
        yd = y.detach().clone().requires_grad_()
        if step == "dists_one_sided":
            loss = dists(x, yd, require_grad=True, batch_average=True)
        elif step == "dists_target":
            loss = dists.forward_target(dists.prepare_target(x), yd, require_grad=True, batch_average=True)
        elif step == "adists_auto":
            loss = adists(x, yd)
        elif step == "adists_target":
            loss = adists.forward_target(adists.prepare_target(x), yd)
        else:
            d, a = pair.forward_target(dists, adists, adists.prepare_target(x), yd, batch_average=True)
            loss = d + a
        loss.backward()
        return loss.detach(), yd.grad
    print()
    # (a DISTS target step runs the layer-by-layer pyramid and the statistics kernels: no ops.Workspace anywhere)
    runs = three_runs(f"{step} {h}x{w} B={b} grad_precision={gp}", call, monkeypatch, modules=(dists, adists),
                      need_ws=step != "dists_target")
    loss, grad = runs[0xFF]
    assert torch.isfinite(loss).all() and torch.isfinite(grad).all() and grad.abs().max().item() > 0


# ---- 10. reuse: where stale data actually occurs ----------------------------------------------------------------------
@pytest.mark.parametrize("entry,prec", [("dists", "f16"), ("dists", "f32s"), ("adists", "f32s")])
def test_a_large_call_then_a_small_one_in_one_workspace(entry, prec, blobs, dev, monkeypatch):
    """A 97x131 call followed by a 37x70 call in the same grow-only workspace: the second gets the first's bytes back,
    its partials and seam planes under another layout.  The second call must equal a fresh run -- with a plain
    ops.Workspace (the first call's real data left in place) and with a poisoned one (the whole larger buffer filled)."""
    from nerf_qa_amd import ops
    big, small = [t.to(dev) for t in _frames(2, 97, 131)], [t.to(dev) for t in _frames(2, 37, 70)]
    packed = blobs(prec)
    fn = ops.dists_forward if entry == "dists" else ops.adists_forward
    fresh = [t.detach() for t in _flat(fn(*small, packed, prec, ops.Workspace()))]
    runs = {"a fresh run": fresh}
    stale = ops.Workspace()
    fn(*big, packed, prec, stale)
    size = next(iter(stale.bufs.values())).numel()
    runs["a plain workspace after the 97x131 call"] = [t.detach() for t in _flat(fn(*small, packed, prec, stale))]
    assert next(iter(stale.bufs.values())).numel() == size  # (the same buffer again, not a smaller one)
    print()
    for byte in poison.FILLS:
        with poison.poisoned(byte, monkeypatch=monkeypatch) as p:
            ws = p.workspace()
            fn(*big, packed, prec, ws)
            out = fn(*small, packed, prec, ws)
            torch.cuda.synchronize()
            assert ws.gets == 2 and ws.filled == 2 * size
        print(f"  {entry} {prec} 97x131 then 37x70: {p.report()}")
        p.require()
        runs[f"fill 0x{byte:02X} after the 97x131 call"] = [t.detach() for t in _flat(out)]
    same_results(f"{entry} {prec} 37x70 after 97x131", runs, ref_key="a fresh run")


def test_a_sliced_batch_shares_one_workspace(dists, adists, oracle_convs, dev, monkeypatch):
    """NQA_MAX_WORKSPACE_GB set small (as tests/test_gpu_module.py::test_oversized_batches_are_sliced does): five pairs
    run as slices of 2, 2 and 1 through ONE workspace, the last slice smaller than the buffer it gets."""
    from nerf_qa_amd import ops
    b, h, w = 5, 37, 70
    xc, yc = _frames(b, h, w)
    x, y = xc.to(dev), yc.to(dev)
    monkeypatch.setattr(dists, "precision", "f16")
    print()
    for name, model, bytes_for, kw in (
            ("DISTS f16", dists, lambda n: ops.lib().nqa_workspace_bytes(2 * n, h, w, ops.prec_id("f16")), {}),
            ("ADISTS f32s", adists, lambda n: ops.lib().nqa_adists_workspace_bytes(n, h, w, ops.prec_id("f32s")),
             {"as_loss": False})):
        with torch.no_grad():
            whole = model(x, y, **kw)
        monkeypatch.setenv("NQA_MAX_WORKSPACE_GB", repr(2.5 * bytes_for(1) / (1 << 30)))
        assert ops._max_pairs(bytes_for, b) == 2  # 2, 2, 1

        def module(p):
            with torch.no_grad():
                out = model(x, y, **kw)
            if p is not None:
                assert len(model._ws.bufs) == 1 and model._ws.gets == 3  # one buffer, asked once per slice
            return out
        runs = three_runs(f"{name} module {h}x{w} B={b} in slices of 2", module, monkeypatch, modules=(model,))
        monkeypatch.delenv("NQA_MAX_WORKSPACE_GB")
        # (pairs are independent; only the statistics' block partition follows the batch size: the bound of
        # tests/test_gpu_adists.py::test_adists_two_stream_halves_equal_one_call)
        assert (runs[None][0] - whole).abs().max().item() <= 3e-7
        if model is dists:
            ref, bar = _oracle("dists", b, h, w, oracle_convs, dists), DISTS_BAR["f16"]
        else:
            ref, bar = _oracle("adists", b, h, w, oracle_convs), ADISTS_BAR
        err = (runs[0xFF][0].cpu() - ref).abs().max().item()
        print(f"  {name} sliced: |score - oracle| under fill 0xFF = {err:.2e} (bar {bar:.0e})")
        assert err <= bar, (name, err)
