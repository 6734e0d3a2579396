"""CPU-side checks of the shared-pyramid pair scorer: the C entry point nqa_adists_dists_forward (exported, declared,
argument validation on the host before anything touches a device), the two-column sharded gather under gloo, and the
refusals of pair.score_pair / video.score_video(shared_pyramid=True) that need no GPU work."""
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from nerf_qa_amd import build, _lib
    build.build()
    return _lib.lib()


def test_entry_point_exported_and_declared(lib):
    from nerf_qa_amd import _lib
    assert "nqa_adists_dists_forward" in _lib.EXPORTS
    assert hasattr(lib, "nqa_adists_dists_forward")
    hdr = open(os.path.join(ROOT, "include", "nqa.h")).read()
    assert re.search(r"\bint\s+nqa_adists_dists_forward\s*\(", hdr)
    assert lib.nqa_version() == 1  # adding a function is compatible
    assert len(_lib.K_NAMES) == 7  # NQA_K_COUNT is part of the ABI: no new timing class


def _call(lib, x=0x1000, y=0x2000, B=2, H=32, W=32, packed=0x3000, prec=0, ws=0x4000, ws_bytes=1 << 40, d=0x5000,
          s1=0x6000, s2=0x7000, m=None):
    # (the pointers are never dereferenced: every case below is refused on the host)
    return lib.nqa_adists_dists_forward(x, y, B, H, W, packed, prec, ws, ws_bytes, d, s1, s2, m, None)


@pytest.mark.parametrize("kw", [{"x": None}, {"y": None}, {"packed": None}, {"ws": None}, {"d": None}, {"s1": None},
                                {"s2": None}], ids=lambda kw: "null_" + next(iter(kw)))
def test_null_pointers_are_argument_errors(lib, kw):
    assert _call(lib, **kw) == -1
    assert b"null" in lib.nqa_last_error()


@pytest.mark.parametrize("kw", [{"B": 0}, {"B": -2}, {"H": 0}, {"W": -1}, {"prec": 99}, {"prec": -1}],
                         ids=lambda kw: "%s_%d" % next(iter(kw.items())))
def test_bad_sizes_and_precision_are_argument_errors(lib, kw):
    assert _call(lib, **kw) == -1
    msg = lib.nqa_last_error()
    assert b"bad size or prec" in msg and msg.strip()


def test_short_workspace_and_oversized_image(lib):
    need = lib.nqa_adists_workspace_bytes(2, 32, 32, 0)
    assert need > 0
    assert _call(lib, ws_bytes=need - 1) == -3
    assert b"workspace" in lib.nqa_last_error()
    # the 32-bit in-image byte offset limit of nqa_adists_forward: H * W * 64 channels * 4 bytes >= 2^31
    assert _call(lib, B=1, H=4096, W=2048) == -1
    assert b"32-bit" in lib.nqa_last_error()
    # the same answers as the A-DISTS entry point it extends
    assert lib.nqa_adists_forward(0x1000, 0x2000, 2, 32, 32, 0x3000, 0, 0x4000, need - 1, 0x5000, None) == -3
    assert lib.nqa_adists_forward(0x1000, 0x2000, 1, 4096, 2048, 0x3000, 0, 0x4000, 1 << 40, 0x5000, None) == -1


# ---- two-column sharded gather (video.score_video(shared_pyramid=True): ONE all-gather for both metrics) ------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _table(lo, hi):
    i = torch.arange(lo, hi, dtype=torch.float32)
    return torch.stack([i * 0.5 + 1.0, -i - 0.25], dim=1)


def _worker(rank, world, port, n_frames, batch, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from nerf_qa_amd import sharding
    calls = []

    def two(lo, hi):
        calls.append((lo, hi))
        return _table(lo, hi)

    full = sharding.score_frames_sharded(two, n_frames, batch, torch.device("cpu"), columns=2)
    one = sharding.score_frames_sharded(lambda lo, hi: _table(lo, hi)[:, 0], n_frames, batch, torch.device("cpu"))
    q.put((rank, full.numpy(), one.numpy(), calls))
    dist.destroy_process_group()


@pytest.mark.parametrize("world,n_frames,batch", [(2, 10, 4), (2, 7, 3), (2, 1, 8), (4, 21, 8), (4, 9, 2), (4, 3, 8)],
                         ids=["w2_10", "w2_7_uneven", "w2_1_empty_rank", "w4_21_uneven", "w4_9_last_rank_empty",
                              "w4_3_empty_ranks"])
def test_two_column_gather_on_every_rank(world, n_frames, batch):
    if world == 4 and n_frames == 9:  # ceil(9/4) = 3 frames per rank: ranks 0..2 hold 3 each, rank 3 holds none
        from nerf_qa_amd.sharding import shard_range
        assert shard_range(9, 3, 4) == (9, 9)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n_frames, batch, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = _table(0, n_frames).numpy()
    seen = []
    for rank, full, one, calls in results:
        assert full.shape == (n_frames, 2) and full.dtype == np.float32
        assert np.array_equal(full, want), f"rank {rank} got {full}"
        assert one.shape == (n_frames,) and np.array_equal(one, want[:, 0])  # the one-column call, as before
        seen += calls
    assert sorted(i for lo, hi in seen for i in range(lo, hi)) == list(range(n_frames))


def test_gather_without_process_group_two_columns():
    from nerf_qa_amd import sharding
    t = _table(0, 5)
    assert torch.equal(sharding.gather_scores(t, 5, columns=2), t)
    got = sharding.score_frames_sharded(_table, 11, 4, torch.device("cpu"), columns=2)
    assert got.shape == (11, 2) and torch.equal(got, _table(0, 11))
    one = sharding.score_frames_sharded(lambda lo, hi: _table(lo, hi)[:, 1], 11, 4, torch.device("cpu"))
    assert one.shape == (11,) and torch.equal(one, _table(0, 11)[:, 1])
    empty = sharding.score_frames_sharded(_table, 0, 4, torch.device("cpu"), columns=2)
    assert empty.shape == (0, 2)


# ---- refusals that are reached before any device work ----------------------------------------------------------------
def test_score_pair_refuses_a_named_dists_precision_that_differs():
    import nerf_qa_amd
    from nerf_qa_amd.ADISTS import ADISTS
    from nerf_qa_amd.DISTS_pytorch import DISTS
    x = torch.rand(1, 3, 160, 160)
    with pytest.raises(ValueError, match=r"'f32s'.*'f16'"):  # names both: what the pair runs in, what was asked for
        nerf_qa_amd.score_pair(DISTS(precision="f16"), ADISTS(), x, x)
    with pytest.raises(ValueError, match=r"'f32'.*'f32s'"):  # A-DISTS' auto runs frames this small in exact f32
        nerf_qa_amd.score_pair(DISTS(precision="f32s"), ADISTS(), x[..., :64, :64], x[..., :64, :64])
    with pytest.raises(ValueError, match=r"'f32'.*'f32s'"):
        nerf_qa_amd.score_pair(DISTS(precision="f32s"), ADISTS(precision="f32"), x, x)
    # matching names and DISTS' auto pass this check: the next refusal is the device's (no CPU path)
    for dm, am in ((DISTS(precision="f32s"), ADISTS()), (DISTS(), ADISTS()), (DISTS(precision="fp32"), ADISTS(precision="f32"))):
        with pytest.raises(nerf_qa_amd.NqaError, match="GPU only"):
            nerf_qa_amd.score_pair(dm, am, x, x)


def test_score_pair_refuses_images_that_require_grad_and_bad_shapes():
    import nerf_qa_amd
    from nerf_qa_amd.ADISTS import ADISTS
    from nerf_qa_amd.DISTS_pytorch import DISTS
    dm, am = DISTS(), ADISTS()
    x = torch.rand(2, 3, 32, 32)
    with pytest.raises(ValueError, match="separately"):
        nerf_qa_amd.score_pair(dm, am, x.clone().requires_grad_(True), x)
    with pytest.raises(ValueError, match="separately"):
        nerf_qa_amd.score_pair(dm, am, x, x.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="equal shape"):
        nerf_qa_amd.score_pair(dm, am, x, x[:1])


def test_score_video_shared_pyramid_needs_both_models():
    from nerf_qa_amd import video
    from nerf_qa_amd.ADISTS import ADISTS
    from nerf_qa_amd.DISTS_pytorch import DISTS
    x = torch.rand(3, 3, 32, 32)
    for kw in ({"dists_model": DISTS()}, {"adists_model": ADISTS()}, {}):
        with pytest.raises(ValueError, match="both"):
            video.score_video(x, x, shared_pyramid=True, **kw)
