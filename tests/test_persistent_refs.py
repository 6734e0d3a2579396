"""tests/persistent_refs.py without a GPU: the schedule model partitions every launch's tiles, the batches it chooses reach
the persistent regime on every CU count the kernels may meet, and the integer references are exact where the GPU tests
(tests/test_gpu_conv_persistent.py) rely on it.  Every precondition is printed."""
import numpy as np
import pytest
import torch

import persistent_refs as P

# (kernel, channel tiles): every grid rule; regw covers conv1_regw and conv1_regw_split (the same rule and split)
MODELS = [("regw", 1), ("regw128", 1), ("regw128", 2), ("regw128", 4), ("regw_split", 1), ("regw_split", 2)]


@pytest.mark.parametrize("cus", P.CU_COUNTS)
@pytest.mark.parametrize("kernel,nct", [m for m in MODELS if m[1] <= 2], ids=lambda v: str(v))
def test_every_tile_has_exactly_one_owner(kernel, nct, cus):
    for total in range(1, 3001):
        units = total * nct if kernel == "regw_split" else total  # (regw128's total already counts its channel tiles)
        got = np.sort(P.flat_tiles(kernel, total, cus, nct))
        assert got.size == units and got[0] == 0 and got[-1] == units - 1 and bool((np.diff(got) == 1).all()), \
            f"{kernel} nct {nct}: {total} tiles on {cus} CUs are not dealt once each (grid {P.grid_for(kernel, total, cus, nct)})"


def test_the_list_form_of_the_model_is_the_array_form():
    for kernel, nct in MODELS:
        for total, cus in ((1, 256), (7, 8), (100, 256), (810, 256), (1531, 104), (2999, 304)):
            lists = P.block_tiles(kernel, total, cus, nct)
            assert len(lists) == P.grid_for(kernel, total, cus, nct)
            assert [t for ts in lists for t in ts] == P.flat_tiles(kernel, total, cus, nct).tolist()
            assert P.owners(kernel, total, cus, nct)[lists[-1][-1] if lists[-1] else 0] is not None


def test_the_trimmed_grid_of_the_issue_example():
    """conv3_1 in f16 on 1 x 20 x 300, 256 CUs: 100 tiles, grid trimmed from 100 to 92, class stride 11 on XCDs 4..7."""
    total = P.total_tiles("regw128", 1, 20, 300, 2)
    first, stride, count = P.block_walks("regw128", total, 256, 2)
    assert total == 100 and first.size == 92 and stride[:4].tolist() == [12] * 4 and stride[4:8].tolist() == [11] * 4
    assert P.reloads(total, 256, 2) and all(b % 8 >= 4 for b in P.reloads(total, 256, 2))


# the launches of tests/test_gpu_conv_persistent.py: (kernel, channel tiles, H, W)
LAUNCHES = [("regw", 1, P.H, P.W), ("regw_split", 2, P.H, P.W), ("regw128", 1, P.H, P.W), ("regw128", 2, P.H, P.W),
            ("regw128", 4, P.H, P.W), ("conv1_regw", 1, P.S1_H, P.S1_W), ("conv1_regw_split", 1, P.S1_H, P.S1_W)]


@pytest.mark.parametrize("cus", P.CU_COUNTS)
def test_batches_reach_the_persistent_regime(cus):
    for kernel, nct, h, w in LAUNCHES:
        if (kernel, nct, cus) == ("regw128", 4, 8):
            # 120 tiles per image on 8 blocks, one per XCD class: every batch is dealt evenly, so no batch has an uneven
            # tail there and batch_for says so (four channel tiles on an 8-CU device: the one combination without a case)
            assert all(P.regime(kernel, n, h, w, cus, nct)["least"] * 8 == 120 * n for n in range(1, 130))
            with pytest.raises(AssertionError, match="no batch"):
                P.batch_for(kernel, h, w, cus, nct)
            continue
        n = P.batch_for(kernel, h, w, cus, nct)
        r = P.regime(kernel, n, h, w, cus, nct)
        print(f"\n {cus} CUs {kernel} nct {nct} {h}x{w}: batch {n}, {r['total']} tiles on {r['grid']} blocks, "
              f"{r['least']}..{r['most']} tiles per block")
        assert n % 3 == 0 and P.in_regime(r) and r["most"] >= 4 and r["least"] < r["most"]
        if (h, w) == (P.H, P.W):
            assert n <= 128
        assert n == 3 or not P.in_regime(P.regime(kernel, n - 3, h, w, cus, nct))  # the smallest such batch
    for nct in (1, 2):
        b = P.pool_batch_for(P.H, P.W, cus, nct)
        r = P.pool_regime(b, P.H, P.W, cus, nct)
        print(f"\n {cus} CUs fused conv2_2 nct {nct}: {b} pairs, {r['units']} units on {r['grid']} blocks, {r['least']}.."
              f"{r['most']} steps per block, {r['warm']} runs start inside a strip, {r['cross']} cross an image pair")
        assert b % 3 == 0 and 2 * b <= 128 and P.pool_in_regime(r)
        runs, strips, rows = P.pool_runs(b, P.H, P.W, cus, nct)
        assert runs[0][0] == 0 and sorted(lo for lo, _, _ in runs)[1:] == sorted(hi for _, hi, _ in runs)[:-1]
        assert max(hi for _, hi, _ in runs) == r["units"]  # contiguous runs that cover every unit once


@pytest.mark.parametrize("cus", P.CU_COUNTS)
def test_reload_case_makes_a_block_change_its_channel_tile(cus):
    for nct in (2, 4):  # conv3_1: 256 channels in blocks of 128 (one-term) or 64 (two-term)
        n, h, w = P.reload_case(cus, nct)
        total = P.total_tiles("regw128", n, h, w, nct)
        blocks = P.reloads(total, cus, nct)
        tiles = P.block_tiles("regw128", total, cus, nct)
        print(f"\n {cus} CUs conv3_1 nct {nct}: {n}x{h}x{w}, {total} tiles on {len(tiles)} blocks, {len(blocks)} blocks reload; "
              f"block {blocks[0]} walks {tiles[blocks[0]][:4]}")
        assert blocks and n * h * w <= 128 * P.H * P.W
        ts = tiles[blocks[0]]
        assert len(ts) >= 2 and ts[0] % nct != ts[1] % nct


def test_integer_references_are_exact():
    from nerf_qa_amd import ops
    for layer in P.INT_LAYERS:
        bound = P.partial_sum_bound(layer, P.H, P.W)
        ref = P.conv_ref(layer, P.H, P.W)
        print(f"\n layer {layer}: partial sums <= {bound:.0f} < 2^24, largest output {ref.max().item():.0f}")
        assert bound < 2 ** 24 and bound <= 2 * 9 * ops.CONV_CIN[layer] + 3
        assert ref.shape == (3, P.H, P.W, ops.CONV_COUT[layer]) and bool((ref == ref.round()).all()) and ref.min() >= 0
        assert torch.equal(P.round_to(ref, torch.float32).double(), ref)
        assert float((ref > 0).double().mean()) > 0.2  # (a reference of zeros would pin nothing)
    w, b = P.sparse_convs()[P.SPARSE_LAYER]
    nz = (w.reshape(w.shape[0], -1) != 0).sum(1)
    assert nz.max() <= P.SPARSE_TERMS and set(np.unique(w)) <= {-1.0, 0.0, 1.0} and set(np.unique(b)) <= {-1.0, 0.0, 1.0}
    for seed in (0, 1):
        tap = P.conv_ref(P.SPARSE_LAYER, P.H, P.W, sparse=True, seed=seed)
        print(f"\n sparse conv2_2, base triple {seed}: tap in [{tap.min().item():.0f}, {tap.max().item():.0f}], "
              f"{float((tap > 0).double().mean()):.2f} of it positive")
        assert tap.min() >= 0 and tap.max() <= 63 and float((tap > 0).double().mean()) > 0.2
        assert torch.equal(tap.half().double(), tap)  # the tap's half store is exact
    # a lane's float32 moments of deviations from a pivot: |d| <= 63, at most H * W samples -> exact integers
    assert 3969 * P.H * P.W < 2 ** 24
    assert not torch.equal(P.int_base(3, P.H, P.W, 0), P.int_base(3, P.H, P.W, 1))


def test_the_float32_replay_of_the_pool_equals_the_float64_one():
    tap = P.conv_ref(P.SPARSE_LAYER, P.H, P.W, sparse=True)
    s = P.pool_window_sums(tap)
    assert bool((s == s.round()).all()) and s.max().item() <= 16 * 3969 and s.shape == (3, 19, 35, 128)
    p64, p32 = P.pooled_refs(tap)
    differ = int((p64.view(torch.int16) != p32.view(torch.int16)).sum())
    print(f"\n pooled halves of the float32 replay that differ from the float64 reference: {differ} of {p64.numel()}")
    assert differ == 0
    x, y = tap, P.conv_ref(P.SPARSE_LAYER, P.H, P.W, sparse=True, seed=1)
    sums = P.five_sums(x, y)
    assert sums.shape == (3, 128, 5) and bool((sums == sums.round()).all()) and sums.max().item() < 2 ** 53
