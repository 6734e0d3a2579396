"""tests/persistent_refs.py without a GPU: the schedule model partitions every launch's tiles, the batches it chooses reach
the persistent regime on every CU count the kernels may meet, and the integer references are exact where the GPU tests
(tests/test_gpu_conv_persistent.py) rely on it -- for the fused stage 1 too: its frames normalise to their integer levels
exactly in half, its sparse weight set keeps relu1_2 in [0, 63], the model of launch_conv1_pool gives every unit one
owner and its batches reach the kernel's regime.  Every precondition is printed."""
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


# ---- the fused conv2_2 at POOL_SHAPES -----------------------------------------------------------------------------------------
def test_pool_shapes_reach_both_instances():
    assert P.POOL_SHAPES[0] == (P.H, P.W)
    assert [P.pool_is_ragged(h, w) for h, w in P.POOL_SHAPES] == [True, False, True, True]
    assert [(h % 4, w % 16) for h, w in P.POOL_SHAPES] == [(1, 6), (0, 0), (0, 6), (2, 0)]
    # the shapes the project exists for run the instance 36 x 64 reaches
    assert not P.pool_is_ragged(128, 128) and not P.pool_is_ragged(540, 960)


@pytest.mark.parametrize("cus", P.CU_COUNTS)
@pytest.mark.parametrize("nct", [1, 2])
@pytest.mark.parametrize("h,w", P.POOL_SHAPES, ids=lambda v: str(v))
def test_pool_batches_reach_the_stronger_regime(h, w, nct, cus):
    """The runs partition the units, the chosen batch is in the stronger regime and a lane's float32 moments between two
    flushes stay exact.  No batch of up to 600 pairs is in the regime where every batch is dealt evenly (36 x 64 with two
    channel tiles on 8 CUs): the chooser returns None there, which this test accepts on every CU count but the MI355X's
    256 -- on the device itself tests/test_gpu_conv_persistent.py fails with that message."""
    strips, rows = P.cdiv(w, 16), P.cdiv(h, 4)
    for b in (1, 2, 3, 7, 11):
        runs, s, r = P.pool_runs(b, h, w, cus, nct)
        units = b * nct * strips * rows
        assert (s, r) == (strips, rows) and len(runs) == min(units, cus, P.PART_BLOCKS)
        covered = np.concatenate([np.arange(lo, hi) for lo, hi, _ in runs])
        assert np.array_equal(np.sort(covered), np.arange(units)), (h, w, nct, cus, b)  # every unit has one owner
        assert all(warm == (lo < hi and lo % rows != 0) for lo, hi, warm in runs)
        owners = {P.pool_owner(n, ct, sx, ty, b, h, w, cus, nct) for n in (0, b - 1) for ct in range(nct)
                  for sx in (0, strips - 1) for ty in (0, rows - 1)}
        assert None not in owners
    b = P.pool_strong_batch_for(h, w, cus, nct)
    if b is None:
        assert cus != 256, f"no batch of {h} x {w} pairs reaches the fused conv2_2's stronger regime on {cus} CUs"
        print(f"\n {cus} CUs fused conv2_2 {h}x{w} nct {nct}: no batch of up to 600 pairs has uneven runs of 4 units")
        return
    r = P.pool_regime(b, h, w, cus, nct)
    print(f"\n {cus} CUs fused conv2_2 {h}x{w} nct {nct} (RAGGED = {P.pool_is_ragged(h, w)}): {b} pairs, {r['units']} units on "
          f"{r['grid']} blocks, {r['least']}..{r['most']} steps per block (at most {r['own']} units of its own, {r['inside']} of "
          f"one pair), {r['warm']} runs start inside a strip, {r['cross']} cross an image pair")
    assert b >= 3 and P.pool_in_strong_regime(r)
    assert r["warm"] >= 1 and r["cross"] >= 1 and r["most"] >= 4 and r["own"] >= 4 and r["least"] < r["most"]
    assert b == 3 or not P.pool_in_strong_regime(P.pool_regime(b - 1, h, w, cus, nct))  # the smallest such batch
    assert cus < 256 or 2 * b <= 52  # (a launch of well under a second)
    # a lane's float32 moments take one sample per pass, four per unit, |deviation| <= 63, between two flushes
    assert 1 <= r["inside"] <= r["own"] and 4 * r["inside"] * 63 ** 2 < 2 ** 24
    # one unit per block: the largest batch whose units all find a block
    one = P.pool_single_unit_batch(h, w, cus, nct)
    per_pair = nct * strips * rows
    assert one * per_pair <= min(cus, P.PART_BLOCKS) < (one + 1) * per_pair
    if one:
        r1 = P.pool_regime(one, h, w, cus, nct)
        assert r1["grid"] == r1["units"] and r1["own"] == 1 and r1["most"] == 2 and r1["cross"] == 0
        assert r1["warm"] == r1["units"] - one * nct * strips  # every run but a strip's first starts with the warm-up


def test_the_stronger_regime_on_the_mi355x_is_the_documented_one():
    """256 CUs: the batches and unit counts of the table in DESIGN.md."""
    want = {(36, 64): (22, 11, 792), (36, 70): (18, 9, 810), (38, 48): (26, 13, 780)}
    for (h, w), (b1, b2, units) in want.items():
        for nct, b in ((1, b1), (2, b2)):
            assert P.pool_strong_batch_for(h, w, 256, nct) == b
            r = P.pool_regime(b, h, w, 256, nct)
            assert (r["units"], r["grid"], r["own"]) == (units, 256, 4) and 3 <= r["least"] < r["most"] <= 5
            assert 224 <= r["warm"] <= 230 and 6 <= r["cross"] <= 16


@pytest.mark.parametrize("h,w", P.POOL_SHAPES, ids=lambda v: str(v))
def test_pool_references_are_exact_at_every_shape(h, w):
    taps = [P.conv_ref(P.SPARSE_LAYER, h, w, sparse=True, seed=s) for s in (0, 1)]
    assert not torch.equal(P.int_base(P.SPARSE_LAYER, h, w, 0), P.int_base(P.SPARSE_LAYER, h, w, 1))
    for seed, tap in enumerate(taps):
        print(f"\n {h}x{w} base triple {seed}: tap in [{tap.min().item():.0f}, {tap.max().item():.0f}], "
              f"{float((tap > 0).double().mean()):.2f} of it positive")
        assert tap.min() >= 0 and tap.max() <= 63 and float((tap > 0).double().mean()) > 0.2
        assert bool((tap == tap.round()).all()) and torch.equal(tap.half().double(), tap)
        s = P.pool_window_sums(tap)
        assert bool((s == s.round()).all()) and s.max().item() <= 16 * 3969 < 2 ** 24
        assert s.shape == (3, (h + 1) // 2, (w + 1) // 2, 128)
        p64, p32 = P.pooled_refs(tap)
        differ = int((p64.view(torch.int16) != p32.view(torch.int16)).sum())
        print(f"   pooled halves of the float32 replay that differ from the float64 reference: {differ} of {p64.numel()}")
        assert differ == 0
    sums = P.five_sums(*taps)
    assert sums.shape == (3, 128, 5) and bool((sums == sums.round()).all()) and sums.max().item() < 2 ** 53


def test_a_carried_row_leaked_into_the_next_strip_shows_only_where_the_last_tap_row_is_live():
    """Why 36 x 64 and 36 x 70 are there: a pooled reference formed with the last tap row of a strip leaked into the first
    pooled row of the next strip (c_keep stuck at 1) is more than half a unit in the last place of half -- and more than
    the GPU test's whole bar -- from the true one where H % 4 = 0, and IDENTICAL to it at 37 x 70 (and 38 x 48), where
    that row lies outside the image and is masked to zero."""
    for h, w in P.POOL_SHAPES:
        tap = P.conv_ref(P.SPARSE_LAYER, h, w, sparse=True)
        true64 = np.sqrt(P.pool_window_sums(tap).numpy() / 16.0 + 1e-12)
        leak64 = np.sqrt(P.leaked_window_sums(tap).numpy() / 16.0 + 1e-12)
        half_ulp = 0.5 * np.spacing(np.maximum(true64, 6.1e-5).astype(np.float16)).astype(np.float64)
        off = np.abs(leak64 - true64) > half_ulp
        ref = true64.astype(np.float16).astype(np.float64)
        over_bar = np.abs(leak64.astype(np.float16).astype(np.float64) - ref) > np.maximum(ref, 6.1e-5) * 2.0 ** -10
        print(f"\n {h}x{w}: {int(off.sum())} of {off.size} pooled values move by more than half a unit in the last place of "
              f"half under the leak, {int(over_bar.sum())} beyond the GPU test's bar; rows hit {sorted(set(np.nonzero(off)[1]))}")
        if h % 4 == 0:
            assert off.any() and over_bar.any()
            assert set(np.nonzero(off)[1]) == {0} and np.nonzero(off)[2].min() >= 8  # the first pooled row, past strip 0
        else:
            assert not off.any() and np.array_equal(leak64, true64)
    # the leak-free form of the same function is the reference itself
    tap = P.conv_ref(P.SPARSE_LAYER, 37, 70, sparse=True)
    assert torch.equal(P.leaked_window_sums(tap), P.pool_window_sums(tap))


# ---- the fused stage 1 ------------------------------------------------------------------------------------------------------
def test_integer_frames_normalise_to_their_levels_exactly_in_half():
    """Both forms of (x - mean) / std the kernels use, replayed in float32 (the fmas through float64: one further rounding
    of ~6e-8 at most, far inside the margin): within 2^-13 of the level -- a quarter of half's spacing below 2, a
    sixteenth of bfloat16's -- so the half (and the bfloat16) is the level itself; level 0 gives exactly 0."""
    for c in range(3):
        for v in P.S1_LEVELS:
            x = P.s1_pixel(c, v)
            assert x.dtype == np.float32 and 0.0 <= x <= 1.0
            assert v != 0 or x == P.S1_MEAN[c]
            for form in ("fused", "div"):
                q = P.s1_normalise(x, c, form)
                print(f" channel {c} level {v:2d}: pixel {x:.9g} -> {form:5s} {q:.9g} (off by {float(q) - v:+.2e})")
                assert q.dtype == np.float32 and abs(float(q) - v) <= 2.0 ** -13 and abs(float(q) - v) <= 5e-7
                assert float(np.float16(q)) == v and float(torch.tensor(float(q)).bfloat16()) == v
                assert v != 0 or q == 0.0


def test_stage1_integer_set_and_references():
    from nerf_qa_amd import ops
    convs = P.s1_convs()
    assert len(convs) == ops.NUM_CONVS and all(np.array_equal(a[0], b[0]) for a, b in zip(convs[2:], P.int_convs()[2:]))
    (w0, b0), (w1, b1) = convs[:2]
    for w, b, terms in ((w0, b0, P.S1_TERMS[0]), (w1, b1, P.S1_TERMS[1])):
        flat = w.reshape(64, -1)
        assert set(np.unique(w)) <= {-1.0, 0.0, 1.0} and bool(((flat != 0).sum(1) == terms).all())
        assert bool((flat != 0).any(0).all())  # every (input channel, tap) position is used by some output channel
        assert bool((b == np.round(b)).all())
    assert int((b0 >= 1).sum()) >= 8 and int((b0 < 0).sum()) >= 8 and set(np.unique(b1)) <= {-1.0, 0.0, 1.0}
    for h, w in P.S1_SHAPES:
        lv = [P.s1_levels(h, w, s) for s in (0, 1)]
        assert not torch.equal(lv[0], lv[1]) and not torch.equal(lv[0][0], lv[0][1])
        assert set(lv[0].unique().tolist()) == set(float(v) for v in P.S1_LEVELS)
        for s in (0, 1):
            fr = P.s1_frames(h, w, s)
            assert fr.dtype == torch.float32 and fr.shape == (3, 3, h, w) and 0.0 <= fr.min() and fr.max() <= 1.0
            for c in range(3):  # the frame is the level's pixel, bit for bit
                for v in P.S1_LEVELS:
                    assert bool((fr[:, c][lv[s][:, c] == v] == float(P.s1_pixel(c, v))).all())
            tap = P.s1_ref(h, w, s)  # (asserts integrality, the partial-sum bounds and relu1_2 <= 63 itself)
            print(f"\n {h}x{w} base triple {s}: relu1_2 in [{tap.min().item():.0f}, {tap.max().item():.0f}], "
                  f"{float((tap > 0).double().mean()):.2f} of it positive")
            assert tap.shape == (3, h, w, 64) and tap.min() >= 0 and tap.max() <= 63 and bool((tap == tap.round()).all())
            assert float((tap > 0).double().mean()) > 0.2 and tap.max() >= 16
            assert torch.equal(tap.half().double(), tap) and torch.equal(tap.bfloat16().double(), tap)
            win = P.pool_window_sums(tap)
            assert bool((win == win.round()).all()) and win.max().item() <= 16 * 3969 < 2 ** 24
            p64, p32 = P.pooled_refs(tap)
            share = float((p64.view(torch.int16) != p32.view(torch.int16)).double().mean())
            print(f"   pooled halves of the float32 replay that differ from the float64 reference: {share:.2e} of {p64.numel()}")
            assert share <= 2e-2 and p64.shape == (3, (h + 1) // 2, (w + 1) // 2, 64)
        sums = P.five_sums(P.s1_ref(h, w, 0), P.s1_ref(h, w, 1))
        assert sums.shape == (3, 64, 5) and bool((sums == sums.round()).all()) and sums.max().item() < 2 ** 53


@pytest.mark.parametrize("cus", P.CU_COUNTS)
def test_every_stage1_unit_has_exactly_one_owner(cus):
    for h, w in P.S1_SHAPES + ((4, 32), (5, 33), (1080, 1920)):
        for b in (1, 2, 3, 7) if h < 1080 else (1,):
            runs, spairs, rows = P.s1_runs(b, h, w, cus)
            units = b * spairs * rows
            assert len(runs) == min(units, cus, 256) and (spairs, rows) == (P.cdiv(w, 32), P.cdiv(h, 4))
            own = P.s1_owners(b, h, w, cus)
            assert len(own) == units and all(len(v) == 1 for v in own.values()), (h, w, b, cus)
            assert set(own) == {(n, sp, ty) for n in range(b) for sp in range(spairs) for ty in range(rows)}
            blk, step = own[(b - 1, spairs - 1, rows - 1)][0]
            lo, hi, warm = runs[blk]
            assert hi == units and step == hi - lo - 1 + warm
            assert all(warm == (lo < hi and lo % rows != 0) for lo, hi, warm in runs)
    # pool_runs is the same rule with other units: its runs are unit_runs'
    runs, strips, rows = P.pool_runs(6, P.H, P.W, cus, 2)
    assert runs == P.unit_runs(6 * 2 * strips * rows, min(6 * 2 * strips * rows, cus, P.PART_BLOCKS), rows)


@pytest.mark.parametrize("cus", P.CU_COUNTS)
def test_stage1_batches_reach_the_fused_kernels_regime(cus):
    for h, w in P.S1_SHAPES:
        b = P.s1_batch_for(h, w, cus)
        r = P.s1_regime(b, h, w, cus)
        print(f"\n {cus} CUs fused stage 1 {h}x{w}: {b} pairs, {r['units']} units on {r['grid']} blocks, {r['least']}..{r['most']} "
              f"steps per block (at most {r['own']} units of its own, {r['inside']} of one pair), {r['warm']} runs start inside a "
              f"strip, {r['cross']} cross an image pair")
        assert b % 3 == 0 and P.s1_in_regime(r)
        assert r["warm"] >= 1 and r["cross"] >= 1 and r["most"] >= 4 and r["own"] >= 4 and r["least"] < r["most"]
        assert b == 3 or not P.s1_in_regime(P.s1_regime(b - 3, h, w, cus))  # the smallest such batch
        assert cus < 256 or 2 * b * h * w <= 64 * 150 * 130  # (a launch of well under a second)
        # a lane's float32 moments take one sample per pass, four per unit, |deviation| <= 63, between two flushes
        assert 1 <= r["inside"] <= r["own"] and 4 * r["inside"] * 63 ** 2 < 2 ** 24
        # the conv1_regw companions of the same frames
        if (h, w, cus) == (64, 96, 8):  # 24 tiles per image on 8 blocks: every batch is dealt evenly, no uneven tail
            with pytest.raises(AssertionError, match="no batch"):
                P.batch_for("conv1_regw", h, w, cus)
            continue
        n = P.batch_for("conv1_regw", h, w, cus)
        assert n % 3 == 0 and P.in_regime(P.regime("conv1_regw", n, h, w, cus))
    # one pair of 150 x 130: one unit per block where the device has the CUs, most runs start with a warm-up
    r = P.s1_regime(1, P.S1_H, P.S1_W, cus)
    assert r["units"] == 190 and r["grid"] == min(190, cus, 256)
    if cus >= 190:
        assert r["own"] == 1 and r["most"] == 2 and r["warm"] == 190 - 5 and r["cross"] == 0
