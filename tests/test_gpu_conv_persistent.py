"""The persistent register-weights convolutions (nqa_conv.hip), the fused conv2_2 + pool + statistics kernel
(nqa_conv_pool.hip) and the fused stage 1 (nqa_conv1_pool.hip) against exact references IN THE REGIME IN WHICH THEIR SCHEDULING CODE RUNS (GPU box only).

Their grid is min(tiles, CUs); a block walks its tiles through a two- or three-slot LDS-DMA ring that it retires with one
counted vmcnt per tile, and takes its tile list from an XCD-aware split.  With at most one tile per block -- all that the
small maps of the operator tests give a 256-CU device -- the ring never wraps, the counted wait behind a previous tile's
stores never runs and the dummy halo past the last tile is the only second issue.  Here every launch is sized by the
schedule model of tests/persistent_refs.py from the device's CU count so that some block owns at least 4 tiles and some
block fewer than another; the test asserts that before it launches and prints the regime.

Every output tensor is passed in (`out=`, `pooled=`, `sums=`) pre-filled with 0xFF bytes -- NaN in half, bfloat16,
float, split16 records and float64 -- and each test asserts first that no NaN is left: a store the kernel skipped cannot
hide behind an allocator block that still holds an earlier, correct result.

Integer cases (operands of tests/persistent_refs.py: every partial sum an integer below 2^24, so the output must be
BIT-EQUAL to relu(conv2d) in float64 rounded once), 37 x 70 maps, ragged under the 8 x 32 and the 4 x 32 tile.  The
instance launch_conv reaches (read off nqa_conv.hip; W >= 16, default conv variant):
  conv2_1 (layer 2)  f16, bf16   conv3x3_regw_kernel<P, 4, 1>          three-slot ring, 8 x 32 tiles
  conv2_1            f16w        conv3x3_regw_kernel<PrecF16, 4, 2>    two-term weights
  conv2_1            f32s        conv3x3_regw_split_kernel             split16 in and out (decoded), 4 x 32, two halves
  conv1_2 (layer 1)  f16w        conv3x3_regw_kernel<PrecF16, 2, 2>    (one-term conv1_2 is the implicit GEMM's)
  conv2_2 (layer 3)  f16, bf16   conv3x3_regw128_kernel<P, 3, 1>       two-slot ring, one channel tile
  conv2_2            f16w        conv3x3_regw128_kernel<PrecF16, 3, 2> two channel tiles of 64
  conv3_1 (layer 4)  f16, bf16   conv3x3_regw128_kernel<P, 3, 1>       two channel tiles of 128
  conv3_1            f16w        conv3x3_regw128_kernel<PrecF16, 3, 2> four channel tiles of 64
plus conv3_1 on the small maps of persistent_refs.reload_case, where a block's consecutive tiles belong to different
channel tiles (load_weights + vmcnt(0) inside the tile loop).  The conv variant carries + 512 (the implicit GEMM's mixed
grid on every 70-wide map), so ops.mixed_grid_launches() == 0 shows that no implicit-GEMM kernel ran for these layers.
A failure names the pixels, rows, columns and channels hit and, from the model, the blocks that own the failing tiles and
the step (and ring slot) of their walk: a ring bug follows the step, an address bug the position.

Stage 1 on random frames, 150 x 130, image k = base[k % 3]: the copies of a base image sit at different tile indices,
owned by different blocks at different ring positions, and must be bit-equal within the launch; the three distinct images
meet the bars these kernels are held to at small sizes (tests/test_gpu_ops.py: 3 x OUT_RTOL against F.conv2d in f16 /
bf16, 2e-6 of the largest activation against float64 in f32s; tests/test_gpu_mixed_layers.py: the float64 replay of
mixed_refs with 4 x the float32 replay's own distance and share in f16w).

Stage 1 on integers.  The normalisation does not stand in the way: a raw pixel float32(mean_c + std_c v), v in {-1, 0, 1,
2}, normalises to a float32 within 5e-7 of v by the fused kernel's corrected reciprocal and by conv1_regw_kernel's
division alike (tests/test_persistent_refs.py replays both), i.e. to exactly v in half and bfloat16.  With the sparse
integer conv1_1 and conv1_2 of persistent_refs.s1_convs (relu1_2 in [0, 63]):
  conv1_regw_kernel<P> (f16, bf16), <PrecF16, 2> (f16w) through ops.conv1_fused, batches of batch_for("conv1_regw"):
    BIT-EQUAL to relu1_2 in float64 rounded once (f32s stays on the random frames here: its normalised pixel is a float32,
    and its exact frames, with lo halves, are those of tests/test_gpu_stage1_split_exact.py);
  conv1_pool_kernel<RAGGED> + pool_seam_kernel + part_reduce_kernel (nqa_conv1_pool.hip) through ops.conv1_pool_stats,
    x and y from two base triples, 150 x 130 (H % 4 = 2, W % 32 = 2: the last unit's second half-strip wholly outside),
    37 x 70 (H odd: the last pooled row from one tap row), 64 x 96 (full units: the other instance) and 36 x 70 (the
    ragged instance with a live last row in every strip: the reset of the carried row above), a batch in which
    some run starts inside a strip (the warm-up unit), some run crosses a pair (flush_stats inside the loop), some run has
    at least 4 units of its own (both halo slots, raw patches and exchange buffers reused, the counted vmcnt(2 * NST))
    and runs are uneven; and one pair of 150 x 130, one unit per block, most behind a warm-up.  The bars of the fused
    conv2_2 below: pooled halves within one unit in the last place of half(sqrt(S / 16 + 1e-12)) in float64, at most 2e-2
    of them differing at all, copies bit-equal, the sums EXACTLY the float64 sums (a lane's moments: 4 samples per unit,
    |deviation| <= 63, below 2^24 by the model's longest run inside a pair).

The fused conv2_2 on the sparse integer set (tap in [0, 63]), x images then y images from another base triple, at the
maps of persistent_refs.POOL_SHAPES.  The instance conv_pool_stats_fused reaches (RAGGED = H % 4 or W % 16; NTERM = 1 in
f16, one channel tile of 128; NTERM = 2 in f16w and f32m, two of 64):
  37 x 70  conv3x3_regw128_pool_kernel<NTERM, true, false>   a strip's last tile has ONE live row, its last tap row is masked
  36 x 64  conv3x3_regw128_pool_kernel<NTERM, false, false>  what 256^2 and 1080p frames run: no masking code, PF = 3
                                                             fragment sets in flight; every strip's last tile fully live
  36 x 70  conv3x3_regw128_pool_kernel<NTERM, true, false>   a live last row in every strip, a last strip 6 columns wide
  38 x 48  conv3x3_regw128_pool_kernel<NTERM, true, false>   only H ragged (H % 4 = 2): the last pooled row completes in pass 1
At 37 x 70 the batch is pool_batch_for's: some block's run starts inside a strip (warm-up step), some block's run crosses
an image pair (statistics flush inside the loop), some run has 4 steps.  At the other three it is the stronger regime the
fused stage 1 is held in: in addition some run has at least 4 units of its own and runs are uneven.  Only where a strip's
last tap row is live (H % 4 = 0) can a carried row that is not dropped at a strip change (c_keep) show: at 37 x 70 that row
is masked to zero (tests/test_persistent_refs.py shows both on the references alone).  (What these maps found in the
two-term instances: the last tap row of a channel tile took the NEXT tile's bias, loaded with its weights before the
previous step's last epilogue had run -- the last pooled row of the last strip, in f16w and f32m.)  36 x 64 also runs with the largest
batch that leaves every block ONE unit: most runs are a warm-up step, the wait vmcnt(NST) behind it, one unit and the
drain.  Pooled map: within one unit in the last place of half of sqrt(S / 16 + 1e-12) in float64, at most 2e-2 of the
values differing at all (the cap of test_gpu_conv_pool.py; the reference's float32 replay differs in none), image k
bit-equal to image k % 3 within each half of the batch.  Sums: EXACTLY the float64 sums -- read off the kernel: the pivot,
the deviations, their float32 moments (4 samples per unit, |deviation| <= 63, below 2^24 by the model's longest run inside
a pair), the float64 conversion in flush_stats, the shuffles and part_reduce_kernel all stay on integers below 2^53."""
import pytest
import torch
import torch.nn.functional as F

import mixed_refs as R
import persistent_refs as P
from test_gpu_ops import OUT_RTOL

pytestmark = pytest.mark.gpu

DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f16w": torch.float16, "f32s": torch.float32, "f32m": torch.float16}
BITS = {torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32}
# (layer, mode, the model's kernel, channel tiles | halves, output channels per block)
INT_CASES = [(2, "f16", "regw", 1, 128), (2, "bf16", "regw", 1, 128), (2, "f16w", "regw", 1, 128),
             (2, "f32s", "regw_split", 2, 64), (1, "f16w", "regw", 1, 64),
             (3, "f16", "regw128", 1, 128), (3, "bf16", "regw128", 1, 128), (3, "f16w", "regw128", 2, 64),
             (4, "f16", "regw128", 2, 128), (4, "bf16", "regw128", 2, 128), (4, "f16w", "regw128", 4, 64)]
_ID = lambda v: str(v)  # noqa: E731


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


@pytest.fixture(scope="module")
def blob(np_convs, dev):
    """blob(kind, mode): the packed weights, made on first use."""
    made = {}

    def get(kind, prec):
        if (kind, prec) not in made:
            from nerf_qa_amd import ops
            convs = {"int": P.int_convs, "sparse": P.sparse_convs, "s1": P.s1_convs, "random": lambda: np_convs}[kind]()
            made[kind, prec] = ops.pack_vgg_weights(convs, prec).to(dev)
        return made[kind, prec]
    return get


def _nan_filled(shape, dtype, dev):
    t = torch.empty(shape, dtype=dtype, device=dev)
    t.view(torch.uint8).fill_(0xFF)
    assert bool(torch.isnan(t).all())
    return t


def _no_nan_left(t, what):
    """t: (images, rows, columns, ...) in any float type (split16 records: viewed as their halves)."""
    nan = torch.isnan(t).reshape(*t.shape[:3], -1).any(dim=3)
    if bool(nan.any()):
        bad = nan.nonzero().cpu()
        raise AssertionError(f"{what}: {bad.shape[0]} pixels were never written (the NaN fill is still there); first (image, "
                             f"row, column) {bad[:8].tolist()}; rows hit {sorted(set(bad[:, 1].tolist()))[:16]}; columns hit "
                             f"{sorted(set(bad[:, 2].tolist()))[:16]}")


def _walk_report(kernel, bad_elems, n, h, w, cus, nct, bc):
    """Which blocks own the tiles of the failing (image, row, column, channel) elements, and at which step of their walk."""
    total = P.total_tiles(kernel, n, h, w, nct)
    own, ring = P.owners(kernel, total, cus, nct), P.KERNELS[kernel]["ring"]
    hit = sorted({own[P.tile_of(kernel, i, r, c, ch, h, w, nct, bc)] for i, r, c, ch in bad_elems.tolist()})
    steps = sorted({s for _, s in hit})
    return (f"{len(hit)} (block, step) walks hit, first {hit[:8]}; steps hit {steps} (ring slots {sorted({s % ring for s in steps})} "
            f"of {ring}); blocks hit {sorted({b for b, _ in hit})[:16]}")


def _assert_bit_equal(got, ref, what, kernel, n, h, w, cus, nct, bc):
    """got, ref: (n, h, w, C) CPU tensors of one dtype."""
    same = got.view(BITS[got.dtype]) == ref.view(BITS[ref.dtype])
    print(f"   {int((~same).sum())} of {same.numel()} values differ; largest expected value {ref.float().max().item():.0f}")
    if not bool(same.all()):
        elems = (~same).nonzero()
        bad = (~same).any(dim=3).nonzero()
        ch = sorted(set(elems[:, 3].tolist()))
        raise AssertionError(f"{what}: {bad.shape[0]} pixels differ from the float64 convolution; first (image, row, column) "
                             f"{bad[:6].tolist()}; rows hit {sorted(set(bad[:, 1].tolist()))}; columns hit "
                             f"{sorted(set(bad[:, 2].tolist()))}; channels hit {ch[:8]} .. {ch[-1]}; "
                             + _walk_report(kernel, elems[:4096], n, h, w, cus, nct, bc))


def _run_int_conv(layer, prec, n, h, w, blob, dev):
    """One launch of the integer layer on image k = base[k % 3] into a NaN-filled out=; (output as floats of its storage
    type on the CPU, the reference rounded once to that type)."""
    from nerf_qa_amd import ops
    a = P.batch_of(P.int_base(layer, h, w), n).to(DT[prec]).to(dev)
    inp = ops.split16_encode(a) if prec == "f32s" else a
    out = _nan_filled((n, h, w, ops.CONV_COUT[layer]), DT[prec], dev)
    ops.set_conv_variant(ops.DEFAULT_CONV_VARIANT | ops.CONV_MIXED_GRID)
    try:
        ops.mixed_grid_launches()
        res = ops.conv3x3_relu(inp, layer, blob("int", prec), prec, out=out)
        launched = ops.mixed_grid_launches()
    finally:
        ops.set_conv_variant(ops.DEFAULT_CONV_VARIANT)
    assert res is out and launched == 0, f"an implicit-GEMM kernel ran ({launched} mixed grids)"
    what = f"layer {layer} [{prec}] {n}x{h}x{w}"
    if prec == "f32s":  # split16 records out: conv2_1 is no tapped layer
        assert layer not in ops.TAP_LAYERS
        _no_nan_left(out.view(torch.float16), what)
        got = ops.split16_decode(out).cpu()
    else:
        _no_nan_left(out, what)
        got = out.cpu()
    ref = P.batch_of(P.round_to(P.conv_ref(layer, h, w), DT[prec]), n)
    return got, ref, what


@pytest.mark.parametrize("layer,prec,kernel,nct,bc", INT_CASES, ids=_ID)
def test_integer_operands_are_bit_exact_past_one_tile(layer, prec, kernel, nct, bc, blob, cus, dev):
    n = P.batch_for(kernel, P.H, P.W, cus, nct)
    r = P.regime(kernel, n, P.H, P.W, cus, nct)
    print(f"\n layer {layer} [{prec}] {kernel}: {n}x{P.H}x{P.W}, {r['total']} tiles on {r['grid']} blocks of {cus} CUs, "
          f"{r['least']}..{r['most']} tiles per block, ring of {r['ring']}")
    assert P.in_regime(r) and r["most"] >= 4 and r["least"] < r["most"] and r["dummy_halo"], r
    got, ref, what = _run_int_conv(layer, prec, n, P.H, P.W, blob, dev)
    _assert_bit_equal(got, ref, what, kernel, n, P.H, P.W, cus, nct, bc)


@pytest.mark.parametrize("prec,nct,bc", [("f16", 2, 128), ("f16w", 4, 64)], ids=_ID)
def test_conv3_1_reloads_its_weights_between_tiles(prec, nct, bc, blob, cus, dev):
    shapes = [P.reload_case(cus, nct)]
    if (1, 20, 300) not in shapes and P.reloads(P.total_tiles("regw128", 1, 20, 300, nct), cus, nct):
        shapes.append((1, 20, 300))  # (a trimmed grid with an odd class stride on 256 CUs)
    for n, h, w in shapes:
        total = P.total_tiles("regw128", n, h, w, nct)
        blocks, tiles = P.reloads(total, cus, nct), P.block_tiles("regw128", total, cus, nct)
        print(f"\n layer 4 [{prec}] regw128: {n}x{h}x{w}, {total} tiles on {len(tiles)} blocks of {cus} CUs, {len(blocks)} blocks "
              f"reload their weights; block {blocks[0]} walks {tiles[blocks[0]]}")
        ts = tiles[blocks[0]]
        assert len(ts) >= 2 and ts[0] % nct != ts[1] % nct
        got, ref, what = _run_int_conv(4, prec, n, h, w, blob, dev)
        _assert_bit_equal(got, ref, what, "regw128", n, h, w, cus, nct, bc)


# ---- stage 1 --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stage1_refs(np_convs):
    """The three base frames and their references, made on first use: ("f32", F.conv2d in float32), ("f64", float64),
    ("replay", mixed_refs' float64 replay of the two-term kernel's rounding points, its float32 replay's distance and share)."""
    x = R.image((3, 3, P.S1_H, P.S1_W), 21)
    made = {}

    def get(kind):
        if kind not in made:
            (w0, b0), (w1, b1) = ((torch.from_numpy(w), torch.from_numpy(b)) for w, b in np_convs[:2])
            if kind == "replay":
                r64, r32 = R.fused_stage1_ref(x, torch.float64), R.to_half(R.fused_stage1_ref(x, torch.float32))
                made[kind] = (r64, R.rel_to_max(r32, r64), R.share_of_halves_differing(r32, r64))
            else:
                dt = torch.float32 if kind == "f32" else torch.float64
                mean, std = torch.tensor(R.MEAN, dtype=dt).view(1, 3, 1, 1), torch.tensor(R.STD, dtype=dt).view(1, 3, 1, 1)
                h = F.relu(F.conv2d((x.to(dt) - mean) / std, w0.to(dt), b0.to(dt), padding=1))
                made[kind] = F.relu(F.conv2d(h, w1.to(dt), b1.to(dt), padding=1))
        return made[kind]
    return x, get


@pytest.mark.parametrize("prec", ["f16", "bf16", "f16w", "f32s"])
def test_stage1_copies_are_bit_equal_and_each_meets_its_small_size_bar(prec, stage1_refs, blob, cus, dev):
    """conv1_regw_kernel<P> (f16, bf16), conv1_regw_kernel<PrecF16, 2> (f16w), conv1_regw_split_kernel (f32s) through
    ops.conv1_fused (nqa_conv.hip conv1_fused: the default stage-1 variant)."""
    from nerf_qa_amd import ops
    kernel = "conv1_regw_split" if prec == "f32s" else "conv1_regw"
    h, w = P.S1_H, P.S1_W
    n = P.batch_for(kernel, h, w, cus)
    r = P.regime(kernel, n, h, w, cus)
    print(f"\n stage 1 [{prec}] {kernel}: {n}x{h}x{w}, {r['total']} tiles on {r['grid']} blocks of {cus} CUs, "
          f"{r['least']}..{r['most']} tiles per block, ring of {r['ring']}")
    assert P.in_regime(r) and r["most"] >= 4 and r["least"] < r["most"] and r["dummy_halo"], r
    x, ref_of = stage1_refs
    out = _nan_filled((n, h, w, 64), DT[prec], dev)
    assert ops.conv1_fused(P.batch_of(x, n).to(dev), blob("random", prec), prec, out=out) is out
    what = f"stage 1 [{prec}] {n}x{h}x{w}"
    _no_nan_left(out, what)
    got = out.cpu()
    bits = got.view(BITS[got.dtype])
    same = bits == bits[torch.arange(n) % 3]
    if not bool(same.all()):
        elems = (~same).nonzero()
        bad = (~same).any(dim=3).nonzero()
        raise AssertionError(f"{what}: {bad.shape[0]} pixels of the copies differ from images 0..2; first (image, row, column) "
                             f"{bad[:6].tolist()}; rows hit {sorted(set(bad[:, 1].tolist()))}; columns hit "
                             f"{sorted(set(bad[:, 2].tolist()))}; " + _walk_report(kernel, elems[:4096], n, h, w, cus, 1, 64))
    first = got[:3].permute(0, 3, 1, 2)
    if prec in ("f16", "bf16"):
        ref = ref_of("f32")
        err, scale = (first.float() - ref).abs().max().item(), ref.abs().max().item() + 1e-30
        print(f"   max |out - conv2d| = {err / scale:.2e} of the map's scale (bar {3 * OUT_RTOL[prec]:.1e})")
        assert err <= 3 * OUT_RTOL[prec] * scale, (err, scale)
    elif prec == "f32s":
        ref = ref_of("f64")
        err = (first.double() - ref).abs().max().item() / ref.abs().max().item()
        print(f"   {err:.2e} of the largest activation from float64 (bar 2e-6)")
        assert err <= 2e-6, err
    else:
        r64, own, own_share = ref_of("replay")
        err, share = R.rel_to_max(first, r64), R.share_of_halves_differing(first, r64)
        print(f"   {err:.2e} of the maximum from the float64 replay (float32 replay: {own:.2e}, bar {4 * own:.2e}); {share:.2e} of "
              f"the outputs differ from its halves (float32 replay: {own_share:.2e}, cap {4 * own_share:.2e})")
        assert err <= 4 * own and share <= 4 * own_share, (err, own, share, own_share)


# ---- the fused conv2_2 + pool + statistics ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool_refs():
    """refs(h, w): taps of the two base triples on the sparse set, the pooled references (three x images, three y images)
    and the five sums of pair k = (x base k, y base k); made on first use, once for all modes."""
    made = {}

    def get(h, w):
        if (h, w) not in made:
            tx, ty = (P.conv_ref(P.SPARSE_LAYER, h, w, sparse=True, seed=s) for s in (0, 1))
            assert tx.max() <= 63 and ty.max() <= 63
            made[h, w] = (P.pooled_refs(tx)[0], P.pooled_refs(ty)[0], P.five_sums(tx, ty))
        return made[h, w]
    return get


# (H, W, batch): "regime" = the model's batch (37 x 70: pool_batch_for, as ever; the others: the stronger regime);
# "single" = the largest batch that leaves every block one unit
POOL_CASES = [(h, w, "regime") for h, w in P.POOL_SHAPES] + [(36, 64, "single")]


@pytest.mark.parametrize("prec,nct", [("f16", 1), ("f16w", 2), ("f32m", 2)], ids=_ID)
@pytest.mark.parametrize("h,w,batch", POOL_CASES, ids=_ID)
def test_fused_conv_pool_stats_on_integers_past_one_unit(h, w, batch, prec, nct, pool_refs, blob, cus, dev):
    """conv3x3_regw128_pool_kernel<NTERM, RAGGED, false> + pool_seam_kernel<false> + part_reduce_kernel through
    ops.conv_pool_stats (NTERM = 1 in f16: one channel tile; 2 in the mixed modes: two; RAGGED = false at 36 x 64 only)."""
    from nerf_qa_amd import ops
    ho, wo, strips, rows = (h + 1) // 2, (w + 1) // 2, P.cdiv(w, 16), P.cdiv(h, 4)
    if batch == "single":
        b = P.pool_single_unit_batch(h, w, cus, nct)
        assert b >= 1, f"not one pair of {h} x {w} fits {cus} CUs with a unit per block"
    elif (h, w) == (P.H, P.W):
        b = P.pool_batch_for(h, w, cus, nct)
    else:
        b = P.pool_strong_batch_for(h, w, cus, nct)
        assert b is not None, f"no batch of {h} x {w} pairs reaches the fused conv2_2's stronger regime on {cus} CUs"
    r = P.pool_regime(b, h, w, cus, nct)
    print(f"\n conv2_2 + pool + statistics [{prec}] conv3x3_regw128_pool_kernel<{2 if nct == 2 else 1}, "
          f"{str(P.pool_is_ragged(h, w)).lower()}, false>: {b} pairs of {h}x{w}, {r['units']} units on {r['grid']} blocks of {cus} CUs, "
          f"{r['least']}..{r['most']} steps per block (at most {r['own']} units of its own, {r['inside']} of one pair), "
          f"{r['warm']} runs start inside a strip, {r['cross']} cross an image pair")
    if batch == "single":  # one unit per block; every run but a strip's first starts with the warm-up step
        assert r["grid"] == r["units"] <= min(cus, P.PART_BLOCKS) and r["own"] == 1 and r["most"] == 2, r
        assert r["warm"] == r["units"] - b * nct * strips and 2 * r["warm"] > r["grid"], r
    else:
        assert P.pool_in_regime(r) and r["warm"] >= 1 and r["cross"] >= 1 and r["most"] >= 4, r
        if (h, w) != (P.H, P.W):
            assert P.pool_in_strong_regime(r) and r["own"] >= 4 and r["least"] < r["most"], r
    assert 4 * r["inside"] * 63 ** 2 < 2 ** 24  # a lane's float32 moments between two flushes stay exact
    px, py, want = pool_refs(h, w)
    inp = torch.cat([P.batch_of(P.int_base(P.SPARSE_LAYER, h, w, 0), b), P.batch_of(P.int_base(P.SPARSE_LAYER, h, w, 1), b)])
    pooled, sums = _nan_filled((2 * b, ho, wo, 128), torch.float16, dev), _nan_filled((b, 128, 5), torch.float64, dev)
    res = ops.conv_pool_stats(inp.half().to(dev), P.SPARSE_LAYER, blob("sparse", prec), prec, pooled=pooled, sums=sums)
    assert res[0] is pooled and res[1] is sums
    what = f"conv2_2 + pool + statistics [{prec}] {b} pairs of {h}x{w}"
    _no_nan_left(pooled, what)
    nan = torch.isnan(sums).any(dim=2).nonzero().cpu()
    assert nan.shape[0] == 0, f"{what}: {nan.shape[0]} (pair, channel) sums were never written; first {nan[:8].tolist()}"

    def owners_of(bad):  # bad: rows of (image, pooled row, pooled column, channel); tap rows 2 y - 1 and 2 y feed pooled row y
        hit = sorted({P.pool_owner(i % b, ch // (128 // nct), min(2 * c // 16, strips - 1), min(max(t, 0) // 4, rows - 1),
                                   b, h, w, cus, nct) for i, y, c, ch in bad.tolist() for t in (2 * y - 1, 2 * y)} - {None})
        return f"(block, step) of the units behind them: first {hit[:8]}; steps hit {sorted({s for _, s in hit})}"

    def report(mask, verb):
        bad = mask.nonzero()
        ch = sorted(set(bad[:, 3].tolist()))
        return (f"{what}: {bad.shape[0]} pooled values {verb} (seam columns {int(mask[:, :, seam].sum())}, others "
                f"{int(mask[:, :, ~seam].sum())}); first (image, row, column, channel) {bad[:6].tolist()}; rows hit "
                f"{sorted(set(bad[:, 1].tolist()))}; columns hit {sorted(set(bad[:, 2].tolist()))}; channels hit {ch[:8]} .. "
                f"{ch[-1]}; " + owners_of(bad[:4096]))

    got = pooled.cpu()
    seam = torch.zeros(wo, dtype=torch.bool)
    seam[::8] = True  # pooled column 8 * sx: pool_seam_kernel's
    # image k = base image k % 3 within each half of the batch: the copies sit at other units, blocks and ring slots
    bits = got.view(torch.int16)
    copy_of = torch.cat([torch.arange(b) % 3, b + torch.arange(b) % 3]) if b >= 3 else torch.arange(2 * b)
    unlike = bits != bits[copy_of]
    print(f"   copies: {int(unlike.sum())} of {unlike.numel()} halves differ from the first three pairs'")
    assert not bool(unlike.any()), report(unlike, "of the copies differ from images 0..2")
    ref = torch.cat([P.batch_of(px, b), P.batch_of(py, b)])
    d = (got.float() - ref.float()).abs()
    ulp = ref.float().abs().clamp_min(6.1e-5) * 2.0 ** -10
    differ, over = d > 0, d > ulp
    frac = float(differ.float().mean())
    print(f"   pooled: {int(differ.sum())} of {differ.numel()} halves differ from the float64 reference ({frac:.2e}; seam columns "
          f"{int(differ[:, :, seam].sum())}, others {int(differ[:, :, ~seam].sum())}); beyond one unit in the last place: "
          f"{int(over.sum())}")
    assert not bool(over.any()), report(over, "are more than one unit in the last place from the float64 reference")
    assert frac <= 2e-2, report(differ, f"({frac:.2e} of all) differ from the float64 reference")
    ref_sums = want[torch.arange(b) % 3]
    wrong = (sums.cpu() != ref_sums)
    print(f"   sums: {int(wrong.sum())} of {wrong.numel()} differ from the exact float64 sums")
    if bool(wrong.any()):
        bad = wrong.nonzero()
        g, e = sums.cpu()[wrong][:4].tolist(), ref_sums[wrong][:4].tolist()
        runs = P.pool_runs(b, h, w, cus, nct)[0]
        per = nct * strips * rows
        blocks = {p: [k for k, (lo, hi, _) in enumerate(runs) if lo < (p + 1) * per and hi > p * per][:12]
                  for p in sorted(set(bad[:, 0].tolist()))[:4]}
        raise AssertionError(f"{what}: {bad.shape[0]} sums differ from the exact float64 sums; first (pair, channel, sum) "
                             f"{bad[:6].tolist()}: got {g}, expected {e}; pairs hit {sorted(set(bad[:, 0].tolist()))}; channels hit "
                             f"{sorted(set(bad[:, 1].tolist()))[:16]}; sums hit {sorted(set(bad[:, 2].tolist()))}; blocks whose runs "
                             f"hold units of the first pairs hit (at most 12 each): {blocks}")


# ---- stage 1 on integers: conv1_regw_kernel and the fused conv1_pool_kernel -----------------------------------------------
@pytest.fixture(scope="module")
def s1_refs():
    """refs(h, w): relu1_2 of the two base triples on the integer set, the pooled references (three x frames, three y
    frames) and the five sums of pair k = (x base k, y base k); made on first use, once for all tests."""
    made = {}

    def get(h, w):
        if (h, w) not in made:
            tx, ty = P.s1_ref(h, w, 0), P.s1_ref(h, w, 1)
            assert tx.max() <= 63 and ty.max() <= 63
            made[h, w] = (tx, P.pooled_refs(tx)[0], P.pooled_refs(ty)[0], P.five_sums(tx, ty))
        return made[h, w]
    return get


@pytest.mark.parametrize("prec", ["f16", "bf16", "f16w"])
@pytest.mark.parametrize("h,w", P.S1_SHAPES, ids=_ID)
def test_stage1_integer_frames_are_bit_exact_past_one_tile(h, w, prec, s1_refs, blob, cus, dev):
    """conv1_regw_kernel<P> (f16, bf16) and conv1_regw_kernel<PrecF16, 2> (f16w) through ops.conv1_fused."""
    from nerf_qa_amd import ops
    n = P.batch_for("conv1_regw", h, w, cus)
    r = P.regime("conv1_regw", n, h, w, cus)
    print(f"\n stage 1 on integers [{prec}] conv1_regw: {n}x{h}x{w}, {r['total']} tiles on {r['grid']} blocks of {cus} CUs, "
          f"{r['least']}..{r['most']} tiles per block, ring of {r['ring']}")
    assert P.in_regime(r) and r["most"] >= 4 and r["least"] < r["most"] and r["dummy_halo"], r
    out = _nan_filled((n, h, w, 64), DT[prec], dev)
    assert ops.conv1_fused(P.batch_of(P.s1_frames(h, w, 0), n).to(dev), blob("s1", prec), prec, out=out) is out
    what = f"stage 1 on integers [{prec}] {n}x{h}x{w}"
    _no_nan_left(out, what)
    ref = P.batch_of(P.round_to(s1_refs(h, w)[0], DT[prec]), n)
    _assert_bit_equal(out.cpu(), ref, what, "conv1_regw", n, h, w, cus, 1, 64)


S1_POOL_CASES = [(h, w, None) for h, w in P.S1_SHAPES] + [(P.S1_H, P.S1_W, 1)]  # (None: the model's batch)


@pytest.mark.parametrize("h,w,pairs", S1_POOL_CASES, ids=_ID)
def test_fused_stage1_pool_stats_on_integers_past_one_unit(h, w, pairs, s1_refs, blob, cus, dev):
    """conv1_pool_kernel<RAGGED> (RAGGED = false at 64 x 96 only) + pool_seam_kernel + part_reduce_kernel through
    ops.conv1_pool_stats."""
    from nerf_qa_amd import ops
    ho, wo, spairs, rows = (h + 1) // 2, (w + 1) // 2, P.cdiv(w, 32), P.cdiv(h, 4)
    b = P.s1_batch_for(h, w, cus) if pairs is None else pairs
    r = P.s1_regime(b, h, w, cus)
    print(f"\n fused stage 1: {b} pairs of {h}x{w}, {r['units']} units on {r['grid']} blocks of {cus} CUs, {r['least']}..{r['most']} "
          f"steps per block (at most {r['own']} units of its own, {r['inside']} of one pair), {r['warm']} runs start inside a strip, "
          f"{r['cross']} cross an image pair")
    if pairs is None:
        assert P.s1_in_regime(r) and r["warm"] >= 1 and r["cross"] >= 1 and r["most"] >= 4 and r["own"] >= 4 \
            and r["least"] < r["most"], r
    else:  # one unit per block where the device has a CU for each; most runs start with the warm-up unit
        assert r["grid"] == min(r["units"], cus, P.PART_BLOCKS_S1 // 2) and 2 * r["warm"] > r["grid"], r
        assert cus < r["units"] or (r["own"] == 1 and r["most"] == 2 and r["warm"] == r["units"] - spairs), r
    assert 4 * r["inside"] * 63 ** 2 < 2 ** 24  # a lane's float32 moments between two flushes stay exact
    _, px, py, want = s1_refs(h, w)
    x, y = (P.batch_of(P.s1_frames(h, w, s), b).to(dev) for s in (0, 1))
    pooled, sums = _nan_filled((2 * b, ho, wo, 64), torch.float16, dev), _nan_filled((b, 64, 5), torch.float64, dev)
    res = ops.conv1_pool_stats(x, y, blob("s1", "f16"), "f16", pooled=pooled, sums=sums)
    assert res[0] is pooled and res[1] is sums
    what = f"fused stage 1, {b} pairs of {h}x{w}"
    _no_nan_left(pooled, what)
    nan = torch.isnan(sums).any(dim=2).nonzero().cpu()
    assert nan.shape[0] == 0, f"{what}: {nan.shape[0]} (pair, channel) sums were never written; first {nan[:8].tolist()}"
    own = P.s1_owners(b, h, w, cus)

    def owners_of(bad):  # bad: rows of (image, pooled row, pooled column, channel); tap rows 2 y - 1 and 2 y feed pooled row y
        units = {(i % b, min(2 * c // 32, spairs - 1), min(max(t, 0) // 4, rows - 1))
                 for i, yy, c, _ in bad.tolist() for t in (2 * yy - 1, 2 * yy)}
        hit = sorted({bs for u in units for bs in own[u]})
        return f"(block, step) of the units behind them: first {hit[:8]}; steps hit {sorted({s for _, s in hit})}"

    def report(mask, verb):
        bad = mask.nonzero()
        ch = sorted(set(bad[:, 3].tolist()))
        return (f"{what}: {bad.shape[0]} pooled values {verb} (seam columns {int(mask[:, :, seam].sum())}, others "
                f"{int(mask[:, :, ~seam].sum())}); first (image, row, column, channel) {bad[:6].tolist()}; rows hit "
                f"{sorted(set(bad[:, 1].tolist()))}; columns hit {sorted(set(bad[:, 2].tolist()))}; channels hit {ch[:8]} .. "
                f"{ch[-1]}; " + owners_of(bad[:4096]))

    got = pooled.cpu()
    seam = torch.zeros(wo, dtype=torch.bool)
    seam[::8] = True  # pooled column 8 * s16: pool_seam_kernel's
    bits = got.view(torch.int16)
    copy_of = torch.cat([torch.arange(b) % 3, b + torch.arange(b) % 3]) if b >= 3 else torch.arange(2 * b)
    unlike = bits != bits[copy_of]
    print(f"   copies: {int(unlike.sum())} of {unlike.numel()} halves differ from the first three pairs'")
    assert not bool(unlike.any()), report(unlike, "of the copies differ from images 0..2")
    ref = torch.cat([P.batch_of(px, b), P.batch_of(py, b)])
    d = (got.float() - ref.float()).abs()
    ulp = ref.float().abs().clamp_min(6.1e-5) * 2.0 ** -10
    differ, over = d > 0, d > ulp
    frac = float(differ.float().mean())
    print(f"   pooled: {int(differ.sum())} of {differ.numel()} halves differ from the float64 reference ({frac:.2e}; seam columns "
          f"{int(differ[:, :, seam].sum())}, others {int(differ[:, :, ~seam].sum())}); beyond one unit in the last place: "
          f"{int(over.sum())}")
    assert not bool(over.any()), report(over, "are more than one unit in the last place from the float64 reference")
    assert frac <= 2e-2, report(differ, f"({frac:.2e} of all) differ from the float64 reference")
    ref_sums = want[torch.arange(b) % 3]
    wrong = (sums.cpu() != ref_sums)
    print(f"   sums: {int(wrong.sum())} of {wrong.numel()} differ from the exact float64 sums")
    if bool(wrong.any()):
        bad = wrong.nonzero()
        g, e = sums.cpu()[wrong][:4].tolist(), ref_sums[wrong][:4].tolist()
        runs = P.s1_runs(b, h, w, cus)[0]
        per = spairs * rows
        blocks = {p: [k for k, (lo, hi, _) in enumerate(runs) if lo < (p + 1) * per and hi > p * per][:12]
                  for p in sorted(set(bad[:, 0].tolist()))[:4]}
        raise AssertionError(f"{what}: {bad.shape[0]} sums differ from the exact float64 sums; first (pair, channel, sum) "
                             f"{bad[:6].tolist()}: got {g}, expected {e}; pairs hit {sorted(set(bad[:, 0].tolist()))}; channels hit "
                             f"{sorted(set(bad[:, 1].tolist()))[:16]}; sums hit {sorted(set(bad[:, 2].tolist()))}; blocks whose runs "
                             f"hold units of the first pairs hit (at most 12 each): {blocks}")
