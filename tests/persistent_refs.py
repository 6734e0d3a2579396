"""CPU side of tests/test_gpu_conv_persistent.py: where the persistent register-weights convolutions of nqa_conv.hip (and
the fused conv2_2 + pool + statistics kernel of nqa_conv_pool.hip) are held to exact references in the regime in which
their scheduling code runs -- a block that owns SEVERAL tiles.  No GPU needed: tests/test_persistent_refs.py checks
everything here.

(a) A schedule model: the host grid rules (launch_regw, launch_regw128 with its `grid -= 8` trimming, launch_regw_split
    with its streams, launch_conv1_regw / launch_conv1_regw_split, launch_conv_pool) and the kernels' own tile split
    (TileRun and unit_run of csrc/nqa_regw.h; conv3x3_regw_split_kernel's streams; launch_conv1_pool), restated in integer arithmetic.  It only
    chooses batch sizes, proves that a case reaches its regime and names the block and step behind a failing pixel.  It
    is never a reference for values.
(b) Exact-integer operands as in tests/test_gpu_conv_igemm_addr.py: activations in {0, 1, 2}, weights in {-1, 0, 1}, a
    bias in {-3 .. 3}; every partial sum is an integer below 2^24, exact in float32 in any order and on one- or two-term
    weights alike, so a kernel's output must be BIT-EQUAL to relu(conv2d) taken in float64 and rounded once.
(c) A sparse weight set for conv2_2 (at most 31 weights of +-1 per output channel, bias in {-1, 0, 1}): the tap is an
    integer in [0, 63], so its squares, the L2-pool's window sums and every float32 moment the fused kernel keeps per
    lane are exact integers too.
(d) The same for the fused stage 1 (csrc/nqa_conv1_pool.hip): raw pixels float32(mean_c + std_c v) that normalise to the
    integers v in {-1, 0, 1, 2} exactly in half, sparse integer conv1_1 and conv1_2 with relu1_2 in [0, 63], and the
    model of launch_conv1_pool (s1_runs .. s1_owners)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

CU_COUNTS = (8, 64, 104, 256, 304)
H, W = 37, 70                 # ragged under the 8 x 32 and the 4 x 32 tile, and under the pool kernel's 4 x 16 unit
S1_H, S1_W = 150, 130         # stage-1 frames
# the fused conv2_2's maps (a unit is 4 rows x 16 columns of an image pair) and what each reaches:
#   37 x 70: the ragged instance; H % 4 = 1, so a strip's last tile has one live row and its last tap row is masked
#   36 x 64: the RAGGED = false instance (no masking code, PF = 3 fragment sets in flight), every strip's last tile fully live
#   36 x 70: the ragged instance with a live last row in every strip (the carried row above must be dropped at the next
#            strip's top) and a last strip 6 columns wide
#   38 x 48: the ragged instance where only H is ragged (H % 4 = 2): full strips, the last pooled row completes in pass 1
POOL_SHAPES = ((37, 70), (36, 64), (36, 70), (38, 48))
INT_LAYERS = (1, 2, 3, 4)
IGEMM_INT_LAYERS = (7, 8)     # conv4_1, conv4_2: the same construction, for tests/test_gpu_conv_float_exact.py
SPARSE_LAYER = 3
SPARSE_TERMS = 31
PART_BLOCKS = 256             # NQA_FUSED_PART_BLOCKS: the fused kernel's grid never exceeds its partial rows
PART_BLOCKS_S1 = 512          # NQA_FUSED_PART_BLOCKS_S1: the fused stage 1 leaves two partial rows per block
# the fused stage 1's frames: H % 4 = 2 and W % 32 = 2 (the last unit's second half-strip wholly outside, two live columns
# in its first); H odd, six live columns; full units (the kernel's other instance); H % 4 = 0 under a ragged W (only where
# a strip's last tap row is live does the carried row above have to be zeroed at the next strip's top)
S1_SHAPES = ((150, 130), (37, 70), (64, 96), (36, 70))
S1_MEAN = (np.float32(0.485), np.float32(0.456), np.float32(0.406))   # kMean, kStd of csrc/nqa_regw.h: float32 literals
S1_STD = (np.float32(0.229), np.float32(0.224), np.float32(0.225))
S1_LEVELS = (-1, 0, 1, 2)     # the normalised pixel values of the integer frames
S1_TERMS = (6, 12)            # nonzero weights per output channel of the sparse conv1_1, conv1_2

# tile height, slots of the LDS-DMA ring, grid rule -- by the name of the launcher's kernel
KERNELS = {
    "regw": dict(th=8, ring=3, rule="xcd"),               # conv3x3_regw_kernel<., NCG, NTERM>
    "regw128": dict(th=4, ring=2, rule="xcd_trim"),       # conv3x3_regw128_kernel (tiles = pixel tiles x channel tiles)
    "regw_split": dict(th=4, ring=2, rule="streams"),     # conv3x3_regw_split_kernel (units = tiles x 64-channel halves)
    "conv1_regw": dict(th=8, ring=2, rule="xcd"),         # conv1_regw_kernel<., NTERM>
    "conv1_regw_split": dict(th=4, ring=2, rule="xcd"),   # conv1_regw_split_kernel
}


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


# ---- (a) the schedule model --------------------------------------------------------------------------------------------
def grid_for(kernel: str, total: int, cus: int, nct: int = 1) -> int:
    """Blocks the launcher starts for `total` tiles (regw128: pixel tiles x nct channel tiles; regw_split: pixel tiles,
    nct = the layer's 64-channel halves)."""
    rule = KERNELS[kernel]["rule"]
    if rule == "streams":
        streams = max(1, min(cus // (8 * nct), cdiv(total, 8)))
        return 8 * nct * streams
    grid = min(total, cus)
    if rule == "xcd_trim":
        while nct > 1 and grid > 8 * nct and ((grid + 7) // 8) % nct:
            grid -= 8
    return grid


def block_walks(kernel: str, total: int, cus: int, nct: int = 1):
    """(first, stride, count) per block, int64 arrays over the grid: block b owns first[b] + i * stride[b] for i <
    count[b].  regw_split: the ids are units tile * nct + half, so that every unit has one owner."""
    nblk = grid_for(kernel, total, cus, nct)
    b = np.arange(nblk, dtype=np.int64)
    if KERNELS[kernel]["rule"] == "streams":
        xcd, jb = b & 7, b >> 3
        half, stream, streams = jb % nct, jb // nct, (nblk >> 3) // nct
        t_lo, t_hi = total * xcd // 8, total * (xcd + 1) // 8
        count = np.where(t_lo + stream < t_hi, (t_hi - t_lo - stream - 1) // streams + 1, 0)
        return (t_lo + stream) * nct + half, np.full(nblk, streams * nct, dtype=np.int64), count
    nx = min(nblk, 8)
    xcd, jb = b % nx, b // nx
    per = (nblk - xcd + nx - 1) // nx
    t_lo, t_hi = total * xcd // nx, total * (xcd + 1) // nx
    count = np.where(t_lo + jb < t_hi, (t_hi - t_lo - jb - 1) // per + 1, 0)
    return t_lo + jb, per, count


def block_tiles(kernel: str, total: int, cus: int, nct: int = 1):
    """The tile list of every block, in the order of its walk."""
    first, stride, count = block_walks(kernel, total, cus, nct)
    return [[int(f + i * s) for i in range(int(c))] for f, s, c in zip(first, stride, count)]


def flat_tiles(kernel: str, total: int, cus: int, nct: int = 1) -> np.ndarray:
    """Every tile any block is given, concatenated (for the partition property)."""
    first, stride, count = block_walks(kernel, total, cus, nct)
    step = np.arange(int(count.sum()), dtype=np.int64) - np.repeat(np.cumsum(count) - count, count)
    return np.repeat(first, count) + step * np.repeat(stride, count)


def total_tiles(kernel: str, n: int, h: int, w: int, nct: int = 1) -> int:
    """The launcher's `total` (regw_split: pixel tiles; its halves are the model's business)."""
    px = n * cdiv(w, 32) * cdiv(h, KERNELS[kernel]["th"])
    return px * nct if kernel == "regw128" else px


def regime(kernel: str, n: int, h: int, w: int, cus: int, nct: int = 1) -> dict:
    """What the model says of one launch: grid, the largest and the smallest number of tiles a block owns."""
    total = total_tiles(kernel, n, h, w, nct)
    count = block_walks(kernel, total, cus, nct)[2]
    return dict(kernel=kernel, n=n, total=total, grid=int(count.size), most=int(count.max()), least=int(count.min()),
                ring=KERNELS[kernel]["ring"], dummy_halo=bool(count.max() >= 1))


def in_regime(r: dict) -> bool:
    """Some block owns at least 4 tiles (every slot of a two- or three-slot ring is reused, the counted wait behind a
    previous tile's stores runs), some block owns fewer than another (an uneven tail), and the dummy issue_halo past a
    block's last tile runs (true of every block with a tile)."""
    return r["most"] >= 4 and r["least"] < r["most"] and r["dummy_halo"]


def batch_for(kernel: str, h: int, w: int, cus: int, nct: int = 1) -> int:
    """The smallest batch that is a multiple of 3 (image k repeats base image k % 3) and in_regime."""
    for n in range(3, 130, 3):
        if in_regime(regime(kernel, n, h, w, cus, nct)):
            return n
    raise AssertionError(f"{kernel}: no batch of {h} x {w} images reaches the persistent regime on {cus} CUs")


def owners(kernel: str, total: int, cus: int, nct: int = 1) -> dict:
    """{tile: (block, step of its walk)}."""
    return {t: (b, i) for b, ts in enumerate(block_tiles(kernel, total, cus, nct)) for i, t in enumerate(ts)}


def tile_of(kernel: str, img, row, col, ch, h: int, w: int, nct: int = 1, bc: int = 128):
    """The model's tile id of output element (img, row, col, channel); bc = output channels per block."""
    tx, ty = cdiv(w, 32), cdiv(h, KERNELS[kernel]["th"])
    px = (img * ty + row // KERNELS[kernel]["th"]) * tx + col // 32
    if kernel in ("regw128", "regw_split"):
        return px * nct + ch // bc
    return px


def reloads(total: int, cus: int, nct: int, tiles: int = 2):
    """Blocks of conv3x3_regw128_kernel that own at least `tiles` tiles and whose consecutive tiles differ in their
    channel tile (tile % nct): the load_weights + vmcnt(0) path inside the tile loop."""
    first, stride, count = block_walks("regw128", total, cus, nct)
    return [int(b) for b in np.nonzero((count >= tiles) & (stride % nct != 0))[0]]


def reload_case(cus: int, nct: int = 2):
    """The smallest (n, H, W) of conv3_1 (layer 4) in which some block reloads its weights; by pixel count, then shape.
    (Longer walks that reload exist on odd CU counts only: a grid of all the CUs is never trimmed to an odd class, and a
    smaller grid is about one block per tile.)"""
    shapes = sorted((n * h * w, n, h, w) for n in (1, 2, 3) for h in range(4, 41, 4) for w in range(20, 321, 20))
    for _, n, h, w in shapes:
        if reloads(total_tiles("regw128", n, h, w, nct), cus, nct):
            return n, h, w
    raise AssertionError(f"no small conv3_1 map makes a block reload its weights on {cus} CUs with {nct} channel tiles")


def unit_runs(units: int, nblk: int, rows: int):
    """unit_run of csrc/nqa_regw.h for a grid of nblk blocks: per block (u_lo, u_hi, warm-up step) of its contiguous run
    of units; a run that starts inside a strip of `rows` units begins with one warm-up unit (the tile above it)."""
    qq, rr = nblk >> 3, nblk & 7
    runs = []
    for blk in range(nblk):
        xcd, local = blk & 7, blk >> 3
        run = blk if nblk < 8 else (xcd * (qq + 1) if xcd < rr else rr * (qq + 1) + (xcd - rr) * qq) + local
        u_lo, u_hi = units * run // nblk, units * (run + 1) // nblk
        runs.append((u_lo, u_hi, u_lo < u_hi and u_lo % rows != 0))
    return runs


def runs_regime(runs, per_pair: int) -> dict:
    """What pool_in_regime and s1_in_regime ask of a list of runs; per_pair = units of one image pair.  `own`: the most
    units a run holds, `most` / `least`: steps (with the warm-up), `inside`: the most units of ONE pair any run holds (what a lane's moments are summed over between two flushes)."""
    def inside(lo, hi):
        return max((min(hi, (p + 1) * per_pair) - max(lo, p * per_pair) for p in range(lo // per_pair, (hi - 1) // per_pair + 1)),
                   default=0)
    return dict(grid=len(runs), own=max(hi - lo for lo, hi, _ in runs), most=max(hi - lo + warm for lo, hi, warm in runs),
                least=min(hi - lo + warm for lo, hi, warm in runs), warm=sum(1 for lo, hi, warm in runs if warm),
                cross=sum(1 for lo, hi, _ in runs if lo < hi and lo // per_pair != (hi - 1) // per_pair),
                inside=max(inside(lo, hi) for lo, hi, _ in runs))


def pool_runs(b_pairs: int, h: int, w: int, cus: int, nct: int):
    """launch_conv_pool and conv3x3_regw128_pool_kernel: per block (u_lo, u_hi, warm-up step) of its contiguous run of
    units in [pair][channel tile][strip][row] order, and (strips, rows)."""
    strips, rows = cdiv(w, 16), cdiv(h, 4)
    units = b_pairs * nct * strips * rows
    return unit_runs(units, min(units, cus, PART_BLOCKS), rows), strips, rows


def pool_regime(b_pairs: int, h: int, w: int, cus: int, nct: int) -> dict:
    runs, strips, rows = pool_runs(b_pairs, h, w, cus, nct)
    per_pair = nct * strips * rows
    return dict(kernel="regw128_pool", pairs=b_pairs, units=b_pairs * per_pair, **runs_regime(runs, per_pair))


def pool_in_regime(r: dict) -> bool:
    """Some block's run starts inside a strip (the warm-up step), some block's run crosses an image pair (the statistics
    flush inside the loop), and some run is at least 4 steps long (both slots of the ring are reused)."""
    return r["warm"] >= 1 and r["cross"] >= 1 and r["most"] >= 4


def pool_batch_for(h: int, w: int, cus: int, nct: int) -> int:
    """The smallest number of pairs that is a multiple of 3 and pool_in_regime."""
    for b in range(3, 600, 3):
        if pool_in_regime(pool_regime(b, h, w, cus, nct)):
            return b
    raise AssertionError(f"no batch of {h} x {w} pairs reaches the fused kernel's regime on {cus} CUs")


def pool_is_ragged(h: int, w: int) -> bool:
    """conv_pool_stats_fused's choice of instance: RAGGED = H % 4 or W % 16."""
    return bool(h % 4 or w % 16)


def pool_in_strong_regime(r: dict) -> bool:
    """What s1_in_regime asks of the fused stage 1, of the fused conv2_2: pool_in_regime (a warm-up step, a statistics
    flush inside the loop, a run of at least 4 steps) with at least 4 units of the run's own (both ring slots reused by
    units whose outputs count, the counted vmcnt(2 * NST) behind two pooled rows' stores) and uneven runs."""
    return pool_in_regime(r) and r["own"] >= 4 and r["least"] < r["most"]


def pool_strong_batch_for(h: int, w: int, cus: int, nct: int):
    """The smallest number of pairs b >= 3 (any such b keeps the k % 3 copy map) in pool_in_strong_regime, or None where
    no batch of up to 600 pairs is (few CUs under full tiles: every batch is dealt evenly)."""
    for b in range(3, 601):
        if pool_in_strong_regime(pool_regime(b, h, w, cus, nct)):
            return b
    return None


def pool_single_unit_batch(h: int, w: int, cus: int, nct: int) -> int:
    """The largest number of pairs whose units number at most min(cus, PART_BLOCKS): every block owns one unit, and a run
    that starts inside a strip is a warm-up step, the wait vmcnt(NST) behind it, one unit and the drain.  0: not even one
    pair fits."""
    return min(cus, PART_BLOCKS) // (nct * cdiv(w, 16) * cdiv(h, 4))


def pool_owner(img_pair: int, ct: int, sx: int, ty: int, b_pairs: int, h: int, w: int, cus: int, nct: int):
    """(block, step) of the fused kernel's unit (pair, channel tile, strip, tile row)."""
    runs, strips, rows = pool_runs(b_pairs, h, w, cus, nct)
    u = ((img_pair * nct + ct) * strips + sx) * rows + ty
    for blk, (lo, hi, warm) in enumerate(runs):
        if lo <= u < hi:
            return blk, u - lo + warm
    return None


def s1_runs(b_pairs: int, h: int, w: int, cus: int):
    """launch_conv1_pool and conv1_pool_kernel: per block (u_lo, u_hi, warm-up step) of its contiguous run of units of
    4 rows x 32 columns in [pair][strip pair][row] order, and (strip pairs, rows).  Two partial rows per block."""
    spairs, rows = cdiv(w, 32), cdiv(h, 4)
    units = b_pairs * spairs * rows
    return unit_runs(units, min(units, cus, PART_BLOCKS_S1 // 2), rows), spairs, rows


def s1_regime(b_pairs: int, h: int, w: int, cus: int) -> dict:
    runs, spairs, rows = s1_runs(b_pairs, h, w, cus)
    return dict(kernel="conv1_pool", pairs=b_pairs, units=b_pairs * spairs * rows, **runs_regime(runs, spairs * rows))


def s1_in_regime(r: dict) -> bool:
    """pool_in_regime (a warm-up step, a statistics flush inside the loop, a run of at least 4 steps) with at least 4
    units of the run's own (both halo slots, both raw patches and both exchange buffers are reused by units whose
    outputs count, the counted vmcnt(2 * NST) runs behind two pooled rows' stores) and uneven runs."""
    return pool_in_regime(r) and r["own"] >= 4 and r["least"] < r["most"]


def s1_batch_for(h: int, w: int, cus: int) -> int:
    """The smallest number of pairs that is a multiple of 3 and s1_in_regime."""
    for b in range(3, 600, 3):
        if s1_in_regime(s1_regime(b, h, w, cus)):
            return b
    raise AssertionError(f"no batch of {h} x {w} pairs reaches the fused stage 1's regime on {cus} CUs")


def s1_owners(b_pairs: int, h: int, w: int, cus: int) -> dict:
    """{(pair, strip pair, row): [(block, step), ...]} of the fused stage 1's units (the model of a correct launch gives
    every unit one owner; a run's warm-up unit is not owned by it)."""
    runs, spairs, rows = s1_runs(b_pairs, h, w, cus)
    own = {}
    for blk, (lo, hi, warm) in enumerate(runs):
        for u in range(lo, hi):
            own.setdefault((u // (spairs * rows), u // rows % spairs, u % rows), []).append((blk, u - lo + warm))
    return own


# ---- (b), (c) integer operands --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def int_convs():
    """The synthetic VGG weights with layers 1..4 (and conv4_1, conv4_2) in {-1, 0, 1} and a bias in {-3 .. 3}."""
    from nerf_qa_amd import ops, synth
    convs = list(synth.vgg16_weights(1234))
    for layer in INT_LAYERS + IGEMM_INT_LAYERS:
        cout, cin = ops.CONV_COUT[layer], ops.CONV_CIN[layer]
        w = np.floor(synth.uniform(900 + layer, cout * cin * 9) * 3.0).clip(0, 2).astype(np.float32) - 1.0
        b = np.floor(synth.uniform(950 + layer, cout) * 7.0).clip(0, 6).astype(np.float32) - 3.0
        convs[layer] = (w.reshape(cout, cin, 3, 3), b)
    return convs


@functools.lru_cache(maxsize=None)
def sparse_convs():
    """int_convs with conv2_2 (layer 3) replaced: SPARSE_TERMS weights of +-1 per output channel, bias in {-1, 0, 1}.
    With activations in {0, 1, 2} the tap lies in [0, 2 * 31 + 1] = [0, 63]."""
    from nerf_qa_amd import ops, synth
    convs = list(int_convs())
    cout, k = ops.CONV_COUT[SPARSE_LAYER], ops.CONV_CIN[SPARSE_LAYER] * 9
    u = synth.uniform(1900, cout * k).reshape(cout, k)
    sign = np.where(synth.uniform(1901, cout * k).reshape(cout, k) < 0.5, -1.0, 1.0)
    w = np.zeros((cout, k), dtype=np.float32)
    pick = np.argsort(u, axis=1)[:, :SPARSE_TERMS]  # the positions of the 31 smallest draws of each row
    np.put_along_axis(w, pick, np.take_along_axis(sign, pick, axis=1).astype(np.float32), axis=1)
    b = np.floor(synth.uniform(1902, cout) * 3.0).clip(0, 2).astype(np.float32) - 1.0
    convs[SPARSE_LAYER] = (w.reshape(cout, ops.CONV_CIN[SPARSE_LAYER], 3, 3), b)
    return convs


@functools.lru_cache(maxsize=None)
def int_base(layer: int, h: int, w: int, seed: int = 0) -> torch.Tensor:
    """Three base images with activations in {0, 1, 2}: float32 NHWC (3, h, w, Cin of `layer`).  Never modified."""
    from nerf_qa_amd import ops, synth
    cin = ops.CONV_CIN[layer]
    a = np.floor(synth.uniform(700 + layer + 7 * h + w + 1000 * seed, 3 * h * w * cin) * 3.0).clip(0, 2)
    return torch.from_numpy(a.astype(np.float32).reshape(3, h, w, cin))


def batch_of(base: torch.Tensor, n: int) -> torch.Tensor:
    """Image k = base image k % 3."""
    return base[torch.arange(n) % base.shape[0]].contiguous()


@functools.lru_cache(maxsize=None)
def conv_ref(layer: int, h: int, w: int, sparse: bool = False, seed: int = 0) -> torch.Tensor:
    """relu(conv2d) of the three base images in float64, NHWC (3, h, w, Cout): integers, asserted below 2^24 together
    with a bound on every PARTIAL sum (sum |a||w| + |b|).  Round once to the storage type with round_to."""
    wq, b = (torch.from_numpy(t).double() for t in (sparse_convs() if sparse else int_convs())[layer])
    a = int_base(layer, h, w, seed).double().permute(0, 3, 1, 2)
    pre = F.conv2d(a, wq, b, padding=1)
    mag = F.conv2d(a, wq.abs(), b.abs(), padding=1)
    assert mag.max().item() < 2 ** 24 and bool((pre == pre.round()).all())
    return F.relu(pre).permute(0, 2, 3, 1).contiguous()


def partial_sum_bound(layer: int, h: int, w: int, sparse: bool = False, seed: int = 0) -> float:
    """max over the outputs of sum |a||w| + |b|: no partial sum of the convolution, in any order, exceeds it."""
    wq, b = (torch.from_numpy(t).double() for t in (sparse_convs() if sparse else int_convs())[layer])
    a = int_base(layer, h, w, seed).double().permute(0, 3, 1, 2)
    return float(F.conv2d(a, wq.abs(), b.abs(), padding=1).max())


def round_to(ref64: torch.Tensor, dtype) -> torch.Tensor:
    """One rounding of float64 INTEGERS below 2^24 to the storage type (they are exact in float32, so a conversion that
    passes through float32 still rounds once)."""
    return ref64.to(torch.float32).to(dtype)


# ---- the fused conv2_2 + L2-pool + statistics ------------------------------------------------------------------------------
def pool_window_sums(tap64_nhwc: torch.Tensor) -> torch.Tensor:
    """S = the (1,2,1) x (1,2,1) window sum of the squares, stride 2, zero pad 1: exact integers in float64."""
    k = torch.tensor([1.0, 2.0, 1.0], dtype=torch.float64)
    sq = (tap64_nhwc * tap64_nhwc).permute(0, 3, 1, 2)
    c = sq.shape[1]
    s = F.conv2d(sq, (k[:, None] * k[None, :]).expand(c, 1, 3, 3).contiguous(), None, stride=2, padding=1, groups=c)
    return s.permute(0, 2, 3, 1).contiguous()


def pooled_refs(tap64_nhwc: torch.Tensor):
    """(float64 reference, float32 replay) of the pooled map sqrt(S / 16 + 1e-12), each rounded to half, NHWC."""
    s = pool_window_sums(tap64_nhwc).numpy()
    assert s.max() < 2 ** 24
    p64 = np.sqrt(s / 16.0 + 1e-12).astype(np.float16)
    s32 = s.astype(np.float32)
    p32 = np.sqrt(s32 * np.float32(0.0625) + np.float32(1e-12), dtype=np.float32).astype(np.float16)
    return torch.from_numpy(p64), torch.from_numpy(p32)


def leaked_window_sums(tap64_nhwc: torch.Tensor) -> torch.Tensor:
    """pool_window_sums as a fused conv2_2 whose carried row is NOT dropped at a strip change would form it (c_keep stuck
    at 1, one block walking an image's strips in run order): the squares of the last tap row of a strip's last tile (row
    4 * ceil(H / 4) - 1; outside the image, i.e. zero, unless H % 4 = 0) at columns [16 s, 16 s + 16) stand as row -1 above
    columns [16 (s + 1), 16 (s + 2)) of the same image.  A model of a WRONG kernel, used only to show on the references
    which shapes can tell it from the right one; never compared with a kernel's output."""
    n, h, w, c = tap64_nhwc.shape
    sq = (tap64_nhwc * tap64_nhwc).permute(0, 3, 1, 2)
    above = torch.zeros(n, c, 1, w, dtype=torch.float64)
    last = 4 * cdiv(h, 4) - 1
    if last < h:
        above[:, :, 0, 16:] = sq[:, :, last, : w - 16]
    k = torch.tensor([1.0, 2.0, 1.0], dtype=torch.float64)
    ext = F.pad(torch.cat([above, sq], dim=2), (1, 1, 0, 1))  # row -1 in place of the top padding; zero right, left, below
    s = F.conv2d(ext, (k[:, None] * k[None, :]).expand(c, 1, 3, 3).contiguous(), None, stride=2, groups=c)
    return s.permute(0, 2, 3, 1).contiguous()


def five_sums(tap_x64: torch.Tensor, tap_y64: torch.Tensor) -> torch.Tensor:
    """(B, C, 5) float64: sum x, sum y, sum x^2, sum y^2, sum xy over the pixels of the half-rounded taps (NHWC)."""
    x, y = tap_x64.half().double(), tap_y64.half().double()
    return torch.stack([x.sum((1, 2)), y.sum((1, 2)), (x * x).sum((1, 2)), (y * y).sum((1, 2)), (x * y).sum((1, 2))], -1)


# ---- the fused stage 1 (csrc/nqa_conv1_pool.hip) on integers -------------------------------------------------------------
# A raw pixel float32(mean_c + std_c v), v in S1_LEVELS, normalises to a float32 within 5e-7 of v by either form the
# kernels use, i.e. to exactly v in half (and bfloat16); v = 0 is float32(mean_c) itself and gives exactly 0, as the zero
# padding does.  With sparse integer conv1_1 and conv1_2, relu1_1 and relu1_2 (in [0, 63] on these frames) are integers,
# and so is everything the fused kernel makes of them, as for the fused conv2_2 above.
def s1_pixel(c: int, v: int) -> np.float32:
    """The raw pixel of channel c that normalises to the integer v."""
    return S1_MEAN[c] if v == 0 else np.float32(np.float64(S1_MEAN[c]) + np.float64(S1_STD[c]) * v)


def _fma32(a, b, c) -> np.float32:
    """fmaf through float64: the product of two float32 is exact there, the sum is rounded twice (the callers' margin)."""
    return np.float32(np.float64(a) * np.float64(b) + np.float64(c))


def s1_normalise(x: np.float32, c: int, form: str) -> np.float32:
    """(x - mean) / std in float32 as conv1_pool_kernel ("fused": a multiplication by 1 / std with one residual
    correction) or conv1_regw_kernel ("div") computes it."""
    mean, std = S1_MEAN[c], S1_STD[c]
    d = np.float32(x - mean)
    if form == "div":
        return np.float32(d / std)
    isd = np.float32(np.float32(1.0) / std)
    q0 = np.float32(d * isd)
    return _fma32(_fma32(-q0, std, d), isd, q0)


def _sparse_rows(seed: int, cout: int, k: int, terms: int, cover: int) -> np.ndarray:
    """(cout, k) weights, `terms` of +-1 in each row: row o takes `cover` consecutive entries of a permutation of the k
    positions, from entry o * cover on (cout * cover >= k: every position is used by some row), then its smallest draws."""
    from nerf_qa_amd import synth
    assert cout * cover >= k and cover <= terms
    u = synth.uniform(seed, cout * k).reshape(cout, k)
    perm = np.argsort(synth.uniform(seed + 1, k))
    for o in range(cout):
        u[o, perm[(o * cover + np.arange(cover)) % k]] = -1.0
    sign = np.where(synth.uniform(seed + 2, cout * k).reshape(cout, k) < 0.5, -1.0, 1.0)
    w = np.zeros((cout, k), dtype=np.float32)
    pick = np.argsort(u, axis=1)[:, :terms]
    np.put_along_axis(w, pick, np.take_along_axis(sign, pick, axis=1).astype(np.float32), axis=1)
    return w


@functools.lru_cache(maxsize=None)
def s1_convs():
    """int_convs with conv1_1 and conv1_2 (layers 0, 1) replaced by sparse integer layers: S1_TERMS weights of +-1 per
    output channel; conv1_1's bias in {-1 .. 2} (a halo pixel outside the image that is left at relu(bias) instead of
    zero shows), conv1_2's in {-1, 0, 1}; every (input channel, tap) position of either layer is used by some output."""
    from nerf_qa_amd import synth
    convs = list(int_convs())
    w0 = _sparse_rows(2900, 64, 27, S1_TERMS[0], 1).reshape(64, 3, 3, 3)
    b0 = np.floor(synth.uniform(2903, 64) * 4.0).clip(0, 3).astype(np.float32) - 1.0
    w1 = _sparse_rows(2910, 64, 576, S1_TERMS[1], 9).reshape(64, 64, 3, 3)
    b1 = np.floor(synth.uniform(2913, 64) * 3.0).clip(0, 2).astype(np.float32) - 1.0
    convs[0], convs[1] = (w0, b0), (w1, b1)
    return convs


@functools.lru_cache(maxsize=None)
def s1_levels(h: int, w: int, seed: int = 0) -> torch.Tensor:
    """Three base frames as their integer levels: float64 NCHW (3, 3, h, w) in S1_LEVELS.  Never modified."""
    from nerf_qa_amd import synth
    v = np.floor(synth.uniform(4100 + 7 * h + w + 1000 * seed, 9 * h * w) * len(S1_LEVELS)).clip(0, len(S1_LEVELS) - 1)
    return torch.from_numpy(v.reshape(3, 3, h, w) + float(S1_LEVELS[0]))


@functools.lru_cache(maxsize=None)
def s1_frames(h: int, w: int, seed: int = 0) -> torch.Tensor:
    """The raw frames of s1_levels: float32 NCHW (3, 3, h, w), pixels in [0, 1].  Never modified."""
    lv = s1_levels(h, w, seed).numpy().astype(np.int64) - S1_LEVELS[0]
    table = np.array([[s1_pixel(c, v) for v in S1_LEVELS] for c in range(3)], dtype=np.float32)
    out = np.stack([table[c][lv[:, c]] for c in range(3)], axis=1)
    assert out.dtype == np.float32 and 0.0 <= out.min() and out.max() <= 1.0
    return torch.from_numpy(out)


@functools.lru_cache(maxsize=None)
def s1_ref(h: int, w: int, seed: int = 0) -> torch.Tensor:
    """relu1_2 of the three base frames in float64 from their integer levels, NHWC (3, h, w, 64): integers in [0, 63],
    asserted together with the integrality of relu1_1 and a bound below 2^24 on every partial sum of either layer."""
    (w0, b0), (w1, b1) = (tuple(torch.from_numpy(t).double() for t in wb) for wb in s1_convs()[:2])
    a = s1_levels(h, w, seed)
    r11 = F.relu(F.conv2d(a, w0, b0, padding=1))
    r12 = F.relu(F.conv2d(r11, w1, b1, padding=1))
    for inp, wq, b in ((a, w0, b0), (r11, w1, b1)):
        assert F.conv2d(inp.abs(), wq.abs(), b.abs(), padding=1).max().item() < 2 ** 24
    assert bool((r11 == r11.round()).all()) and bool((r12 == r12.round()).all())
    assert r11.max().item() <= 2048 and r12.max().item() <= 63, (r11.max().item(), r12.max().item())
    return r12.permute(0, 2, 3, 1).contiguous()
