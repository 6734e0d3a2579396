"""The group statistics kernels (nqa_group_stats.hip: group_stats_nhwc_kernel in float, f16 and bf16; group_stats_nchw_kernel)
held to EXACT sums and float-ulp S1 / S2, through ops.dists_group_sums / ops.dists_group_stats (include/nqa.h:
nqa_dists_group_sums, nqa_dists_group_stats), and the pair path's plane kernel (stats_nchw_kernel) through
ops.dists_stats_nchw, against the float64 references of tests/group_refs.py.  Every call writes into 0xFF-filled sums,
s1, s2 and scratch, and the outputs are searched for NaN first: a partial that no block wrote leaves its NaN behind.

(a) BIT-EQUAL SUMS.  On group_refs.group_exact_maps (multiples of 1/4 in [0, 4], 40 % zeros; a channel dead everywhere,
    one dead in the references, one dead in render 0 of each group; render K - 1 identical to its reference) nothing
    the kernels compute for the five sums rounds (the argument is in group_refs.py), so ops.dists_group_sums must be
    torch.equal to group_sums_ref: no tolerance.  tests/test_group_refs.py shows on the reference alone that a dropped
    last pixel, a strip item counted twice, a render read from the neighbouring group, two renders' rows exchanged and
    a reference strip that belongs to the block before all fail this check.  "f32s" must alias "f32" bit for bit.
(b) S1 / S2 OF THE PRODUCTION ENTRY on the same inputs: ops.dists_group_stats against pool_refs.s_from_sums of the
    float64 sums, |got - ref| <= 2^-23 |ref| + 2^-40 -- the float rounding of an fp64 result and nothing else
    (test_group_refs.py: a float64 replay of finalize_kernel's order sits at 0.50 of it, a dropped pixel far outside).
    Rows of the identical render must be exactly 1.0 in S1 and S2, and their sum x^2, sum y^2 and sum xy equal in bits.
(c) EXACT PROPERTIES of the sums: two launches are bit-equal; permuting a group's renders permutes the rows; a group's
    rows do not depend on the other groups while the grid query reports the same pixels per block.
(d) THE PAIR PATH'S PLANE KERNEL: ops.dists_stats_nchw on six exact NCHW maps (C = 3, 64, 128, 256, 512, 512) of 1 x 1,
    of 5 x 7, and with the C = 3 map at 17 x 241 = 4097 pixels (two blocks, one pixel in the second), three pairs with
    y = x in pair 1 and the dead channels in place: S1 / S2 to the criterion of (b), the y = x rows exactly 1.0.

Shapes (R, K, HW, C) of the NHWC kernel, the smallest that reach each regime; every regime is asserted from
nqa_dists_group_stats_grid and the plan (pixels per block, blocks per map, pixels side by side, items) is printed:
  - HW < PL, threads that hold nothing: (1, 1, 1, 64);
  - 4 items per thread, a ragged last block: HW = 35 (C = 64), 299 (C = 128), 77 (C = 512), in the three storage types;
  - many blocks per map with R = 3, where blockIdx.x has to split into (r, blk): (3, 2, 1551, 256);
  - 5 to 15 items: (1, 2, 6007, 512) in float; 16 items with a ragged last block whose threads hold different counts:
    (1, 2, 24589, 512) in float and f16;
  - 16 items at C = 64 in each storage type, where the planner reaches them from HW * R >= 262144 (float) / 524288
    (16-bit): K = 1, HW = 262144 + 37 / 524288 + 37 (134 MB of maps; the float64 reference is taken on the device);
  - K = 1 at R = 2: (2, 1, 77, 128); odd K >= 7 at a small map: (2, 7, 35, 64), (1, 9, 77, 256).
The plane kernel: (R, K, C) = (2, 3, 3) at HW = 1, 35 (one ragged block), 4096 (one full block: 16 items in every
thread), 4097 and 8193 (one pixel in the last block; R * C = 6 planes, each with blk > 0).

Measured on an MI355X: every S1 / S2 at 0.50 of the criterion or less (the plane kernels 0.48); the 45 cases of this file
take 3.1 s of wall time together, 0.7 s of it the first launch.
"""
import pytest
import torch

import group_refs as G
import pool_refs as P

pytestmark = pytest.mark.gpu

DTYPE = {"f32": torch.float32, "f32s": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
NHWC_STORAGE = ("f32", "f16", "bf16")
SMALL = [(1, 1, 1, 64), (2, 3, 35, 64), (1, 5, 299, 128), (3, 2, 1551, 256), (2, 4, 77, 512), (2, 1, 77, 128), (2, 7, 35, 64),
         (1, 9, 77, 256)]
MID = [("f32", 1, 2, 6007, 512)]
UNEVEN16 = [("f32", 1, 2, 24589, 512), ("f16", 1, 2, 24589, 512)]
LONG64 = [("f32", 1, 1, 262144 + 37, 64), ("f16", 1, 1, 524288 + 37, 64), ("bf16", 1, 1, 524288 + 37, 64)]
CASES = [(p,) + s for p in NHWC_STORAGE for s in SMALL] + MID + UNEVEN16 + LONG64
PLANE_HW = (1, 35, 4096, 4097, 8193)
PLANE_RKC = (2, 3, 3)


def _id(case):
    return "%s_R%dK%d_hw%d_c%d" % case


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _ff(shape, dtype, dev):
    """A tensor whose every byte is 0xFF: NaN as float and as float64."""
    t = torch.empty(shape, dtype=dtype, device=dev)
    t.view(torch.uint8).fill_(0xFF)
    return t


def _sums(feat, R, K, prec, dev, nchw=False):
    """ops.dists_group_sums into 0xFF-filled sums (its scratch is 0xFF-filled by the wrapper), searched for NaN."""
    from nerf_qa_amd import ops
    c = feat.shape[1] if nchw else feat.shape[2]
    sums = _ff((R * K, c, 5), torch.float64, dev)
    assert torch.isnan(sums).all()
    s = ops.dists_group_sums(feat, R, K, prec, nchw=nchw, sums=sums)
    assert s.data_ptr() == sums.data_ptr() and s.shape == (R * K, c, 5) and s.dtype == torch.float64
    assert not torch.isnan(s).any(), "a partial sum was never written"
    return s


def _s(feat, R, K, prec, dev, nchw=False):
    """ops.dists_group_stats into 0xFF-filled s1, s2 and scratch, searched for NaN."""
    from nerf_qa_amd import _lib, ops
    c, hw = (feat.shape[1], feat.shape[2]) if nchw else (feat.shape[2], feat.shape[1])
    s1, s2 = _ff((R * K, c), torch.float32, dev), _ff((R * K, c), torch.float32, dev)
    nbytes = _lib.lib().nqa_dists_group_stats_bytes(R, K, hw, c, ops.prec_id(prec), int(nchw))
    assert nbytes > 0
    scratch = _ff((nbytes,), torch.uint8, dev)
    t1, t2 = ops.dists_group_stats(feat, R, K, prec, nchw=nchw, s1=s1, s2=s2, scratch=scratch)
    assert t1.data_ptr() == s1.data_ptr() and t2.data_ptr() == s2.data_ptr()
    assert not torch.isnan(s1).any() and not torch.isnan(s2).any(), "an S1 / S2 entry was never written, or read an unwritten partial"
    return s1, s2


def _grid(prec, R, K, hw, c, nchw=False):
    from nerf_qa_amd import ops
    return ops.dists_group_stats_grid(R, K, hw, c, prec, nchw=nchw)


def test_the_shapes_reach_the_regimes_they_are_chosen_for():
    """From nqa_dists_group_stats_grid, for the cases of this file (no launch)."""
    print("\npixels per block / blocks per map / pixels side by side / most items of a thread, of every case:")
    plans = {}
    for case in CASES:
        plans[case] = g = _grid(*case)
        print(f"  {_id(case)}: {g}")
        prec, R, K, hw, c = case
        ppb, nblk, pl, items = g
        assert pl == P.pl_of(c, prec) and ppb % pl == 0 and items == -(-min(ppb, hw) // pl), (case, g)
        assert nblk == -(-hw // ppb) and 1 <= items <= 16, (case, g)
    last = lambda case: case[3] - (plans[case][1] - 1) * plans[case][0]  # pixels of the last block
    for p in NHWC_STORAGE:
        assert plans[(p, 1, 1, 1, 64)][2] > 1 and plans[(p, 1, 1, 1, 64)][3] == 1  # HW = 1 < PL: most threads hold nothing
        for s in SMALL[1:]:
            ppb, nblk, pl, items = plans[(p,) + s]
            assert ppb == 4 * pl, (p, s)  # 4 items per thread ...
            assert last((p,) + s) < ppb, (p, s)  # ... and a ragged last block
        assert plans[(p, 3, 2, 1551, 256)][1] >= 24  # many blocks per map, three maps: blockIdx.x = r * nblk + blk
        assert any(plans[(p,) + s][1] == 1 for s in SMALL) and any(last((p,) + s) % plans[(p,) + s][2] for s in SMALL)
    for case in MID:
        assert 5 <= plans[case][3] <= 15 and plans[case][1] > 1, plans[case]
    for case in UNEVEN16:
        ppb, nblk, pl, items = plans[case]
        assert items == 16 and nblk > 1 and 0 < last(case) < ppb and last(case) % pl, plans[case]  # threads of the last block differ
    for case in LONG64:
        ppb, nblk, pl, items = plans[case]
        assert items == 16 and case[4] == 64 and 0 < last(case) < ppb and last(case) % pl, plans[case]
        esz = 4 if case[0] == "f32" else 2
        assert (case[1] + case[1] * case[2]) * case[3] * case[4] * esz <= 150 << 20  # the maps stay under 150 MB
        # the planner's threshold: one pixel row less per block below it
        half = (262144 if case[0] == "f32" else 524288) - pl * 1024
        assert _grid(case[0], 1, 1, half, 64)[3] == 15
    assert {c for _, _, _, _, c in CASES} == {64, 128, 256, 512}
    assert any(k == 1 for _, r, k, _, _ in CASES if r > 1) and any(k >= 7 and k % 2 for _, _, k, _, _ in CASES)
    R, K, c = PLANE_RKC
    print("the plane kernel:")
    for hw in PLANE_HW:
        g = _grid("f32", R, K, hw, c, nchw=True)
        print(f"  hw={hw}: {g}")
        assert g == (min(hw, 4096), -(-hw // 4096), 256, -(-min(hw, 4096) // 256))
    assert R * c > 1 and _grid("f32", R, K, 4097, c, nchw=True)[1] == 2 and 8193 - 2 * 4096 == 1


def _check(feat, R, K, prec, dev, nchw, label):
    """(a) and (b) for one input; feat is NHWC (n, HW, C) in the storage type.  Returns the sums."""
    n, hw, c = feat.shape
    want = G.group_sums_ref(feat, R, K)
    arg = feat.transpose(1, 2).contiguous() if nchw else feat
    sums = _sums(arg, R, K, prec, dev, nchw)
    mism = int((sums != want).sum())
    print(f"\ngroup_sums {label}: plan {_grid(prec, R, K, hw, c, nchw)}; sums differing {mism} of {sums.numel()}")
    assert torch.equal(sums, want), f"{mism} of {sums.numel()} sums are not bit-equal to the float64 sums"
    s1, s2 = _s(arg, R, K, prec, dev, nchw)
    r1, r2 = P.s_from_sums(want, hw)
    e1, e2 = G.s_excess(s1, r1), G.s_excess(s2, r2)
    print(f"   S1 at {e1:.3f}, S2 at {e2:.3f} of 2^-23 |ref| + 2^-40")
    assert e1 <= 1.0 and e2 <= 1.0, (e1, e2)
    (both, dead_x, ren0), groups = G.special_channels(c)
    rows = torch.arange(R if groups is None else groups, device=dev) * K
    for k in range(K):
        assert not sums[rows + k][:, both].any() and not sums[rows + k][:, dead_x][:, [0, 2, 4]].any()
        assert (s1[rows + k][:, both] == 1.0).all() and (s2[rows + k][:, both] == 1.0).all()  # (0 + c) / (0 + c)
    if K >= 2:
        same = torch.arange(R, device=dev) * K + K - 1
        assert (s1[same] == 1.0).all() and (s2[same] == 1.0).all(), "a render identical to its reference does not score exactly 1.0"
        q = sums[same]
        assert torch.equal(q[..., 0], q[..., 1]) and torch.equal(q[..., 2], q[..., 3]) and torch.equal(q[..., 2], q[..., 4])
        assert hw < 9 or not (s2[rows] == 1.0).all()
    return sums, s1, s2


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_nhwc_exact_sums_and_s(case, dev):
    prec, R, K, hw, c = case
    feat = G.group_exact_maps(R, K, hw, c, 17 * hw + c + K, device=dev).to(DTYPE[prec])
    sums, s1, s2 = _check(feat, R, K, prec, dev, False, _id(case))
    if prec == "f32":  # the same kernel under "f32s" (float taps)
        assert torch.equal(_sums(feat, R, K, "f32s", dev), sums)
        t1, t2 = _s(feat, R, K, "f32s", dev)
        assert torch.equal(t1, s1) and torch.equal(t2, s2)


@pytest.mark.parametrize("hw", PLANE_HW)
def test_plane_kernel_exact_sums_and_s(hw, dev):
    R, K, c = PLANE_RKC
    feat = G.group_exact_maps(R, K, hw, c, 77 + hw, device=dev)
    sums, s1, s2 = _check(feat, R, K, "f32", dev, True, f"planes R{R}K{K}_hw{hw}_c{c}")
    planes = feat.transpose(1, 2).contiguous()
    assert torch.equal(_sums(planes, R, K, "f16", dev, True), sums)  # planes are float whatever prec says
    t1, t2 = _s(planes, R, K, "bf16", dev, True)
    assert torch.equal(t1, s1) and torch.equal(t2, s2)


PROPERTY = [("f32", False, 2, 4, 77, 512), ("f16", False, 3, 3, 1551, 256), ("bf16", False, 2, 5, 299, 128),
            ("f32", False, 2, 3, 6007, 512), ("f32", True, 2, 4, 4097, 3), ("f32", True, 3, 3, 35, 3)]


@pytest.mark.parametrize("case", PROPERTY, ids=lambda k: "%s_%s_R%dK%d_hw%d_c%d" % (k[0], "planes" if k[1] else "nhwc", *k[2:]))
def test_exact_properties_of_the_sums(case, dev):
    """(c)."""
    prec, nchw, R, K, hw, c = case
    feat = G.group_exact_maps(R, K, hw, c, 5 + hw + c, device=dev).to(DTYPE[prec])
    ref, ren = feat[:R], feat[R:].view(R, K, hw, c)

    def run(rf, rn, r):
        f = torch.cat([rf, rn.flatten(0, 1)]).contiguous()
        if nchw:
            f = f.transpose(1, 2).contiguous()
        return _sums(f, r, K, prec, dev, nchw).view(r, K, c, 5)

    s = run(ref, ren, R)
    assert torch.equal(s.view(R * K, c, 5), G.group_sums_ref(feat, R, K))
    assert torch.equal(run(ref, ren, R), s), "two launches differ"
    perm = torch.roll(torch.arange(K), 1)
    perm[[0, 1]] = perm[[1, 0]]
    assert not torch.equal(s[:, perm], s)
    assert torch.equal(run(ref, ren[:, perm], R), s[:, perm]), "permuting a group's renders does not permute the rows"
    # a group's rows do not depend on the other groups (the planner reports the same split for the group alone)
    assert _grid(prec, 1, K, hw, c, nchw)[:2] == _grid(prec, R, K, hw, c, nchw)[:2] or (hw, c) == (6007, 512)
    for r in range(R):
        alone = run(ref[r:r + 1], ren[r:r + 1], 1)
        assert torch.equal(alone[0], s[r]), f"group {r}'s sums depend on the other groups"  # (exact inputs: any split agrees)


PAIR_C = (3, 64, 128, 256, 512, 512)
PAIR_SIZES = {"1x1": [(1, 1)] * 6, "5x7": [(5, 7)] * 6, "4097_at_c3": [(17, 241)] + [(5, 7)] * 5}


@pytest.mark.parametrize("sizes", list(PAIR_SIZES), ids=list(PAIR_SIZES))
def test_pair_path_plane_kernel_s(sizes, dev):
    """(d): stats_nchw_kernel, which serves stage 0 of every pairwise forward and all six maps of forward_from_feats."""
    from nerf_qa_amd import _lib, ops
    import ctypes
    B = 3
    fx, fy, want1, want2, same_cols = [], [], [], [], []
    for k, (c, (h, w)) in enumerate(zip(PAIR_C, PAIR_SIZES[sizes])):
        feat = G.group_exact_maps(B, 1, h * w, c, 300 + 7 * k + h, device=dev)  # pairs = groups of one render
        feat[B + 1] = feat[1]  # y = x in pair 1
        r1, r2 = P.s_from_sums(G.group_sums_ref(feat, B, 1), h * w)
        want1.append(r1)
        want2.append(r2)
        nchw = feat.transpose(1, 2).contiguous().view(2 * B, c, h, w)
        fx.append(nchw[:B].contiguous())
        fy.append(nchw[B:].contiguous())
    want1, want2 = torch.cat(want1, 1), torch.cat(want2, 1)
    ctot = sum(PAIR_C)
    s1, s2 = _ff((B, ctot), torch.float32, dev), _ff((B, ctot), torch.float32, dev)
    ints = lambda v: (ctypes.c_int * 6)(*v)
    nbytes = _lib.lib().nqa_stats_scratch_bytes(B, ints(PAIR_C), ints([h for h, _ in PAIR_SIZES[sizes]]), ints([w for _, w in PAIR_SIZES[sizes]]))
    assert nbytes > 0
    t1, t2 = ops.dists_stats_nchw(fx, fy, s1=s1, s2=s2, scratch=_ff((nbytes,), torch.uint8, dev))
    assert t1.data_ptr() == s1.data_ptr() and not torch.isnan(s1).any() and not torch.isnan(s2).any()
    e1, e2 = G.s_excess(s1, want1), G.s_excess(s2, want2)
    print(f"\nstats_nchw {sizes}: S1 at {e1:.3f}, S2 at {e2:.3f} of 2^-23 |ref| + 2^-40")
    assert e1 <= 1.0 and e2 <= 1.0, (e1, e2)
    assert (s1[1] == 1.0).all() and (s2[1] == 1.0).all(), "y = x does not score exactly 1.0"
    off = 0
    for c in PAIR_C:
        (both, dead_x, ren0), groups = G.special_channels(c)
        rows = slice(0, B if groups is None else groups)
        assert (s1[rows, off + both] == 1.0).all() and (s2[rows, off + both] == 1.0).all()
        off += c
    if sizes != "1x1":
        assert not (s2[0] == 1.0).all() and not (s1[2] == 1.0).all()
