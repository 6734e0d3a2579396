"""The figures behind tests/test_gpu_adists_window_n.py, recomputed without a GPU, and the proof that its check has
teeth.  The general-n replay of window_n_refs (a) rebuilds the host's taps, (b) equals the oracle's F.conv2d moments on
the same maps to float64 rounding, (c) is window_refs.stage bit for bit at n = 21; the float32 yardstick passes the GPU
test's own check; and every deliberately wrong replay of window_n_refs.MUTANTS, in float64, sits at least 10 x above
the LARGEST bound of any case on every case it applies to.  Run with -s for the figures."""
import pytest
import torch

import window_n_refs as N
import window_refs as R21


@pytest.fixture(scope="module")
def refs():
    return {N.case_id(c): N.references(c) for c in N.CASES}


def test_taps_are_the_reference_gaussian():
    """Normalised, centred on n // 2 (so an even window is not symmetric), within two float32 steps of the oracle's
    gaussian_1d (which sums in float32 where the host rounds a float64 sum once), and at 21 the kernels' constants."""
    from oracle import adists_oracle as O
    assert torch.equal(N.taps(21, torch.float32), R21.taps(torch.float32))
    for n in range(N.WMIN, N.WMAX + 1):
        g = N.taps(n, torch.float32)
        assert g.numel() == n and int(g.argmax()) == n // 2 and abs(float(g.double().sum()) - 1) < n * 2.0 ** -24
        o = O.gaussian_1d(n, n / 3)
        # (one step of the sum is up to 2^-23 of it, and each quotient's own rounding half a step more: 2^-22)
        assert float(((g - o).abs() / o).max()) <= 2.0 ** -22, n
        sym = torch.equal(g, g.flip(0))
        assert sym == (n % 2 == 1), n
        assert torch.equal(N.table_row(n, n, torch.float32), g)
    assert float(N.table_row(11, 12, torch.float32)[-1]) == 0.0 and N.table_row(13, 12, torch.float32).numel() == 12


@pytest.mark.parametrize("n", (3, 4, 12, 21, 33, 63))
def test_moments_equal_the_oracles_conv2d(n):
    """The separable float64 means against F.conv2d with the outer-product window, on the same maps and the same taps: to
    float64 rounding.  Against the oracle's own window_2d (outer product ROUNDED to float32, float32-summed taps): to
    float32 rounding of the weights."""
    from oracle import adists_oracle as O
    c = N.Case("lanes", "f32", n, 2, 5, n + 9, n + 6, 0, 0, False)
    x, y, _, _ = N.inputs(c)
    g = N.taps(n, torch.float64)
    win = torch.outer(g, g)[None, None].expand(c.C, 1, n, n).contiguous()
    ours = N.moments(x, y, n, torch.float64)
    xd, yd = x.double(), y.double()
    for a, t in zip(ours, (xd, yd, xd * xd, yd * yd, xd * yd)):
        want = O._wconv(t, win)
        assert a.shape == want.shape == (2, 5, 10, 7)
        assert float((a - want).abs().max()) <= 64 * 2.0 ** -53 * float(want.abs().max())
        loose = O._wconv(t, O.window_2d(c.C, n).double())
        # (each 2-D weight: two taps at most 2^-22 from ours, test above, and one float32 rounding of their product;
        # the maps are non-negative, so a mean moves by no more than its weights do)
        assert float((a - loose).abs().max()) <= (2 * 2.0 ** -22 + 2.0 ** -24) * float(want.abs().max())


def test_at_21_the_replay_is_window_refs_stage_bit_for_bit():
    for c21 in (R21.CASES[2], [c for c in R21.CASES if c.kind == "planar"][3], [c for c in R21.CASES if c.kind == "global"][4],
                [c for c in R21.CASES if c.kind == "lanes" and c.prec == "f16"][2]):
        x, y, q, wgt = R21.inputs(c21)
        for dt in (torch.float64, torch.float32):
            for a, b in zip(N.stage(x, y, q, wgt, 21, dt), R21.stage(x, y, q, wgt, dt)):
                assert a.dtype == dt and torch.equal(a, b), R21.case_id(c21)
    c = [c for c in N.CASES if c.n == 21 and not c.K][0]
    x, y, q, wgt = N.inputs(c)
    for m, m21 in (("rot", "a"), ("shift", "b"), ("img0", "d"), ("yx", "h")):
        for a, b in zip(N.stage(x, y, q, wgt, 21, torch.float64, m), R21.stage(x, y, q, wgt, torch.float64, m21)):
            assert torch.equal(a, b), m


def test_case_list_reaches_every_edge():
    by = lambda kind: [c for c in N.CASES if c.kind == kind]
    lanes, planar, glob = by("lanes"), by("planar"), by("global")
    for cs in (lanes, planar):
        assert {c.n for c in cs} == {3, 4, 12, 21, 33, 63}
        assert any(c.K == 3 for c in cs) and any(c.B == 2 and not c.K for c in cs)
        assert any(c.H == c.n and c.W > c.n for c in cs) and any(c.W == c.n and c.H > c.n for c in cs)
        assert any(c.H - c.n + 1 == 65 and not c.strip for c in cs)  # one row more than a block's 64
        assert any(c.strip > 64 for c in cs)
    assert {c.C for c in lanes} == {64, 128} and {c.prec for c in lanes} == {"f32", "f32s", "f16", "bf16"}
    assert {c.W - c.n + 1 for c in planar} >= {1, 64, 65, 68}  # one column more than a block's 64
    assert all(c.generic == (c.n == 21) for c in N.CASES)
    assert all(c.H == c.n - 1 or c.W == c.n - 1 for c in glob) and any(c.K for c in glob) and {c.C for c in glob} == {3, 64, 128}
    assert max(c.H * c.W * c.C for c in N.CASES) == 96 * 112 * 128


def test_float32_yardstick_passes_the_check(refs):
    for c in N.CASES:
        ins, r64, e32 = refs[N.case_id(c)]
        figs, ok = R21.check(N.replay(c, ins, torch.float32), r64, e32)
        print("%-44s e32 gamma %.2e tw %.2e sw %.2e" % ((N.case_id(c),) + e32))
        assert ok, (N.case_id(c), figs)
        assert r64[0].shape[0] == (c.B // c.K if c.K else c.B) and r64[1].shape[0] == c.B
        assert all(e < 2e-5 for e in e32), (N.case_id(c), e32)  # (a yardstick this loose would bound nothing)


def test_every_mutant_sits_ten_bounds_above_every_case(refs):
    largest_bound = max(R21.bound(e) for c in N.CASES for e in refs[N.case_id(c)][2])
    print("largest bound of any case: %.2e" % largest_bound)
    for m, what in N.MUTANTS.items():
        errs = []
        for c in N.CASES:
            if not N.mutant_applies(m, c):
                continue
            ins, r64, _ = refs[N.case_id(c)]
            err = max(R21.rel_err(a, r) for a, r in zip(N.replay(c, ins, torch.float64, m), r64))
            errs.append((err, N.case_id(c)))
            assert err >= 10 * largest_bound, (m, what, N.case_id(c), err, largest_bound)
        assert errs, m
        print("mutant %-6s (%s): %d cases, smallest error %.2e (%.0f x the largest bound) on %s"
              % (m, what, len(errs), min(errs)[0], min(errs)[0] / largest_bound, min(errs)[1]))
