"""The figures behind tests/test_gpu_adists_front.py, recomputed without a GPU, and the proof that its check has teeth.
The float64 replay's weights are the oracle's (oracle/adists_oracle.py, run in float64) to 1e-12; for every case the
float32 replay -- the yardstick -- passes the GPU test's own check function and sits below the floor it is used with;
and every deliberately wrong replay of front_refs.MUTANTS, in float64, fails that check by at least 4 x the bound on a
case it applies to.  Run with -s for the figures."""
import pytest
import torch

import front_refs as R

E32_MAX = 2e-5  # a yardstick looser than this would bound nothing (tests/test_window_refs.py)


@pytest.fixture(scope="module")
def refs():
    return {R.case_id(c): R.references(c) for c in R.CASES}


def test_float64_replay_gives_the_oracles_weights(refs):
    from oracle import adists_oracle
    for c in R.CASES:
        if c.name != "mixed" or c.prec != "f32":
            continue
        (x, y, taps), r64, _, _ = refs[R.case_id(c)]
        tx, _ = R.nchw(taps, c.B)
        want = torch.cat(adists_oracle.channel_weights([x.double()] + [t.double() for t in tx]), 1)[:, :, 0]
        assert want.dtype == torch.float64 and want.shape == r64["wgt"].shape
        err = float((want - r64["wgt"]).abs().max() / want.abs().max())
        print("%-24s max|wgt - oracle| / max|oracle| = %.2e" % (R.case_id(c), err))
        assert err <= 1e-12, (R.case_id(c), err)
        for k, s in enumerate(R.stage_slices()):  # and the stage's entropy weights, before the clamp
            ew = adists_oracle.entropy_weight(([x] + tx)[k].double())[:, :, 0]
            h = r64["q"][2][:, s]
            assert float((ew - h / (h.sum(1, keepdim=True) + 1e-12) * R.CHNS[k]).abs().max()) <= 1e-12 * float(ew.abs().max())


def test_case_list_reaches_every_edge():
    by = {}
    for c in R.CASES:
        p = R.plan(c.B, c.dims, c.prec)
        for k, want in c.expect.items():
            assert all(w is None or w == g for w, g in zip(want, p[k])), (R.case_id(c), k, want, p[k])
        by.setdefault(c.family, []).append((c, p))
    A = by["A"]
    pool64 = {c.dims[1]: p[1] for c, p in A if c.name.startswith("pool64")}
    assert {d: g[:3] for d, g in pool64.items()} == {
        (8, 32): (1, 4, 16), (8, 33): (2, 4, 16), (9, 32): (2, 4, 16), (9, 33): (4, 4, 16), (3, 5): (1, 2, 16),
        (1, 1): (1, 1, 16), (1, 13): (1, 1, 16), (13, 1): (2, 4, 16), (2, 2): (1, 1, 16)}
    assert {(c.prec, k, p[k][2]) for c, p in A if c.name in ("pool-wide-13x19", "pool-16bit") for k in c.expect} == {
        ("f32", 1, 16), ("f32", 2, 8), ("f32", 3, 4), ("f32", 4, 2), ("f16", 1, 32), ("f16", 4, 4), ("bf16", 1, 32),
        ("bf16", 4, 4)}
    assert all(p[k][0] >= 4 for c, p in A if c.name in ("pool-wide-13x19", "pool-16bit") for k in c.expect if k > 1)
    xcd = {c.name: c.B * p[max(c.expect)][0] for c, p in A if c.name.startswith("pool-xcd")}
    assert xcd == {"pool-xcd12": 12, "pool-xcd8": 8}
    assert {c.dims[5]: (p[5][0], p[5][3]) for c, p in A if c.name.startswith("tap5")} == {
        (2, 4): (1, 1), (3, 3): (2, 2), (23, 23): (67, 67)}
    assert 23 * 23 % 8 == 1 and 3 * 3 % 8 == 1  # (the last block holds one pixel)
    assert {c.dims[1]: p[1][3] for c, p in A if c.name.startswith("ent64")} == {(8, 8): 1, (5, 13): 2}
    assert {c.dims[0]: (p[0][0], p[0][3]) for c, p in A if c.name.startswith("image")} == {
        (5, 7): (1, 1), (64, 64): (1, 4), (65, 64): (2, 5)}
    assert {(c.prec, c.B) for c, _ in A if c.name == "mixed"} == {(p, b) for p in R.STORAGE for b in (1, 3)}
    for fam in ("B", "C"):
        assert {(c.name, c.prec) for c, _ in by[fam]} == {("mixed", "f32"), ("mixed", "f16"), ("tap5-23x23", "f32")}
    # the largest tap is the 23 x 23 x 512 float one the 67 blocks need: a little over 1 MiB an image
    assert max(t[0].numel() * t.element_size() for c in R.CASES for t in R.inputs(c)[2]) == 23 * 23 * 512 * 4


def test_families_are_well_conditioned_and_the_yardstick_passes(refs):
    largest = {}
    for c in R.CASES:
        (x, y, taps), r64, e32, dead = refs[R.case_id(c)]
        assert all(bool(torch.isfinite(v).all()) for v in r64.values()), R.case_id(c)
        tx, ty = R.nchw(taps, c.B)
        r32 = R.front(x, y, tx, ty, torch.float32, prec=c.prec)
        figs, ok = R.check(r32, r64, e32, dead)
        flat = e32["hsum"] + e32["wgt"]
        print("%-28s e32 hsum %.2e wgt %.2e | %s" % (R.case_id(c), max(e32["hsum"]), max(e32["wgt"]), R.show(figs)))
        # the yardstick is used for hsum and wgt alone: the bounds on q's rows are fixed figures, and the reference's
        # own one-pass covariance in float32 misses them on family B's nearly constant channel
        mine = {n: r for n, (r, _) in R.worst(figs).items() if n not in ("mean", "var", "inv")}
        assert ok or c.family == "B", (R.case_id(c), figs)
        assert max(mine.values()) <= 1, (R.case_id(c), mine)
        assert max(flat) < E32_MAX, (R.case_id(c), e32)
        for k, (h, w) in enumerate(c.dims):  # a 1 x 1 tap: entropies of exactly 0 (front_refs.ONE_PIXEL), weights on the clamp
            if h * w == 1:
                s = R.stage_slices()[k]
                assert bool((r64["q"][2][:, s] == 0).all()) and bool((r32["q"][2][:, s] == 0).all())
                assert bool((r64["wgt"][:, s] == r64["lo"][:, None]).all())
        if c.family == "C":  # a dead stage: entropy total 0, every weight on the clamp's lower bound
            s = R.stage_slices()[R.DEAD_STAGE]
            assert bool((r64["q"][2][:, s] == 0).all()) and bool((r64["lo"] > 0).all())
            assert bool((r64["wgt"][:, s] == r64["lo"][:, None]).all())
        for name in ("hsum", "wgt"):
            key = (c.family, name)
            largest[key] = max(largest.get(key, 0.0), max(e32[name]))
    for key, e in sorted(largest.items()):
        print("largest e32 of family %s %-4s: %.2e -> bound %.2e" % (key + (e, max(R.YARD * e, R.FLOOR))))


def test_every_mutant_fails_the_check(refs):
    for m, what in R.MUTANTS.items():
        margins = []
        for c in R.CASES:
            if not R.mutant_applies(m, c):
                continue
            (x, y, taps), r64, e32, dead = refs[R.case_id(c)]
            tx, ty = R.nchw(taps, c.B)
            figs, ok = R.check(R.front(x, y, tx, ty, torch.float64, mutant=m, prec=c.prec), r64, e32, dead)
            margin = max(r for _, r, _ in figs)
            assert ok == (margin <= 1)
            margins.append((margin, R.case_id(c), max(R.worst(figs).items(), key=lambda kv: kv[1][0])[0]))
        assert margins, m
        best = max(margins)
        caught = sum(1 for mg in margins if mg[0] >= 4)
        print("mutant %-8s (%s): fails by >= 4 x bound on %d of %d cases; largest %.3g x (%s) on %s"
              % (m, what, caught, len(margins), best[0], best[2], best[1]))
        assert best[0] >= 4, (m, what, best)
