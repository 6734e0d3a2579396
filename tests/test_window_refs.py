"""The figures behind tests/test_gpu_adists_window.py, recomputed without a GPU, and the proof that its check has teeth.
For every case: the float32 replay's distance e32 from the float64 replay (per map, of the map's maximum) -- the yardstick
the GPU bound is built from -- passes the GPU test's own check function; and every deliberately wrong replay of
window_refs.MUTANTS, in float64, fails that check by at least 4 x the bound on a case it applies to.  Run with -s for
the figures."""
import pytest
import torch

import window_refs as R


@pytest.fixture(scope="module")
def refs():
    return {R.case_id(c): R.references(c) for c in R.CASES}


def test_taps_are_the_kernels_constants():
    g = R.taps(torch.float32)
    want = [float.fromhex(h) for h in R.KG_HEX]
    want = want + want[-2::-1]
    assert [float(v) for v in g] == want
    assert R.taps(torch.float16).dtype == torch.float16 and float(R.taps(torch.float64)[10]) == want[10]


def test_case_list_reaches_every_edge():
    by = lambda kind: [c for c in R.CASES if c.kind == kind and c.family == "A"]
    lds = [c for c in by("lds") if not c.strip]
    assert {c.H - 20 for c in lds} >= {1, 2, 7, 21, 43, 64, 65} and {c.W - 20 for c in lds} >= {1, 2, 3, 4, 5, 10, 24}
    assert {c.C for c in lds if (c.H, c.W) == (27, 30)} == {64, 128, 256, 512}
    assert {(c.H, c.W, c.C, c.strip) for c in by("lds") if c.strip} == {
        (90, 23, 128, 70), (90, 23, 128, 64), (90, 23, 128, 33), (90, 23, 128, 1), (170, 22, 64, 150), (150, 21, 256, 130)}
    assert {c.grid[0] * c.grid[1] * c.B for c in by("lds") if c.grid and not c.strip} == {1, 6, 8, 9, 20}
    lanes = by("lanes")
    assert {(c.prec, c.legacy) for c in lanes} == {("f16", False), ("bf16", False), ("f32", True)}
    assert {(c.H, c.W) for c in lanes} == {(21, 21), (22, 25), (85, 23), (90, 24)} and {c.C for c in lanes} == {64, 256}
    assert {c.W - 20 for c in by("planar")} == {1, 63, 64, 65, 10, 257, 280} and {c.H - 20 for c in by("planar")} >= {64, 65}
    assert {(c.H, c.W, c.C) for c in by("global")} == {(h, w, ch) for h, w in ((1, 1), (5, 7), (20, 50), (50, 20))
                                                        for ch in (3, 64, 512)}
    assert all(c.B == 3 for c in by("global")) and any(c.B > 1 for c in lanes) and any(c.B > 1 for c in by("planar"))
    for fam in ("B", "C"):
        assert {c.kind for c in R.CASES if c.family == fam} == {"lds", "lanes", "planar", "global"}


def test_float32_yardstick_passes_the_check(refs):
    worst = {}
    for c in R.CASES:
        (x, y, q, wgt), r64, e32 = refs[R.case_id(c)]
        r32 = R.stage(x, y, q, wgt, torch.float32)
        figs, ok = R.check(r32, r64, e32, c.family)
        print("%-44s e32 gamma %.2e tw %.2e sw %.2e" % ((R.case_id(c),) + e32))
        assert ok, (R.case_id(c), figs)
        assert all(e < 2e-5 for e in e32), (R.case_id(c), e32)  # (a yardstick this loose would bound nothing)
        key = (c.kind, c.family)
        worst[key] = max(worst.get(key, 0.0), *e32)
    for key, e in sorted(worst.items()):
        print("largest e32 of %-7s family %s: %.2e -> bound %.2e" % (key + (e, R.bound(e, key[1]))))


def test_every_mutant_fails_the_check(refs):
    smallest = float("inf")
    for m, what in R.MUTANTS.items():
        margins = []
        for c in R.CASES:
            if not R.mutant_applies(m, c):
                continue
            (x, y, q, wgt), r64, e32 = refs[R.case_id(c)]
            figs, ok = R.check(R.stage(x, y, q, wgt, torch.float64, mutant=m, strip=c.strip), r64, e32, c.family)
            margin = max(err / b for err, b in figs)
            margins.append((margin, max(err for err, _ in figs), R.case_id(c)))
            assert ok == (margin <= 1)
        assert margins, m
        best = max(margins)
        caught = sum(1 for mg in margins if mg[0] >= 4)
        finite = [mg[1] for mg in margins if mg[0] >= 4 and mg[1] != float("inf")]
        print("mutant %s (%s): fails by >= 4 x bound on %d of %d cases; largest %.3g x on %s; smallest caught error %s"
              % (m, what, caught, len(margins), best[0], best[2], "%.2e" % min(finite) if finite else "NaN"))
        assert best[0] >= 4, (m, what, best)
        if finite:
            smallest = min(smallest, min(finite))
    largest_bound = max(R.bound(e, c.family) for c in R.CASES for e in refs[R.case_id(c)][2])
    print("smallest caught mutant error %.2e; largest bound of any case %.2e" % (smallest, largest_bound))
