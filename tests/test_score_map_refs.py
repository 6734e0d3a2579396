"""The float64 replay of nerf_nr_qa_prep_4.py:71-133 (tests/score_map_refs.py) held to what the script's formula implies,
on the CPU and without the library: the yardstick of tests/test_gpu_score_maps.py has to be right on its own."""
import pytest
import torch

import score_map_refs as R


@pytest.fixture(scope="module")
def cases():
    return {name: (m,) + R.replay_frame(m) for name, m in R.edge_cases().items()}


def test_k1_std_plane_is_zero(cases):
    m, byts, vals, logs = cases["k1"]
    assert byts.shape == (1,) + tuple(m.shape[1:]) + (3,)
    assert not byts[..., 2].any() and torch.isnan(vals[..., 2]).all()
    assert torch.isnan(logs[2]) and torch.isnan(logs[3])  # std_max, std_min: torch.std of one sample
    assert byts[..., 0].any() and byts[..., 1].any()       # mean == the map: both planes live
    assert torch.equal(byts[..., 0], byts[..., 1])


def test_constant_map_plane_is_zero(cases):
    m, byts, _, logs = cases["constant_map"]
    k = m.shape[0]
    assert not byts[1, ..., 1].any() and logs[1] == logs[k + 1]  # spread 0
    for i in (0, 2):
        assert byts[i, ..., 1].any()
    assert byts[..., 0].any() and byts[..., 2].any()


def test_one_pixel_equal_across_k_zeroes_the_whole_std_plane(cases):
    m, byts, _, logs = cases["pixel_equal_across_k"]
    k = m.shape[0]
    assert logs[2 * k] == float("inf")  # std_max = -log10(0)
    assert not byts[..., 2].any()
    assert byts[..., 0].any() and byts[..., 1].any()


def test_one_nan_pixel_zeroes_its_map_the_mean_and_the_std_plane(cases):
    m, byts, _, logs = cases["nan_pixel"]
    k = m.shape[0]
    assert not byts[1, ..., 1].any() and not byts[..., 0].any() and not byts[..., 2].any()
    for i in (0, 2):
        assert byts[i, ..., 1].any() and torch.isfinite(logs[i]) and torch.isfinite(logs[k + i])
    assert torch.isnan(logs[1]) and torch.isnan(logs[k + 1]) and torch.isnan(logs[2 * k:]).all()


def test_values_at_or_below_zero_clamp_to_1e_minus_10(cases):
    m, byts, vals, logs = cases["nonpositive_and_below_clamp"]
    # float32(1e-10) as a double: the clamp runs on the float32 tensor
    want = -torch.log10(torch.tensor(1e-10, dtype=torch.float32).double()).item()
    assert logs[0] == want and logs[1] == want and logs[2] == want
    assert byts[0, 2, 3, 1] == 0 and byts[0, 5, 7, 1] == 0 and byts[1, 0, 0, 1] == 0 and byts[2, 18, 22, 1] == 0
    assert torch.isfinite(vals).all()


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_seeded_inputs_keep_truncation_away_from_integers(shape):
    """On the inputs of the GPU test at most the two extremes of a plane truncate from within 1e-9 of an integer, so the
    byte rule pins every other pixel exactly."""
    maps = R.seeded_maps(*shape)
    assert maps.min() >= 0.05 and maps.max() <= 0.65
    byts, vals, logs = R.replay(maps)
    f, k, h, w = shape
    assert byts.shape == (f, k, h, w, 3) and vals.shape == byts.shape and logs.shape == (f, 2 * k + 4)
    near = R.per_plane(R.near_integer(vals))
    print(f"\n{shape}: {int(near.sum())} of {f * k * h * w * 3} values within {R.NEAR} of an integer, at most "
          f"{int(near.max())} per plane")
    assert int(near.max()) <= R.MAX_NEAR_REPLAY
    live = torch.isfinite(vals)
    assert torch.equal(byts[live].double(), vals[live].floor()) and vals[live].min() >= 0 and vals[live].max() < 256
    if k > 1:
        assert live.all() and int(byts.max()) >= 254 and int(byts.min()) == 0
    assert torch.equal(R.replay(maps)[0], byts)  # the yardstick itself repeats
