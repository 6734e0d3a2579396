"""The yardstick of the score-map kernels (csrc/nqa_score_maps.hip): what the reference's dataset prep does on the CPU
with the K distortion maps of one frame (nerf_nr_qa_prep_4.py:71-133), replayed in float64 torch -- the script's own
operations (clamp, double, torch.std / torch.mean over the renders, amin / amax, -log10, the 255 * (log_max - v) / spread
rescale behind `spread > 0`, byte truncation), written once for all K + 2 quantities of a frame.  A helper module, not a test: the seeded inputs and
the byte rule that the CPU and the GPU tests share live here too.

Two things the script leaves to the platform are pinned down here:
  * `.byte()` of a value that is not finite (an infinite log_max meets `inf / inf`) is 0: what x86 gives, and what
    include/nqa.h states;
  * a plane that is zero by the script's `else torch.zeros_like(...)`, or by the rule above, carries NaN in `values`: its
    bytes did not come from a truncation, so no pixel of it counts as "near an integer".
"""
import warnings

import numpy as np
import torch

NEAR = 1e-9            # a pre-truncation value this close to an integer may truncate either way on another log10
MAX_NEAR_REPLAY = 2    # per plane, on the seeded inputs: the two extremes
MAX_NEAR = 4           # per plane, the most pixels a device result may differ on (by one)
LOGS_RTOL = 1e-12
SHAPES = ((1, 1, 8, 8), (1, 2, 24, 31), (1, 5, 67, 131), (3, 4, 37, 53))  # (F, K, H, W)


def seeded_maps(f, k, h, w, seed=0):
    """(F,K,H,W) float32 uniform in [0.05, 0.65], a pure function of the arguments."""
    from nerf_qa_amd import synth
    u = synth.uniform(1000 + seed, f * k * h * w, stream=31).reshape(f, k, h, w)
    return torch.from_numpy((0.05 + 0.6 * u).astype(np.float32))


def _to_bytes(plane, top, bottom):
    """One quantity's plane (H,W) double onto 0..255 between its two extrema, top = -log10(its minimum) and bottom =
    -log10(its maximum): (values before truncation, NaN where the byte is 0 by rule; bytes)."""
    span = top - bottom
    if not bool(span > 0):  # (also a NaN span)
        return torch.full_like(plane, float("nan")), torch.zeros_like(plane, dtype=torch.uint8)
    depth = -torch.log10(plane)
    scaled = 255 * (top - depth) / span
    ok = torch.isfinite(scaled)
    nan, zero = torch.full_like(scaled, float("nan")), torch.zeros_like(scaled)
    return torch.where(ok, scaled, nan), torch.where(ok, scaled, zero).byte()


def replay_frame(maps):
    """maps (K,H,W) float32 on the CPU: the K as_map results of one frame.  Returns (bytes (K,H,W,3) uint8, values
    (K,H,W,3) float64, logs (2K+4,) float64 in nqa_score_maps' order).  The K maps, their std and their mean are K + 2
    quantities that all go the same way: extrema over the plane, -log10 of both, rescale, truncate."""
    assert maps.dtype == torch.float32 and maps.dim() == 3 and maps.device.type == "cpu"
    k = maps.shape[0]
    v = maps.clamp(1e-10).double()  # the clamp in float32, as on the tensor the metric returns; then float64
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (K = 1: torch.std warns about its degrees of freedom and returns NaN)
        across_std = torch.std(v, dim=0)
    across_mean = torch.mean(v, dim=0)
    quantities = list(v) + [across_std, across_mean]
    top = [-torch.log10(p.amin()) for p in quantities]      # the "log max" of a quantity comes from its minimum
    bottom = [-torch.log10(p.amax()) for p in quantities]
    done = [_to_bytes(p, t, b) for p, t, b in zip(quantities, top, bottom)]
    (std_vals, std_bytes), (mean_vals, mean_bytes) = done[k], done[k + 1]
    # one HWC image per render: channels (mean, that render's map, std)
    vals = torch.stack([torch.stack([mean_vals, done[i][0], std_vals], dim=-1) for i in range(k)])
    byts = torch.stack([torch.stack([mean_bytes, done[i][1], std_bytes], dim=-1) for i in range(k)])
    logs = torch.stack(top[:k] + bottom[:k] + [top[k], bottom[k], top[k + 1], bottom[k + 1]])
    return byts.contiguous(), vals.contiguous(), logs


def replay(maps):
    """replay_frame over the frames of maps (F,K,H,W): (bytes (F,K,H,W,3), values (F,K,H,W,3), logs (F,2K+4))."""
    parts = [replay_frame(m) for m in maps]
    return tuple(torch.stack([p[i] for p in parts]) for i in range(3))


def near_integer(values):
    """Where a pre-truncation value lies within NEAR of an integer (False where the byte is 0 by rule: NaN)."""
    return torch.isfinite(values) & ((values - values.round()).abs() < NEAR)


def per_plane(mask):
    """(F,K,H,W,3) bool -> the count per (frame, render, channel) plane, (F,K,3)."""
    return mask.sum(dim=(2, 3))


def check_bytes(got, ref_bytes, ref_values):
    """The byte rule: `got` equals the replay wherever the replay's pre-truncation value is at least NEAR from an integer
    (and wherever the byte is 0 by rule); on the rest it may differ by one, and the rest is at most MAX_NEAR pixels per
    plane -- a condition on the inputs, not a tolerance.  Returns (pixels that differ, pixels near an integer)."""
    got, near = got.cpu(), near_integer(ref_values)
    assert got.shape == ref_bytes.shape and got.dtype == torch.uint8
    assert int(per_plane(near).max()) <= MAX_NEAR, f"{int(per_plane(near).max())} pixels of one plane within {NEAR} of an integer"
    delta = (got.int() - ref_bytes.int()).abs()
    bad = (delta > 0) & ~near
    assert not bad.any(), f"{int(bad.sum())} bytes differ away from an integer boundary, first at {bad.nonzero()[0].tolist()}"
    assert int(delta.max()) <= 1, f"a byte differs by {int(delta.max())}"
    return int((delta > 0).sum()), int(near.sum())


def check_logs(got, ref):
    """Within LOGS_RTOL relative of the replay; NaN where it is NaN, the same infinity where it is infinite."""
    got = got.cpu()
    assert got.shape == ref.shape and got.dtype == torch.float64
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), (got, ref)
    assert torch.equal(got[torch.isinf(ref)], ref[torch.isinf(ref)]), (got, ref)
    assert torch.isfinite(got[fin]).all(), (got, ref)
    err = ((got[fin] - ref[fin]).abs() / ref[fin].abs().clamp_min(1e-300)).max().item() if fin.any() else 0.0
    assert err <= LOGS_RTOL, f"logs off by {err:.3e} relative"
    return err


# ---- the stated edge cases: name -> (K,H,W) float32 maps of one frame ------------------------------------------------
def edge_cases():
    base = seeded_maps(1, 3, 19, 23, seed=7)[0]
    cases = {}
    m = base.clone()
    m[0, 2, 3], m[0, 5, 7], m[1, 0, 0], m[2, 18, 22] = 0.0, -0.25, 3e-11, -1e-3
    cases["nonpositive_and_below_clamp"] = m
    m = base.clone()
    m[1] = 0.3125
    cases["constant_map"] = m
    m = base.clone()
    m[:, 11, 13] = 0.40625
    cases["pixel_equal_across_k"] = m
    m = base.clone()
    m[1, 4, 9] = float("nan")
    cases["nan_pixel"] = m
    cases["k1"] = base[:1].clone()
    return cases
