"""What does scoring K renders against ONE reference cost with one shared pyramid per group?  (DISTS.forward_group,
ops.dists_forward_group, nqa_dists_forward_group.)

On one GPU, for each configuration -- 256 x 256 frames with R = 4 references and 1080p frames with R = 1, K = 2 and 8
renders each, in "f32s" and (1080p) in "f16" -- two ways of scoring the same R * K pairs are timed in ONE process:

  (g) model.forward_group(ref, renders)                                   R + R K images through the pyramid
  (p) model(ref.repeat_interleave(K, 0), renders.flatten(0, 1))            2 R K images: the only way without this feature

Both run on a module with the NAMED precision, under no_grad, on frames that live on the device (the repeated references
of (p) are built before the clock starts).  A timing is a pair of device events around a window of --steps calls; the
windows of the two ways alternate, the order swapped from window to window, after both have been warmed up.  Printed per
configuration: ms per call as median [min, max] over the windows for both ways, (p) / (g), the margin (p) - (g) against
the larger min-to-max spread of the two, and max |score difference| between them.

Usage: python tools/gpu_group_bench.py [--out FILE] [--windows N] [--steps N] [--config NAME:H:W:R:K:PREC ...]
Needs a GPU: without one it prints the plan and fails (no fallback).  profiles/group_scoring.txt is one such report."""
import os; os.environ.setdefault("NQA_VGG16_WEIGHTS", "synth:1234")  # dev tool: stand-in weights, asked for explicitly
import argparse
import sys
import warnings

import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])

CONFIGS = ("256:256:256:4:2:f32s", "256:256:256:4:8:f32s", "1080p:1080:1920:1:2:f32s", "1080p:1080:1920:1:8:f32s",
           "1080p:1080:1920:1:2:f16", "1080p:1080:1920:1:8:f16")


def parse_config(s):
    try:
        name, h, w, r, k, prec = s.split(":")
        h, w, r, k = int(h), int(w), int(r), int(k)
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected NAME:H:W:R:K:PREC, got {s!r}")
    if min(h, w, r, k) <= 0:
        raise argparse.ArgumentTypeError(f"sizes must be positive: {s!r}")
    return name, h, w, r, k, prec


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", help="also write the report to this file")
    ap.add_argument("--windows", type=int, default=5, help="timed windows of each way per configuration")
    ap.add_argument("--steps", type=int, default=10, help="calls per window")
    ap.add_argument("--config", nargs="+", type=parse_config, default=[parse_config(s) for s in CONFIGS],
                    help="NAME:H:W:R:K:PREC")
    args = ap.parse_args(argv)
    if args.windows < 1 or args.steps < 1:
        ap.error("--windows and --steps must be at least 1")
    return args


def spread(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def group_frames(r, k, h, w, dev, seed=2026):
    """ref (r,3,h,w) uniform noise mixed with a smooth field; render j of every group = clamp(ref + 0.02 (j + 1) N(0,1))."""
    g = torch.Generator(device=dev).manual_seed(seed)
    low = torch.nn.functional.interpolate(torch.rand(r, 3, max(h // 16, 2), max(w // 16, 2), device=dev, generator=g),
                                          size=(h, w), mode="bilinear", align_corners=False)
    ref = 0.6 * torch.rand(r, 3, h, w, device=dev, generator=g) + 0.4 * low
    ren = torch.empty(r, k, 3, h, w, device=dev)
    for j in range(k):
        ren[:, j] = (ref + 0.02 * (j + 1) * torch.randn(r, 3, h, w, device=dev, generator=g)).clamp_(0, 1)
    return ref, ren


def window(fn, steps, dev):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def main(argv=None):
    args = parse_args(argv)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/gpu_group_bench.py: {[f'{n} {h}x{w} R={r} K={k} {p}' for n, h, w, r, k, p in args.config]}; "
        f"{args.windows} alternating windows of {args.steps} calls per way, device events")
    if not torch.cuda.is_available():
        raise SystemExit("gpu_group_bench: no GPU -- this tool measures on the device and has no CPU path")
    from nerf_qa_amd.DISTS_pytorch import DISTS
    dev = torch.device("cuda:0")
    say(f"# {torch.cuda.get_device_name(dev)}; ms per call, median [min, max] over the windows; (g) group = R + R K images, "
        "(p) pairwise = 2 R K images")
    models = {}
    for name, h, w, r, k, prec in args.config:
        if prec not in models:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                models[prec] = DISTS(precision=prec).to(dev).eval()
        m = models[prec]
        ref, ren = group_frames(r, k, h, w, dev)
        x, y = ref.repeat_interleave(k, 0).contiguous(), ren.flatten(0, 1)
        with torch.no_grad():
            ways = {"g": lambda: m.forward_group(ref, ren), "p": lambda: m(x, y)}
            out = {}
            for _ in range(2):  # warm-up of both ways: weights packed, workspaces grown, code objects loaded
                for kk, fn in ways.items():
                    out[kk] = fn()
            torch.cuda.synchronize(dev)
            times = {"g": [], "p": []}
            for i in range(args.windows):
                for kk in ("g", "p") if i % 2 == 0 else ("p", "g"):
                    times[kk].append(window(ways[kk], args.steps, dev))
        (g, glo, ghi), (p, plo, phi) = spread(times["g"]), spread(times["p"])
        sp = max(ghi - glo, phi - plo)
        diff = (out["g"].flatten() - out["p"]).abs().max().item()
        say(f"\n{name} {h}x{w} R={r} K={k} [{prec}]: {r * k} pairs; images through the pyramid {r + r * k} vs {2 * r * k} "
            f"(ratio {(1 + k) / (2 * k):.4f})")
        say(f"  (g) group    {g:9.3f} ms [{glo:.3f}, {ghi:.3f}]   {1e3 * r * k / g:9.1f} pairs/s")
        say(f"  (p) pairwise {p:9.3f} ms [{plo:.3f}, {phi:.3f}]   {1e3 * r * k / p:9.1f} pairs/s")
        say(f"  (p) / (g) = {p / g:.3f}   (g) / (p) = {g / p:.4f}   margin (p) - (g) = {p - g:+.3f} ms against a spread "
            f"(largest max - min) of {sp:.3f} ms: {'group faster, beyond the spread' if p - g > sp else 'group slower' if g > p else 'within the spread'}")
        say(f"  max |score (g) - (p)| = {diff:.3e}")
        del ref, ren, x, y, out
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
