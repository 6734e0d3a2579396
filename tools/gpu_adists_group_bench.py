"""What does A-DISTS of K renders against ONE reference cost when everything it takes from the reference alone runs once
per group?  (ADISTS.forward_group, ops.adists_forward_group, nqa_adists_forward_group.)

On one GPU, for each configuration -- 256 x 256 frames with R = 4 references and 1080p frames with R = 1, K = 2 and 8
renders each, in the default precision ("auto": f32s at these sizes) -- two ways of scoring the same R * K pairs are
timed in ONE process:

  (g) model.forward_group(ref, renders)                                   R + R K images through the pyramid; entropy
                                                                          weights and probability chain per reference
  (p) model(ref.repeat_interleave(K, 0), renders.flatten(0, 1), as_loss=False)   2 R K images: the parent's only way

Both run under no_grad on frames that live on the device (the repeated references of (p) are built before the clock
starts); (p) is the module's own forward, two HIP streams included where it takes them.  A timing is a pair of device
events around a window of --steps calls; the windows of the two ways alternate, the order swapped from window to window,
after both have been warmed up.  Printed per configuration: ms per call as median [min, max] over the windows for both
ways, (p) / (g), the margin (p) - (g) against the larger min-to-max spread of the two, max |score difference|, and the
device time of ONE call of each way per kernel class, from the library's timing ring (nqa_timing_enable), both on one
stream (where (p) splits a batch over two streams its timed calls do; the split is taken with NQA_ADISTS_STREAMS=1).

Every configuration runs in a child process of its own under a time limit (--limit seconds); the parent never touches
the GPU, checks every exit status and starts nothing more after a child that failed or ran out of time.

Usage: python tools/gpu_adists_group_bench.py [--out FILE] [--windows N] [--steps N] [--limit S]
                                               [--config NAME:H:W:R:K ...]
Needs a GPU: without one it prints the plan and fails (no fallback).  profiles/adists_group_scoring.txt is one such
report."""
import os; os.environ.setdefault("NQA_VGG16_WEIGHTS", "synth:1234")  # dev tool: stand-in weights, asked for explicitly
import argparse
import subprocess
import sys
import warnings

sys.path.insert(0, __file__.rsplit("/", 2)[0])

CONFIGS = ("256:256:256:4:2", "256:256:256:4:8", "1080p:1080:1920:1:2", "1080p:1080:1920:1:8")
DEFAULT_OUT = os.path.join(__file__.rsplit("/", 2)[0], "profiles", "adists_group_scoring.txt")


def parse_config(s):
    try:
        name, h, w, r, k = s.split(":")
        h, w, r, k = int(h), int(w), int(r), int(k)
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected NAME:H:W:R:K, got {s!r}")
    if min(h, w, r, k) <= 0:
        raise argparse.ArgumentTypeError(f"sizes must be positive: {s!r}")
    return name, h, w, r, k


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=DEFAULT_OUT, help="the report file (default profiles/adists_group_scoring.txt)")
    ap.add_argument("--windows", type=int, default=5, help="timed windows of each way per configuration")
    ap.add_argument("--steps", type=int, default=10, help="calls per window")
    ap.add_argument("--limit", type=int, default=240, help="seconds a configuration's process may run")
    ap.add_argument("--config", nargs="+", type=parse_config, default=[parse_config(s) for s in CONFIGS],
                    help="NAME:H:W:R:K")
    ap.add_argument("--child", type=parse_config, help=argparse.SUPPRESS)  # one configuration, in this process
    args = ap.parse_args(argv)
    if args.windows < 1 or args.steps < 1 or args.limit < 1:
        ap.error("--windows, --steps and --limit must be at least 1")
    return args


def spread(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def group_frames(r, k, h, w, dev, seed=2026):
    """ref (r,3,h,w) uniform noise mixed with a smooth field; render j of every group = clamp(ref + 0.02 (j + 1) N(0,1))
    (the frames of tools/gpu_group_bench.py)."""
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    low = torch.nn.functional.interpolate(torch.rand(r, 3, max(h // 16, 2), max(w // 16, 2), device=dev, generator=g),
                                          size=(h, w), mode="bilinear", align_corners=False)
    ref = 0.6 * torch.rand(r, 3, h, w, device=dev, generator=g) + 0.4 * low
    ren = torch.empty(r, k, 3, h, w, device=dev)
    for j in range(k):
        ren[:, j] = (ref + 0.02 * (j + 1) * torch.randn(r, 3, h, w, device=dev, generator=g)).clamp_(0, 1)
    return ref, ren


def window(fn, steps, dev):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def run_config(cfg, windows, steps):
    """One configuration in this process; prints its block of the report."""
    import torch
    from nerf_qa_amd import ops
    from nerf_qa_amd.ADISTS import ADISTS
    name, h, w, r, k = cfg
    say = lambda s="": print(s, flush=True)
    if not torch.cuda.is_available():
        raise SystemExit("gpu_adists_group_bench: no GPU -- this tool measures on the device and has no CPU path")
    dev = torch.device("cuda:0")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = ADISTS().to(dev).eval()
    prec = m.precision_for(h, w)
    ref, ren = group_frames(r, k, h, w, dev)
    x, y = ref.repeat_interleave(k, 0).contiguous(), ren.flatten(0, 1)
    with torch.no_grad():
        ways = {"g": lambda: m.forward_group(ref, ren), "p": lambda: m(x, y, as_loss=False)}
        out = {}
        for _ in range(2):  # warm-up of both ways: weights packed, workspaces grown, code objects loaded
            for kk, fn in ways.items():
                out[kk] = fn()
        torch.cuda.synchronize(dev)
        times = {"g": [], "p": []}
        for i in range(windows):
            for kk in ("g", "p") if i % 2 == 0 else ("p", "g"):
                times[kk].append(window(ways[kk], steps, dev))
        split = {}
        # one call of each way with every launch bracketed by events, on ONE stream: the two half-batches that (p) runs
        # side by side at 1080p would each be timed while the other runs, and their sum would say nothing
        streams = os.environ.get("NQA_ADISTS_STREAMS")
        os.environ["NQA_ADISTS_STREAMS"] = "1"
        for kk, fn in ways.items():
            ops.timing_enable(True)
            fn()
            torch.cuda.synchronize(dev)
            split[kk] = ops.timing_collect()
            ops.timing_enable(False)
        if streams is None:
            del os.environ["NQA_ADISTS_STREAMS"]
        else:
            os.environ["NQA_ADISTS_STREAMS"] = streams
    (g, glo, ghi), (p, plo, phi) = spread(times["g"]), spread(times["p"])
    sp = max(ghi - glo, phi - plo)
    diff = (out["g"].flatten() - out["p"]).abs().max().item()
    say(f"\n{name} {h}x{w} R={r} K={k} [{prec}] on {torch.cuda.get_device_name(dev)}: {r * k} pairs; images through the "
        f"pyramid {r + r * k} vs {2 * r * k} (ratio {(1 + k) / (2 * k):.4f})")
    say(f"  (g) group    {g:9.3f} ms [{glo:.3f}, {ghi:.3f}]   {1e3 * r * k / g:9.1f} pairs/s")
    say(f"  (p) pairwise {p:9.3f} ms [{plo:.3f}, {phi:.3f}]   {1e3 * r * k / p:9.1f} pairs/s")
    verdict = "group faster, beyond the spread" if p - g > sp else "group slower" if g > p else "within the spread"
    say(f"  (p) / (g) = {p / g:.3f}   (g) / (p) = {g / p:.4f}   margin (p) - (g) = {p - g:+.3f} ms against a spread "
        f"(largest max - min) of {sp:.3f} ms: {verdict}")
    say(f"  max |score (g) - (p)| = {diff:.3e}")
    say("  device ms of one call per kernel class (launches), timing ring:   (g) group | (p) pairwise")
    for cls in split["g"]:
        (ng, mg), (npw, mp) = split["g"][cls], split["p"][cls]
        if ng or npw:
            say(f"    {cls:<11s} {mg:9.3f} ({ng:3d}) | {mp:9.3f} ({npw:3d})")
    say(f"    {'sum':<11s} {sum(v[1] for v in split['g'].values()):9.3f}       | "
        f"{sum(v[1] for v in split['p'].values()):9.3f}")


def main(argv=None):
    args = parse_args(argv)
    if args.child:
        return run_config(args.child, args.windows, args.steps)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/gpu_adists_group_bench.py: {[f'{n} {h}x{w} R={r} K={k}' for n, h, w, r, k in args.config]}; "
        f"{args.windows} alternating windows of {args.steps} calls per way, device events; ms per call, median [min, max] "
        "over the windows; (g) group = R + R K images, (p) pairwise = 2 R K images; default precision")
    failed = False
    for cfg in args.config:  # one child per configuration, under its own time limit; nothing follows a failure
        cmd = [sys.executable, os.path.abspath(__file__), "--windows", str(args.windows), "--steps", str(args.steps),
               "--child", ":".join(str(v) for v in cfg)]
        try:
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.limit)  # (stderr passes through)
        except subprocess.TimeoutExpired as e:
            say((e.stdout or b"").decode() if isinstance(e.stdout, bytes) else (e.stdout or ""))
            say(f"# {cfg}: no result within {args.limit} s; stopping here")
            failed = True
            break
        say(res.stdout.rstrip("\n"))
        if res.returncode != 0:
            say(f"# {cfg}: exit status {res.returncode}; stopping here")
            failed = True
            break
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main() or 0)
