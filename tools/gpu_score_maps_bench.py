"""What does a frame of the no-reference dataset prep cost (nerf_nr_qa_prep_4.py:55-135: K renders of one frame against
its ground truth, as_map=True, then std / mean / -log10 rescale / bytes), and where does the time go?

On one GPU, for each configuration -- K = 8 renders at 756 x 1344 (the script's 0.7 crop of 1080p) and at 256 x 256 --
three ways of producing the K score-map images and the 2K + 4 logged extrema of ONE frame, on the host, are timed in one
process:

  (p) the parent's way: K calls adists(render, gt, as_map=True), each moved to the CPU as the script does (:70-71), then
      the script's float64 arithmetic on the CPU (:73-133, restated below).  Needs nothing of this change: it also runs
      on a build of the parent commit (--ways p).
  (s) scoremaps.score_maps(adists, renders, gt), then rgb and logs copied to the host
  (g) the same with share_gt=True

All under no_grad, frames on the device, default precision.  A timing is wall-clock time around a window of --steps
frames with the device drained at both ends; the windows of the ways alternate, the order rotated from window to window,
after all have been warmed up.  Every way is split into its metric part (the as_map maps on the device) and its tail
(everything after them, up to bytes and extrema on the host): for (p) both are timed inside the loop, with the device
drained between them; for (s) and (g) the tail -- ops.score_maps and the two copies to the host -- is timed in windows of
its own on maps that are already there.  Printed per configuration: ms per frame as median [min, max] over the windows,
the split, (p) / (s), (p) / (g), (s) / (g), each margin against the larger min-to-max spread, and how the bytes and the
extrema of (s) compare with (p)'s.

Every configuration runs in a child process of its own under a time limit (--limit seconds); the parent never touches
the GPU, checks every exit status and starts nothing more after a child that failed or ran out of time.

Usage: python tools/gpu_score_maps_bench.py [--out FILE] [--windows N] [--steps N] [--limit S] [--ways psg]
                                             [--config NAME:H:W:K ...]
Needs a GPU: without one it fails (no fallback).  profiles/score_maps.txt is one such report."""
import os; os.environ.setdefault("NQA_VGG16_WEIGHTS", "synth:1234")  # dev tool: stand-in weights, asked for explicitly
import argparse
import subprocess
import sys
import time
import warnings

sys.path.insert(0, __file__.rsplit("/", 2)[0])

CONFIGS = ("crop1080p:756:1344:8", "256:256:256:8")
DEFAULT_OUT = os.path.join(__file__.rsplit("/", 2)[0], "profiles", "score_maps.txt")
WAY_NAMES = {"p": "K as_map calls + CPU tail", "s": "score_maps", "g": "score_maps share_gt"}


def parse_config(s):
    try:
        name, h, w, k = s.split(":")
        h, w, k = int(h), int(w), int(k)
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected NAME:H:W:K, got {s!r}")
    if min(h, w, k) <= 0:
        raise argparse.ArgumentTypeError(f"sizes must be positive: {s!r}")
    return name, h, w, k


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=DEFAULT_OUT, help="the report file (default profiles/score_maps.txt)")
    ap.add_argument("--windows", type=int, default=5, help="timed windows of each way per configuration")
    ap.add_argument("--steps", type=int, default=3, help="frames per window")
    ap.add_argument("--limit", type=int, default=300, help="seconds a configuration's process may run")
    ap.add_argument("--ways", default="psg", help="which of p, s, g to time (p alone runs on the parent commit)")
    ap.add_argument("--config", nargs="+", type=parse_config, default=[parse_config(s) for s in CONFIGS], help="NAME:H:W:K")
    ap.add_argument("--child", type=parse_config, help=argparse.SUPPRESS)  # one configuration, in this process
    args = ap.parse_args(argv)
    if args.windows < 1 or args.steps < 1 or args.limit < 1 or not args.ways or set(args.ways) - set("psg"):
        ap.error("--windows, --steps and --limit must be at least 1, --ways a subset of psg")
    return args


def spread(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def host_tail(maps):
    """What the script does on the CPU after its K as_map calls (nerf_nr_qa_prep_4.py:73-133), on the list of K
    (1,1,H,W) float64 CPU maps of :71, in this project's own words (tests/score_map_refs.py is the same arithmetic): the K
    maps, their std and their mean all go one way -- extrema over the plane, -log10 of both, rescale to 0..255, truncate;
    a byte whose value is not finite is 0.  Returns (bytes (K,H,W,3) uint8, the 2K + 4 extrema in nqa_score_maps' order)."""
    import torch
    v = torch.cat(maps)[:, 0]  # (K,H,W)
    k = v.shape[0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        quantities = list(v) + [torch.std(v, dim=0), torch.mean(v, dim=0)]
    top = [-torch.log10(p.amin()) for p in quantities]
    bottom = [-torch.log10(p.amax()) for p in quantities]
    planes = []
    for p, t, b in zip(quantities, top, bottom):
        span = t - b
        if bool(span > 0):
            scaled = 255 * (t - (-torch.log10(p))) / span
            planes.append(torch.where(torch.isfinite(scaled), scaled, torch.zeros_like(scaled)).byte())
        else:
            planes.append(torch.zeros_like(p, dtype=torch.uint8))
    images = torch.stack([torch.stack([planes[k + 1], planes[i], planes[k]], dim=-1) for i in range(k)])
    order = top[:k] + bottom[:k] + [top[k], bottom[k], top[k + 1], bottom[k + 1]]
    return images, [e.item() for e in order]


def frames(k, h, w, dev, seed=2026):
    """gt (3,h,w) uniform noise mixed with a smooth field; render j = clamp(gt + 0.02 (j + 1) N(0,1))."""
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    low = torch.nn.functional.interpolate(torch.rand(1, 3, max(h // 16, 2), max(w // 16, 2), device=dev, generator=g),
                                          size=(h, w), mode="bilinear", align_corners=False)[0]
    gt = 0.6 * torch.rand(3, h, w, device=dev, generator=g) + 0.4 * low
    ren = torch.stack([(gt + 0.02 * (j + 1) * torch.randn(3, h, w, device=dev, generator=g)).clamp_(0, 1) for j in range(k)])
    return gt, ren


def run_config(cfg, windows, steps, which):
    """One configuration in this process; prints its block of the report."""
    import torch
    from nerf_qa_amd.ADISTS import ADISTS
    name, h, w, k = cfg
    say = lambda s="": print(s, flush=True)
    if not torch.cuda.is_available():
        raise SystemExit("gpu_score_maps_bench: no GPU -- this tool measures on the device and has no CPU path")
    dev = torch.device("cuda:0")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = ADISTS().to(dev).eval()
    gt, ren = frames(k, h, w, dev)
    sync = lambda: torch.cuda.synchronize(dev)
    split = {kk: {"metric": [], "tail": []} for kk in which}
    out = {}

    def way_p(record):
        t0 = time.perf_counter()
        maps = [m(ren[j:j + 1], gt[None], as_map=True) for j in range(k)]  # :70, x = the render
        sync()
        t1 = time.perf_counter()
        out["p"] = host_tail([s.clamp(1e-10).detach().cpu().double() for s in maps])  # :71
        t2 = time.perf_counter()
        if record:
            split["p"]["metric"].append(1e3 * (t1 - t0))
            split["p"]["tail"].append(1e3 * (t2 - t1))

    def way_new(kk, share):
        from nerf_qa_amd import scoremaps
        res = scoremaps.score_maps(m, ren, gt, share_gt=share)
        out[kk] = (res.rgb.cpu(), res.logs.cpu().tolist())
        out[kk + "_maps"] = res.maps

    ways = {"p": lambda record=False: way_p(record), "s": lambda record=False: way_new("s", False),
            "g": lambda record=False: way_new("g", True)}
    ways = {kk: ways[kk] for kk in which}

    def window(fn):
        sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn(True)
        sync()
        return 1e3 * (time.perf_counter() - t0) / steps

    with torch.no_grad():
        for _ in range(2):  # warm-up of every way: weights packed, workspaces grown, code objects loaded
            for fn in ways.values():
                fn()
        sync()
        times = {kk: [] for kk in ways}
        order = list(ways)
        for i in range(windows):
            for kk in order[i % len(order):] + order[:i % len(order)]:
                times[kk].append(window(ways[kk]))
        for kk in ("s", "g"):  # the tail alone, on maps that are already there
            if kk in ways:
                from nerf_qa_amd import ops
                maps = out[kk + "_maps"][None].contiguous()

                def tail():
                    rgb, logs = ops.score_maps(maps, m._ws)
                    return rgb.cpu(), logs.cpu()
                tail()
                for _ in range(windows):
                    split[kk]["tail"].append(window(lambda record: tail()))
    say(f"\n{name} {h}x{w} K={k} [{m.precision_for(h, w)}] on {torch.cuda.get_device_name(dev)}: one frame = {k} renders "
        f"against one ground truth; images through the pyramid: (p) (s) {2 * k}, (g) {k + 1}; {torch.get_num_threads()} CPU threads")
    med = {}
    for kk in ways:
        t, lo, hi = spread(times[kk])
        med[kk] = (t, lo, hi)
        tt, tlo, thi = spread(split[kk]["tail"])
        if kk == "p":
            mt, mlo, mhi = spread(split[kk]["metric"])
            part = f"metric {mt:.3f} [{mlo:.3f}, {mhi:.3f}] + tail (K copies to the host, float64 on the CPU) {tt:.3f} [{tlo:.3f}, {thi:.3f}]"
        else:
            part = f"metric {t - tt:.3f} (total - tail) + tail (3 kernels, rgb and logs to the host) {tt:.3f} [{tlo:.3f}, {thi:.3f}]"
        say(f"  ({kk}) {WAY_NAMES[kk]:<26s} {t:9.3f} ms/frame [{lo:.3f}, {hi:.3f}]   = {part}")
    for a, b in (("p", "s"), ("p", "g"), ("s", "g")):
        if a in med and b in med:
            sp = max(med[a][2] - med[a][1], med[b][2] - med[b][1])
            d = med[a][0] - med[b][0]
            verdict = f"({b}) faster, beyond the spread" if d > sp else f"({b}) slower, beyond the spread" if -d > sp else "within the spread"
            say(f"  ({a}) / ({b}) = {med[a][0] / med[b][0]:.3f}   margin ({a}) - ({b}) = {d:+.3f} ms against a spread (largest "
                f"max - min) of {sp:.3f} ms: {verdict}")
    if "p" in out:
        for kk in ("s", "g"):
            if kk in out:
                delta = (out[kk][0].int() - out["p"][0].int()).abs()
                logs = max(abs(a - b) / max(abs(b), 1e-300) for a, b in zip(out[kk][1], out["p"][1]))
                say(f"  ({kk}) against (p): {int((delta > 0).sum())} of {delta.numel()} bytes differ, the largest by "
                    f"{int(delta.max())}; extrema {logs:.2e} relative")


def main(argv=None):
    args = parse_args(argv)
    if args.child:
        return run_config(args.child, args.windows, args.steps, args.ways)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/gpu_score_maps_bench.py: {[f'{n} {h}x{w} K={k}' for n, h, w, k in args.config]}; ways {args.ways}; "
        f"{args.windows} alternating windows of {args.steps} frames per way, wall clock with the device drained; ms per "
        "frame, median [min, max] over the windows; bytes and extrema end on the host in every way")
    failed = False
    for cfg in args.config:  # one child per configuration, under its own time limit; nothing follows a failure
        cmd = [sys.executable, os.path.abspath(__file__), "--windows", str(args.windows), "--steps", str(args.steps),
               "--ways", args.ways, "--child", ":".join(str(v) for v in cfg)]
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
