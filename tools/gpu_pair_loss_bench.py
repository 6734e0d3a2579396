"""What one optimisation step on `wd * DISTS + wa * A-DISTS` against a prepared target costs, on the stand-in weights in
f32s, at 256 x 256 B=8 and 1080 x 1920 B=1:

  (a) the two modules' own target steps back to back on one y -- DISTS.forward_target(require_grad=True) and
      ADISTS.forward_target, summed and back-propagated: two kept pyramids of y, two backward chains, autograd adds the
      two image gradients;
  (b) pair.forward_target + backward: one kept pyramid, one chain over the sum of the tap gradients.

Step times from device events after warm-up: median [min, max] of REPS windows of ITERS steps, with the peak device
memory.  Each shape runs in a process of its own (a call without --shape starts one child per shape).

Then, with the step's two halves called on this thread (the timing ring is per thread and autograd runs a backward on
its own): the per-class device times of (a) and (b) -- conv, statistics, A-DISTS, the rest -- and the accumulating tap
gradient (nqa_dists_stats_nhwc_grad_y_add) against the same backward with the DISTS tap gradients written to maps of
their own and added by torch.

--baseline-only runs (a) alone: it needs nothing this tool's commit added, so the same file times a checkout of the
parent commit (the parent check of DESIGN.md 4.16: alternate the two in fresh processes and compare the ranges).

--grad-precision f16 builds both modules with grad_precision="f16": the same report with the half gradient chain, to be
set beside a run without it.

Usage: python tools/gpu_pair_loss_bench.py [OUT] [--shape HxWxB] [--baseline-only] [--grad-precision f16]  -- prints the
report and appends it to OUT when given (profiles/pair_loss_step_bench.txt holds such reports)."""
import os; os.environ.setdefault("NQA_VGG16_WEIGHTS", "synth:1234")  # dev tool: stand-in weights, asked for explicitly
import subprocess
import sys
import warnings

SHAPES = ("256x256x8", "1080x1920x1")
WARMUP, ITERS, REPS = 3, 10, 5
WD, WA = 1.0, 1.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(fn):
    import torch
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(ITERS):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / ITERS)
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def commit():
    try:
        rev = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
        dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain"], capture_output=True, text=True).stdout.strip()
        return (rev or "unknown") + ("+changes" if dirty else "")
    except OSError:
        return "unknown"


def classes(ops, torch, fn, steps=ITERS):
    """Per-class (launches, ms) per step of fn() called on this thread, and its device-event time per step."""
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    plain = a.elapsed_time(b) / steps
    ops.timing_enable(True)
    try:
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        kt = ops.timing_collect()
    finally:
        ops.timing_enable(False)
    return {k: (n / steps, ms / steps) for k, (n, ms) in kt.items()}, plain


def class_line(kt):
    conv = kt["conv1_1"][1] + kt["conv_igemm"][1]
    rest = sum(v[1] for k, v in kt.items() if k not in ("conv1_1", "conv_igemm", "stats", "adists"))
    return (f"conv {conv:8.3f} ms   statistics {kt['stats'][1]:7.3f} ms ({kt['stats'][0]:.0f} launches)   A-DISTS "
            f"{kt['adists'][1]:8.3f} ms   other timed classes {rest:7.3f} ms")


def one_shape(shape, baseline_only, say, grad_precision=None):
    import torch
    sys.path.insert(0, ROOT)
    from nerf_qa_amd import autograd, build, ops, synth
    from nerf_qa_amd.ADISTS import ADISTS
    from nerf_qa_amd.DISTS_pytorch import DISTS
    h, w, b = (int(v) for v in shape.split("x"))
    dev = torch.device("cuda:0")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gp = {"grad_precision": grad_precision} if grad_precision else {}
        dm = DISTS(precision="f32s", **gp).to(dev).eval()
        am = ADISTS(loss_head="auto", **gp).to(dev).eval()
    say(f"# tools/gpu_pair_loss_bench.py  ({torch.cuda.get_device_name(dev)}; torch {torch.__version__}; commit {commit()}; "
        f"HIP sources {build.source_hash()})")
    say(f"# L = {WD} * DISTS + {WA} * A-DISTS against a prepared target, f32s, gradient chain "
        f"{getattr(dm, 'grad_precision', 'f32s')}, stand-in weights; device events, median "
        f"[min, max] of {REPS} windows of {ITERS} steps after {WARMUP} warm-up steps")
    xn, yn = synth.frame_batch(list(range(100, 100 + b)), h, w)
    x0, y0 = torch.from_numpy(xn).to(dev), torch.from_numpy(yn).to(dev)
    td, ta = dm.prepare_target(x0), am.prepare_target(x0)

    def separate():
        y = y0.detach().requires_grad_()
        (WD * dm.forward_target(td, y, require_grad=True, batch_average=True) + WA * am.forward_target(ta, y)).backward()
        return y.grad

    def paired():
        from nerf_qa_amd import pair
        y = y0.detach().requires_grad_()
        d, a = pair.forward_target(dm, am, td, y, batch_average=True)
        (WD * d + WA * a).backward()
        return y.grad

    say(f"\n{h}x{w} B={b}")
    res = {}
    for name, fn in (("(a) two target steps, summed", separate),) + (() if baseline_only else (("(b) pair.forward_target", paired),)):
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        res[name[:3]] = timed(fn)
        m, lo, hi = res[name[:3]]
        say(f"  {name:30s} {m:9.3f} ms  [{lo:.3f}, {hi:.3f}]   peak memory {torch.cuda.max_memory_allocated(dev) / 2 ** 30:6.2f} GiB")
    if baseline_only:
        return
    a, p = res["(a)"], res["(b)"]
    gain, spread = a[0] - p[0], (a[2] - a[1]) + (p[2] - p[1])
    say(f"  (b) / (a): {p[0] / a[0]:.3f}; saves {gain:.3f} ms a step; the two runs' min-to-max spreads add up to {spread:.3f} ms: "
        f"{'a gain beyond spread' if gain > spread else 'NO gain beyond spread'}")
    ga, gp = separate(), paired()
    say(f"  max |g_pair - g_separate| / max |g_separate|: {((ga - gp).abs().max() / ga.abs().max()).item():.2e}")

    # ---- where the time goes: the halves on this thread, under the timing ring ----
    g1, g2 = ((-(WD * t / b)).expand(b, -1).contiguous().to(dev) for t in dm._score_weights())
    u = torch.full((b,), -WA / b, device=dev)

    def separate_halves():
        _, _, ds = autograd.dists_target_forward(dm, td, y0)
        _, st = autograd.adists_target_d(am, ta, y0, keep=True)
        return (autograd.dists_target_backward(dm, td, ds, g1, g2)
                + autograd.adists_y_backward(am, ta.x, list(ta.taps), y0, st, u))

    _, _, _, state = autograd.pair_target_forward(am, td, y0)

    def pair_halves():
        _, _, _, st = autograd.pair_target_forward(am, td, y0)
        return autograd.pair_target_backward(am, td, y0, st, g1, g2, u)

    def pair_backward():
        return autograd.pair_target_backward(am, td, y0, state, g1, g2, u)

    def pair_backward_torch_add():
        """pair_target_backward with the DISTS tap gradients in maps of their own, added by torch."""
        pyramid = state.adists.pyramid
        g0, g_taps = autograd._adists_y_tap_grads(am, td.x, list(td.taps), y0, state.adists, u)
        gy0, d_taps = autograd._dists_y_tap_grads(td, pyramid.taps, state.stats, g1, g2)
        for g, d in zip(g_taps, d_taps):
            g.add_(d)
        return autograd.pyramid_backward_device(dm, pyramid.acts, pyramid.taps, pyramid.pooled, g_taps, masked=True) + g0 + gy0

    say("  per step, halves called on one thread (timing ring: per-class device time; the event time beside it):")
    for name, fn in (("(a) separate", separate_halves), ("(b) pair", pair_halves)):
        kt, ms = classes(ops, torch, fn)
        say(f"    {name:14s} {ms:9.3f} ms   {class_line(kt)}")
    say("  the backward alone, DISTS tap gradients accumulated in place against written out and added by torch:")
    same = torch.equal(pair_backward().view(torch.int32), pair_backward_torch_add().view(torch.int32))
    for name, fn in (("accumulating", pair_backward), ("torch add", pair_backward_torch_add)):
        kt, _ = classes(ops, torch, fn)
        m, lo, hi = timed(fn)
        say(f"    {name:14s} {m:9.3f} ms  [{lo:.3f}, {hi:.3f}]   statistics class {kt['stats'][1]:7.3f} ms "
            f"({kt['stats'][0]:.0f} launches)")
    taps = sum(t.numel() for t in td.taps) * 4
    say(f"    bit-identical: {same}; the five taps hold {taps / 2 ** 20:.1f} MiB: the accumulating kernel moves 4 tap volumes "
        f"(x, y, g in, g out: {4 * taps / 2 ** 20:.1f} MiB) where a separate write and add move 3 + 3 ({6 * taps / 2 ** 20:.1f} MiB)")


def main():
    flags = sys.argv[1:]
    grad_precision = flags[flags.index("--grad-precision") + 1] if "--grad-precision" in flags else None
    args = [a for a in flags if not a.startswith("--") and a != grad_precision]
    baseline_only = "--baseline-only" in flags
    shape = flags[flags.index("--shape") + 1] if "--shape" in flags else None
    if shape is None:  # one fresh process per shape
        for s in SHAPES:
            cmd = [sys.executable, os.path.abspath(__file__), *args[:1], "--shape", s] + (["--baseline-only"] if baseline_only else []) \
                + (["--grad-precision", grad_precision] if grad_precision else [])
            if subprocess.run(cmd).returncode:
                sys.exit(1)
        return
    args = [a for a in args if a != shape]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    one_shape(shape, baseline_only, say, grad_precision)
    if args:
        out = args[0]
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
