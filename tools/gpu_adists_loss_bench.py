"""What one optimisation step on A-DISTS costs, and what the HIP windowed moments (csrc/nqa_window_moments.hip) change:
forward + backward of `ADISTS(x, y)` (as_loss=True) on the stand-in weights at 256 x 256 B=8 and 1080 x 1920 B=1, with a
gradient on y only and on both images, run two ways in one process:

  slices    head.adists_d(..., window_impl="slices"): every window mean as 2 x 21 shifted-slice multiply-adds in torch
            (the head's arithmetic before the kernels existed);
  default   the window means from autograd.WindowMoments (one HIP launch forward, one backward, per stage and use).

The same split for the head alone on fixed taps (no pyramid, no conv backward), and the two kernels' own times on the
largest windowed stage (relu1_2) with their fraction of the HBM stream figure of profiles/r04_stream_bw.txt and of the
non-packed fp32 vector rate (210 multiply-adds per value pair forward: 5 moments x 42 taps).

The loss step with the gradient on y only has a third row:

  hip       ADISTS(loss_head="auto"): autograd.AdistsLossY, the one-sided backward of csrc/nqa_adists_backward.hip -- no
            torch head, no autograd graph over maps.  (slices and default force loss_head="torch", the head they measure.)

Times from device events after warm-up: median [min, max] of REPS windows of ITERS steps.

Usage: python tools/gpu_adists_loss_bench.py [OUT] [--loss-y-only | --target]  -- prints the report, and also writes it
to OUT when given (profiles/adists_loss_step_bench.txt holds such reports).  --loss-y-only: only the loss step with the
gradient on y, default against hip (a minute instead of the whole report; also what a baseline tree is measured with).
--target: only the hip loss step with the gradient on y against the step on a prepared target (ADISTS.prepare_target
once, then forward_target(target, y) per step: one kept pyramid of y, nothing of x's), same pairs, one process, with the
time of prepare_target itself; that report is APPENDED to OUT.  With --target, --grad-precision f16 builds the module with
grad_precision="f16" (the half gradient chain, to be set beside a run without it) and --shape HxWxB runs that one shape,
so that every shape can have a process of its own.

--window N builds the module with window_size=N (3..63; default 21) for --loss-y-only, --target and --kernels.  At N other
than 21 the loss step's `default` row is adists(x, y) as loss_head="auto" runs it -- the torch head on shifted slices --
and the hip row is replaced by

  hip-n     ADISTS(window_size=N, loss_head="hip"): the one-sided HIP backward on the generic window-moments kernels
            (csrc/nqa_window_moments_n.hip), and with --target the prepared-target step under the same head.

--arm default|hip-n runs only that row of --loss-y-only (one process per arm; a tree from before loss_head="hip" has the
default row only), --shape HxWxB applies to --loss-y-only and --kernels too, and --kernels times only the two
window-moments kernels on relu1_2 at the window.  With --window every report is APPENDED to OUT."""
import os; os.environ.setdefault("NQA_VGG16_WEIGHTS", "synth:1234")  # dev tool: stand-in weights, asked for explicitly
import functools
import re
import subprocess
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nerf_qa_amd import autograd, build, ops, synth  # noqa: E402
from nerf_qa_amd.ADISTS import ADISTS, head  # noqa: E402

HIP_HEAD = hasattr(autograd, "AdistsLossY")  # (False on a tree from before the one-sided backward: the baseline's rows only)
try:
    from nerf_qa_amd.ADISTS.ADISTS import LOSS_HEADS
except ImportError:
    LOSS_HEADS = ()
HIP_N = "hip" in LOSS_HEADS  # (False on a tree from before loss_head="hip": the default row only)

WARMUP, ITERS, REPS = 2, 10, 5
SHAPES = ((256, 256, 8), (1080, 1920, 1))
FMA_PER_S = 256 * 64 * 2.4e9  # 256 CUs x 64 lanes x one non-packed fp32 FMA per lane and clock at 2.4 GHz


def timed(fn):
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


def stream_gbs():
    """The best copy figure of profiles/r04_stream_bw.txt (GB/s)."""
    best = 0.0
    with open(os.path.join(ROOT, "profiles", "r04_stream_bw.txt")) as f:
        for line in f:
            m = re.search(r"^copy .*?([0-9.]+) GB/s", line)
            if m:
                best = max(best, float(m.group(1)))
    return best


def target_report(model, dev, say, shapes=SHAPES):
    """The one-sided hip step (x fixed, gradient on y) against the step on a prepared target, same pairs, one process."""
    model.loss_head = "hip" if HIP_N and model.window_size != 21 else "auto"
    for h, w, b in shapes:
        xn, yn = synth.frame_batch(list(range(100, 100 + b)), h, w)
        x0, y0 = torch.from_numpy(xn).to(dev), torch.from_numpy(yn).to(dev)
        target = model.prepare_target(x0)

        def step():
            y = y0.detach().requires_grad_()
            model(x0, y).backward()
            return y.grad

        def target_step():
            y = y0.detach().requires_grad_()
            model.forward_target(target, y).backward()
            return y.grad

        say(f"\n{h}x{w} B={b}")
        res = {}
        for name, fn in (("loss step, grad on y only, hip", step), ("target step, grad on y only", target_step),
                         ("prepare_target(x)", lambda: model.prepare_target(x0))):
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats(dev)
            res[name] = timed(fn)
            m, lo, hi = res[name]
            say(f"  {name:42s} {m:9.3f} ms  [{lo:.3f}, {hi:.3f}]   peak memory "
                f"{torch.cuda.max_memory_allocated(dev) / 2 ** 30:6.2f} GiB")
        o, t = res["loss step, grad on y only, hip"], res["target step, grad on y only"]
        gain, spread = o[0] - t[0], (o[2] - o[1]) + (t[2] - t[1])
        say(f"  target / one-sided: {t[0] / o[0]:.3f} (saves {gain:.3f} ms a step; the two runs' min-to-max spreads add up to "
            f"{spread:.3f} ms: {'a gain beyond spread' if gain > spread else 'NO gain beyond spread'}); the target holds "
            f"{target.nbytes / 2 ** 20:.1f} MiB")
        say(f"  y.grad bit-identical: {bool(torch.equal(step().view(torch.int32), target_step().view(torch.int32)))}")
        del x0, y0, target
        torch.cuda.empty_cache()


def main():
    flags = sys.argv[1:]
    valued = {flags[i + 1] for i, a in enumerate(flags[:-1]) if a in ("--grad-precision", "--shape", "--window", "--arm")}
    args = [a for a in flags if not a.startswith("--") and a not in valued]
    quick = "--loss-y-only" in flags
    with_target = "--target" in flags
    grad_precision = flags[flags.index("--grad-precision") + 1] if "--grad-precision" in flags else None
    shapes = (tuple(int(v) for v in flags[flags.index("--shape") + 1].split("x")),) if "--shape" in flags else SHAPES
    window = int(flags[flags.index("--window") + 1]) if "--window" in flags else 21
    arm = flags[flags.index("--arm") + 1] if "--arm" in flags else None
    kernels_only = "--kernels" in flags
    quick = quick or kernels_only
    hip_row = "hip" if window == 21 else "hip-n"
    kw = ({"grad_precision": grad_precision} if grad_precision else {})
    if window != 21:
        kw["window_size"] = window
    dev = torch.device("cuda:0")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = ADISTS(**kw).to(dev).eval()
    stream = stream_gbs()
    lines = [f"# tools/gpu_adists_loss_bench.py  ({torch.cuda.get_device_name(dev)}; torch {torch.__version__}; commit {commit()}; "
             f"HIP sources {build.source_hash()})",
             "# forward + backward of ADISTS(x, y) (as_loss=True), stand-in weights; device events, median [min, max] of "
             f"{REPS} windows of {ITERS} steps after {WARMUP} warm-up steps",
             f"# HBM stream figure {stream:.0f} GB/s (profiles/r04_stream_bw.txt); non-packed fp32 vector rate "
             f"{FMA_PER_S / 1e12:.1f} T multiply-adds/s"]
    if "--window" in flags:
        lines.append(f"# --window {window}" + (f" --arm {arm}" if arm else "") + (" --kernels" if kernels_only else ""))

    def say(s):
        print(s, flush=True)
        lines.append(s)

    plain = head.adists_d
    slices = functools.partial(plain, window_impl="slices")
    if with_target:
        lines[1] = (f"# --target: ADISTS(x, y) (as_loss=True, window_size {window}, loss_head "
                    f"{'hip' if HIP_N and window != 21 else 'auto'}) with x fixed against forward_target on a prepared "
                    f"target, gradient chain {model.grad_precision}, stand-in weights; device events, median [min, max] of "
                    f"{REPS} windows of {ITERS} steps after {WARMUP} warm-up steps")
        target_report(model, dev, say, shapes)
    for h, w, b in () if with_target else shapes:
        xn, yn = synth.frame_batch(list(range(100, 100 + b)), h, w)
        x0, y0 = torch.from_numpy(xn).to(dev), torch.from_numpy(yn).to(dev)
        tx = [x0] + model._taps_nograd(x0)
        ty = [y0] + model._taps_nograd(y0)

        def step(both):
            x = x0.detach().requires_grad_() if both else x0
            y = y0.detach().requires_grad_()
            model(x, y).backward()
            return y.grad

        def head_step(both):
            fx = [t.detach().requires_grad_() for t in tx] if both else tx
            fy = [t.detach().requires_grad_() for t in ty]
            (1 - head.adists_d(fx, fy, window).mean()).backward()
            return fy[1].grad

        say(f"\n{h}x{w} B={b}")
        res = {}
        for what, fn in () if kernels_only else (("loss step", step),) if quick else (("loss step", step), ("head alone", head_step)):
            for both in (False,) if quick else (False, True):
                impls = (("default", plain),) if quick else (("slices", slices), ("default", plain))
                if what == "loss step" and not both and HIP_HEAD and (window == 21 or HIP_N):
                    impls += ((hip_row, plain),)  # the one-sided HIP backward (autograd.AdistsLossY): no torch head at all
                if arm:
                    impls = tuple(i for i in impls if i[0] == arm)
                for impl, f in impls:
                    head.adists_d = f  # (ADISTS._loss_with_grad and head_step look it up at call time)
                    # slices / default: the torch head, as before (at a window other than 21 what "auto" runs anyway)
                    model.loss_head = {"hip": "auto", "hip-n": "hip"}.get(impl, "torch")
                    try:
                        torch.cuda.empty_cache()
                        torch.cuda.reset_peak_memory_stats(dev)
                        name = f"{what}, grad on {'x and y' if both else 'y only'}, {impl}"
                        res[what, both, impl] = timed(lambda: fn(both))
                    finally:
                        head.adists_d = plain
                    m, lo, hi = res[what, both, impl]
                    say(f"  {name:42s} {m:9.3f} ms  [{lo:.3f}, {hi:.3f}]   peak memory "
                        f"{torch.cuda.max_memory_allocated(dev) / 2 ** 30:6.2f} GiB")
        if ("loss step", False, hip_row) in res and ("loss step", False, "default") in res:
            d, p = res["loss step", False, "default"], res["loss step", False, hip_row]
            say(f"  loss step, grad on y only: default / {hip_row} = {d[0] / p[0]:.2f} (worst case, slowest hip window against "
                f"fastest default window: {d[1] / p[2]:.2f}; min-to-max spread of the repeats: default "
                f"{(d[2] - d[1]) / d[0] * 100:.1f} %, hip {(p[2] - p[1]) / p[0] * 100:.1f} %)")
        if quick and not kernels_only:
            del x0, y0, tx, ty
            torch.cuda.empty_cache()
            continue
        for what in () if kernels_only else ("loss step", "head alone"):
            for both in (False, True):
                s, d = res[what, both, "slices"], res[what, both, "default"]
                say(f"  {what}, grad on {'x and y' if both else 'y only'}: slices / default = {s[0] / d[0]:.2f} "
                    f"(worst case, slowest default window against fastest slices window: {s[1] / d[2]:.2f}; "
                    f"min-to-max spread of the repeats: slices {(s[2] - s[1]) / s[0] * 100:.1f} %, default {(d[2] - d[1]) / d[0] * 100:.1f} %)")
        head.adists_d = slices
        ga = gb = None
        if not kernels_only:
            ga = head_step(True).clone()
            head.adists_d = plain
            gb = head_step(True).clone()
        head.adists_d = plain
        if not kernels_only:
            say(f"  max |g_default - g_slices| / max |g_slices| on relu1_2 of y (head alone): {((ga - gb).abs().max() / ga.abs().max()).item():.2e}")
        # the kernels alone, on the largest windowed stage
        fx, fy = tx[1], ty[1]
        pb, c, hh, ww = fx.shape
        wkw = {} if window == 21 else {"window": window}  # (a tree from before the keyword takes the default call)
        gs = [torch.randn_like(m) for m in ops.window_moments(fx, fy, **wkw)]
        vals = pb * c * hh * ww
        outs = pb * c * (hh - window + 1) * (ww - window + 1)
        t2 = 2 * window  # multiply-adds per value and moment: n taps down, n across
        for name, fn, nbytes, fma in (
                ("window_moments forward, pair", lambda: ops.window_moments(fx, fy, **wkw), 4 * (2 * vals + 5 * outs), 5 * t2 * outs),
                ("window_moments forward, x only", lambda: ops.window_moments(fx, **wkw), 4 * (vals + 2 * outs), 2 * t2 * outs),
                ("window_moments backward, gx and gy", lambda: ops.window_moments_backward(fx, fy, gs, **wkw), 4 * (4 * vals + 5 * outs), 5 * t2 * vals),
                ("window_moments backward, gy only", lambda: ops.window_moments_backward(fx, fy, gs, (False, True), **wkw),
                 4 * (3 * vals + 3 * outs), 3 * t2 * vals)):
            m, lo, hi = timed(fn)
            say(f"  {name:38s} n={window} on relu1_2 {tuple(fx.shape)}: {m:8.3f} ms  [{lo:.3f}, {hi:.3f}]   {nbytes / m / 1e6:7.0f} GB/s compulsory "
                f"= {nbytes / m / 1e6 / stream * 100:5.1f} % of stream;  {fma / m / 1e9:6.2f} T multiply-adds/s useful "
                f"= {fma / m * 1e3 / FMA_PER_S * 100:5.1f} % of the vector rate")
        del x0, y0, tx, ty, fx, fy, gs
        torch.cuda.empty_cache()
    if args:
        out = args[0]
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        append = with_target or "--window" in flags
        with open(out, "a" if append else "w") as f:
            f.write(("\n" if append else "") + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
