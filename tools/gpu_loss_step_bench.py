"""What one optimisation step on DISTS costs: forward + backward of `DISTS(x, y, require_grad=True, batch_average=True)`
with precision="f32s" on the stand-in weights, at 256 x 256 B=4, 256 x 256 B=32 and 1080 x 1920 B=1, for

  (a) the first form of the backward (autograd.dists_backward(..., host_scaled=True)): both images through the chain,
      the statistics' gradient in torch, the renormalisation exponent read back to the host before every layer;
  (b) the loss path with a gradient on both images (csrc/nqa_loss_backward.hip, pyramid_backward_device);
  (c) the loss path with a gradient on x only (y: taps for the statistics, nothing else).

Step times from device events after warm-up: median [min, max] of REPS windows of ITERS steps.  The forward is the same
fused f32s forward in all three.  Also printed: the forward alone, the host's wall time to ENQUEUE a step (equal to the
step time when the host waits for the device inside it, a fraction of it when it does not), and the peak device memory.

With --target the report is another one: the existing one-sided step with x FIXED and the gradient on y (the training use:
a render y against a ground-truth frame x) against the step on a prepared target (DISTS.prepare_target once, then
forward_target(target, y, require_grad=True, batch_average=True) per step: one kept pyramid of y, nothing of x), on the same
pairs in the same process, with the time of prepare_target itself.

--grad-precision f16 (with --target) builds the module with grad_precision="f16": the same steps with the half gradient
chain, to be set beside a run without it; --shape HxWxB (with --target) runs that one shape, so that every shape can have a
process of its own; --step c (with --target) builds the module with target_step="c", whose target step is the library's
two step calls on one state tensor (autograd.DistsTargetStep) instead of the launches issued from autograd.py: the same
report, to be set beside a run without it (profiles/target_step_c.txt).

Usage: python tools/gpu_loss_step_bench.py [OUT] [--target [--grad-precision f16] [--shape HxWxB] [--step c]]  -- prints the report,
and also writes it to OUT when given (profiles/loss_step_bench.txt holds such reports; a --target report is APPENDED to OUT)."""
import os; os.environ.setdefault("NQA_VGG16_WEIGHTS", "synth:1234")  # dev tool: stand-in weights, asked for explicitly
import subprocess
import sys
import time
import warnings

import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from nerf_qa_amd import autograd, build, ops, synth  # noqa: E402
from nerf_qa_amd.DISTS_pytorch import DISTS  # noqa: E402

WARMUP, ITERS, REPS = 3, 10, 5
SHAPES = ((256, 256, 4), (256, 256, 32), (1080, 1920, 1))


class FirstFormSimilarities(torch.autograd.Function):
    """DistsSimilarities with the backward it had before the loss path: the baseline."""

    @staticmethod
    def forward(ctx, x, y, module):
        s1, s2 = ops.dists_forward(x, y, module._packed_weights(x.device, "f32s"), "f32s", module._ws)
        ctx.module = module
        ctx.save_for_backward(x, y)
        return s1, s2

    @staticmethod
    def backward(ctx, g1, g2):
        x, y = ctx.saved_tensors
        gx, gy = autograd.dists_backward(ctx.module, x, y, g1.contiguous(), g2.contiguous(), need=ctx.needs_input_grad[:2],
                                         host_scaled=True)
        return gx, gy, None


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    out, wall = [], []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        for _ in range(ITERS):
            fn()
        b.record()
        wall.append((time.perf_counter() - t0) * 1e3 / ITERS)  # host time to ENQUEUE a step (includes any host wait inside it)
        b.synchronize()
        out.append(a.elapsed_time(b) / ITERS)
    out.sort()
    wall.sort()
    return out[len(out) // 2], out[0], out[-1], wall[len(wall) // 2]


def commit():
    try:
        root = __file__.rsplit("/", 2)[0]
        rev = subprocess.run(["git", "-C", root, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
        dirty = subprocess.run(["git", "-C", root, "status", "--porcelain"], capture_output=True, text=True).stdout.strip()
        return (rev or "unknown") + ("+changes" if dirty else "")
    except OSError:
        return "unknown"


def target_report(model, dev, say, shapes=SHAPES):
    """The one-sided step (x fixed, gradient on y) against the step on a prepared target, same pairs, one process."""
    for h, w, b in shapes:
        xn, yn = synth.frame_batch(list(range(100, 100 + b)), h, w)
        x0, y0 = torch.from_numpy(xn).to(dev), torch.from_numpy(yn).to(dev)
        target = model.prepare_target(x0)

        def step():
            y = y0.detach().requires_grad_()
            model(x0, y, require_grad=True, batch_average=True).backward()
            return y.grad

        def target_step():
            y = y0.detach().requires_grad_()
            model.forward_target(target, y, require_grad=True, batch_average=True).backward()
            return y.grad

        say(f"\n{h}x{w} B={b}")
        res = {}
        for name, fn in (("one-sided step, grad on y only", step), ("target step,    grad on y only", target_step),
                         ("prepare_target(x)", lambda: model.prepare_target(x0))):
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats(dev)
            res[name] = timed(fn)
            m, lo, hi, wall = res[name]
            say(f"  {name:30s} {m:9.3f} ms  [{lo:.3f}, {hi:.3f}]   enqueue {wall:8.3f} ms   peak memory "
                f"{torch.cuda.max_memory_allocated(dev) / 2 ** 30:6.2f} GiB")
        o, t = res["one-sided step, grad on y only"], res["target step,    grad on y only"]
        gain, spread = o[0] - t[0], (o[2] - o[1]) + (t[2] - t[1])
        say(f"  target / one-sided: {t[0] / o[0]:.3f} (saves {gain:.3f} ms a step; the two runs' min-to-max spreads add up to "
            f"{spread:.3f} ms: {'a gain beyond spread' if gain > spread else 'NO gain beyond spread'}); the target holds "
            f"{target.nbytes / 2 ** 20:.1f} MiB")
        say(f"  y.grad bit-identical: {bool(torch.equal(step().view(torch.int32), target_step().view(torch.int32)))}")
        del x0, y0, target
        torch.cuda.empty_cache()


def main():
    flags = sys.argv[1:]
    valued = {flags[i + 1] for i, a in enumerate(flags[:-1]) if a in ("--grad-precision", "--shape", "--step")}
    args = [a for a in flags if not a.startswith("--") and a not in valued]
    with_target = "--target" in flags
    grad_precision = flags[flags.index("--grad-precision") + 1] if "--grad-precision" in flags else None
    shapes = (tuple(int(v) for v in flags[flags.index("--shape") + 1].split("x")),) if "--shape" in flags else SHAPES
    target_step = flags[flags.index("--step") + 1] if "--step" in flags else None
    dev = torch.device("cuda:0")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = DISTS(precision="f32s", **({"grad_precision": grad_precision} if grad_precision else {}),
                      **({"target_step": target_step} if target_step else {})).to(dev).eval()
    lines = [f"# tools/gpu_loss_step_bench.py  ({torch.cuda.get_device_name(dev)}; torch {torch.__version__}; commit {commit()}; "
             f"HIP sources {build.source_hash()})",
             f"# forward + backward of DISTS(x, y, require_grad=True, batch_average=True), precision f32s, stand-in weights;",
             f"# device events, median [min, max] of {REPS} windows of {ITERS} steps after {WARMUP} warm-up steps; "
             f"'enqueue': host wall time per step until the last launch is issued"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if with_target:
        lines[1] = ("# --target: DISTS(x, y, require_grad=True, batch_average=True) with x fixed against forward_target on a "
                    f"prepared target, precision f32s, gradient chain {model.grad_precision}, target step issued from "
                    f"{'the library (two calls)' if model.target_step == 'c' else 'Python'}, stand-in weights;")
        target_report(model, dev, say, shapes)
    for h, w, b in () if with_target else SHAPES:
        xn, yn = synth.frame_batch(list(range(100, 100 + b)), h, w)
        x0, y0 = torch.from_numpy(xn).to(dev), torch.from_numpy(yn).to(dev)

        def step(first_form, both):
            x = x0.detach().requires_grad_()
            y = y0.detach().requires_grad_() if both else y0
            if first_form:
                loss = model._weighted(*FirstFormSimilarities.apply(x, y, model), True)
            else:
                loss = model(x, y, require_grad=True, batch_average=True)
            loss.backward()
            return x.grad

        def fwd():
            with torch.no_grad():
                return model(x0, y0, batch_average=True)

        say(f"\n{h}x{w} B={b}")
        res = {}
        for name, fn in (("forward alone (no grad)", fwd),
                         ("first form, grad on x and y", lambda: step(True, True)),
                         ("first form, grad on x only", lambda: step(True, False)),
                         ("loss path,  grad on x and y", lambda: step(False, True)),
                         ("loss path,  grad on x only", lambda: step(False, False))):
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats(dev)
            res[name] = timed(fn)
            m, lo, hi, wall = res[name]
            say(f"  {name:30s} {m:9.3f} ms  [{lo:.3f}, {hi:.3f}]   enqueue {wall:8.3f} ms   peak memory "
                f"{torch.cuda.max_memory_allocated(dev) / 2 ** 30:6.2f} GiB")
        p2, n2, n1 = (res[k][0] for k in ("first form, grad on x and y", "loss path,  grad on x and y", "loss path,  grad on x only"))
        say(f"  loss path / first form (x and y): {n2 / p2:.3f};  x only / x and y (loss path): {n1 / n2:.3f};  "
            f"x only (loss path) / first form: {n1 / p2:.3f}")
        ga, gb = step(True, True).clone(), step(False, True).clone()
        say(f"  max |g_loss_path - g_first_form| / max |g_first_form| on x: {((ga - gb).abs().max() / ga.abs().max()).item():.2e}")
        del x0, y0
        torch.cuda.empty_cache()
    if args:
        out = args[0]
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a" if with_target else "w") as f:
            f.write(("\n" if with_target else "") + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
