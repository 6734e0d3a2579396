"""forward_from_feats under autograd (the NR models' training loss, model_nr_v8.py:258-265) at the NR batch (B=4,
nerf_qa/settings.py) and at B=32, 256 x 256 taps from forward_once of stand-in pairs:

  (a) this build: DISTS.forward_from_feats -> autograd.FeatsSimilarities (statistics kernel forward, the two launches of
      csrc/nqa_stats_backward.hip backward), the alpha/beta weighted sum in torch;
  (b) the same score written as a plain torch expression (per-tap means, variances, covariance, S1, S2, weighted sum)
      under torch autograd on the same GPU: what a user would otherwise write.

Forward + backward step times from device events after warm-up (median of REPS windows of ITERS steps), both feature
lists carrying a gradient, plus the NR case (one list).  The backward alone (ops.dists_stats_nchw_backward: coefficient
kernel + gradient kernel) is timed the same way and set against its algorithmic bytes: x and y read once, both
gradients written once (16 bytes per element pair; the fp64 partials and coefficients are < 1 % and not counted), over
8 TB/s (spec) and 6.3 TB/s (a measured float4 copy on this GPU).

Usage: python tools/gpu_feats_grad_bench.py [OUT]  -- prints the report, and also writes it to OUT when given
(profiles/feats_grad_bench.txt is one such report)."""
import os; os.environ.setdefault("NQA_VGG16_WEIGHTS", "synth:1234")  # dev tool: stand-in weights, asked for explicitly
import sys
import warnings

import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from nerf_qa_amd import ops, synth  # noqa: E402
from nerf_qa_amd.DISTS_pytorch import DISTS  # noqa: E402

WARMUP, ITERS, REPS = 5, 20, 5
SPEC_TBS, COPY_TBS = 8.0, 6.3
C1 = C2 = 1e-6


def torch_score(f0, f1, alpha, beta, chns):
    """DISTS' score from two feature lists as plain torch operations (DISTS_pt.py:181-208 restated)."""
    w = alpha.sum() + beta.sum()
    d1 = d2 = 0
    o = 0
    for x, y, c in zip(f0, f1, chns):
        mx, my = x.mean([2, 3], keepdim=True), y.mean([2, 3], keepdim=True)
        s1 = (2 * mx * my + C1) / (mx ** 2 + my ** 2 + C1)
        vx, vy = ((x - mx) ** 2).mean([2, 3], keepdim=True), ((y - my) ** 2).mean([2, 3], keepdim=True)
        cov = (x * y).mean([2, 3], keepdim=True) - mx * my
        s2 = (2 * cov + C2) / (vx + vy + C2)
        d1 = d1 + ((alpha[:, o:o + c] / w) * s1).sum(1, keepdim=True)
        d2 = d2 + ((beta[:, o:o + c] / w) * s2).sum(1, keepdim=True)
        o += c
    return 1 - (d1 + d2).flatten()


def timed(fn):
    for _ in range(WARMUP):
        fn()
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


def main():
    dev = torch.device("cuda:0")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = DISTS(precision="f32s").to(dev)
    lines = [f"# tools/gpu_feats_grad_bench.py  ({torch.cuda.get_device_name(dev)}; median [min, max] of {REPS} windows "
             f"of {ITERS} steps after {WARMUP} warm-up steps)"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for b in (4, 32):
        xn, yn = synth.frame_batch(list(range(100, 100 + b)), 256, 256)
        with torch.no_grad():
            f0 = model.forward_once(torch.from_numpy(xn).to(dev))
            f1 = model.forward_once(torch.from_numpy(yn).to(dev))
        f0 = [f.detach().clone().contiguous() for f in f0]
        f1 = [f.detach().clone().contiguous() for f in f1]
        elems = sum(f.numel() for f in f0)  # per list
        a0 = [f.clone().requires_grad_() for f in f0]
        a1 = [f.clone().requires_grad_() for f in f1]
        maps = a0 + a1

        def step(score_fn, lists):
            for t in maps + [model.alpha, model.beta]:
                t.grad = None
            score_fn(*lists).sum().backward()

        hip = lambda p, q: model.forward_from_feats(p, q)
        ref = lambda p, q: torch_score(p, q, model.alpha, model.beta, model.chns)
        say(f"\n256x256 B={b}: {elems // b} floats per image over the six taps")
        res = {}
        for name, fn, lists in (("hip  fwd+bwd, grad on both lists", hip, (a0, a1)),
                                ("torch fwd+bwd, grad on both lists", ref, (a0, a1)),
                                ("hip  fwd+bwd, grad on feats1 only (NR)", hip, (f0, a1)),
                                ("torch fwd+bwd, grad on feats1 only (NR)", ref, (f0, a1))):
            res[name] = timed(lambda: step(fn, lists))
            m, lo, hi = res[name]
            say(f"  {name:42s} {m:8.3f} ms  [{lo:.3f}, {hi:.3f}]")
        say(f"  speed-up (both lists): {res['torch fwd+bwd, grad on both lists'][0] / res['hip  fwd+bwd, grad on both lists'][0]:.2f}x;"
            f"  (NR): {res['torch fwd+bwd, grad on feats1 only (NR)'][0] / res['hip  fwd+bwd, grad on feats1 only (NR)'][0]:.2f}x")
        # the two modes' gradients side by side (the torch expression is float32 autograd: agreement to its rounding)
        step(hip, (a0, a1))
        gh = [t.grad.clone() for t in maps]
        step(ref, (a0, a1))
        rel = max(((g - t.grad).abs().max() / t.grad.abs().max().clamp_min(1e-30)).item() for g, t in zip(gh, maps))
        say(f"  max |g_hip - g_torch| / max |g_torch| over the 12 maps: {rel:.2e}")
        # the backward alone: coefficient + gradient kernels
        with torch.no_grad():
            _, _, scratch = ops.dists_stats_nchw(f0, f1, keep_scratch=True)
            ctot = sum(model.chns)
            g1 = torch.randn(b, ctot, device=dev)
            g2 = torch.randn(b, ctot, device=dev)
            for need0, label, nbytes in (((1,) * 6, "both gradients", 16 * elems), ((0,) * 6, "feats1 gradient", 12 * elems)):
                call = lambda: ops.dists_stats_nchw_backward(f0, f1, scratch, g1, g2, need0, (1,) * 6)
                m, lo, hi = timed(call)
                # device time of the two launches themselves (the library's timing ring brackets each with events)
                ops.timing_collect()
                ops.timing_enable(True)
                for _ in range(ITERS):
                    call()
                n, kms = ops.timing_collect()["stats"]
                ops.timing_enable(False)
                kms /= ITERS
                tbs = nbytes / (kms * 1e-3) / 1e12
                say(f"  backward alone, {label:15s} step {m:7.3f} ms [{lo:.3f}, {hi:.3f}]; kernels {kms:.3f} ms ({n // ITERS} "
                    f"launches)  {nbytes / 1e9:.3f} GB algorithmic -> {tbs:.2f} TB/s = {tbs / SPEC_TBS:.0%} of {SPEC_TBS} (spec), "
                    f"{tbs / COPY_TBS:.0%} of {COPY_TBS} (copy)")
        del a0, a1, maps, f0, f1, scratch
        torch.cuda.empty_cache()
    if len(sys.argv) > 1:
        out = sys.argv[1]
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
