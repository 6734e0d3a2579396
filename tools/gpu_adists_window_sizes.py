"""A-DISTS `as_loss=False` in f32s by window size (GPU box): device-event times of ADISTS(window_size=n) at 1080p B=8 and
256x256 B=32 for n = 7, 21 on the specialised kernels, 21 forced onto the generic kernels, 33 and 63 -- the table of
DESIGN.md 4.19 and profiles/adists_window_sizes.txt.

    python tools/gpu_adists_window_sizes.py                  # every (shape, window) arm, one process each
    python tools/gpu_adists_window_sizes.py --tree <checkout>   # the default window alone, run on another checkout
                                                                 # (the parent commit, built) for the side-by-side line
    python tools/gpu_adists_window_sizes.py --only-default      # the default window alone on this checkout

Per arm: 3 warm-up calls, then 5 windows of 10 calls, each window bracketed by a pair of device events; the line gives
the median window and [min, max], in ms per call.  Every arm is a fresh child process under its own time limit, and
the run stops at the first arm that fails."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"1080p": (8, 1080, 1920), "256": (32, 256, 256)}
ARMS = (("7", 7, False), ("21", 21, False), ("21-generic", 21, True), ("33", 33, False), ("63", 63, False))
LIMIT = 240  # seconds per arm


def child(tree, shape, window, generic):
    sys.path.insert(0, tree)
    import warnings
    import torch
    from nerf_qa_amd import ops
    from nerf_qa_amd.ADISTS import ADISTS
    dev = torch.device("cuda:0")
    b, h, w = SHAPES[shape]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        kw = {} if window == 21 else {"window_size": window}  # (a checkout from before the keyword worked takes 21 only)
        m = ADISTS(precision="f32s", vgg16_path="synth:1234", **kw).to(dev).eval()
    if generic:
        ops.set_conv_variant(ops.DEFAULT_CONV_VARIANT | ops.CONV_WINDOW_GENERIC)
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.rand(b, 3, h, w, device=dev, generator=g)
    y = (x + 0.1 * torch.randn(b, 3, h, w, device=dev, generator=g)).clamp(0, 1)
    with torch.no_grad():
        for _ in range(3):
            s = m(x, y, as_loss=False)
        torch.cuda.synchronize()
        times = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                s = m(x, y, as_loss=False)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) / 10)
    times.sort()
    print(f"{shape:6s} B={b:<2d} window {window:2d}{' generic' if generic else '        '}  "
          f"{times[2]:9.3f} ms/call  [{times[0]:.3f}, {times[4]:.3f}]  {b / times[2] * 1e3:7.1f} pairs/s  "
          f"mean score {s.mean().item():.6f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT, help="the checkout to import nerf_qa_amd from (default: this one)")
    ap.add_argument("--only-default", action="store_true", help="time window 21 on the specialised kernels only")
    ap.add_argument("--child", nargs=3, metavar=("SHAPE", "WINDOW", "GENERIC"))
    a = ap.parse_args()
    tree = os.path.abspath(a.tree)
    if a.child:
        return child(tree, a.child[0], int(a.child[1]), a.child[2] == "1")
    arms = ARMS if tree == ROOT and not a.only_default else ARMS[1:2]
    print(f"# tree {'(this checkout)' if tree == ROOT else '(--tree: another checkout)'}", flush=True)
    env = dict(os.environ, NQA_VGG16_WEIGHTS="synth:1234")
    for shape in SHAPES:
        for _, window, generic in arms:
            cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--tree", tree, "--child",
                   shape, str(window), "1" if generic else "0"]
            rc = subprocess.run(cmd, env=env).returncode
            if rc != 0:
                print(f"# arm {shape} window {window} ended with status {rc}: stopping", flush=True)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
