"""What does scoring BOTH metrics of a video cost with one shared VGG pyramid?  (video.score_video(shared_pyramid=True),
pair.score_pair, nqa_adists_dists_forward.)

On one GPU, for each weight set (default synth:1234, synth:1234:1.3, synth:1234:1.6) and each workload -- 64
device-generated 1080p frames in batches of 8 (video.synthetic_frames, the set-up of
profiles/r04_video_both_streams_experiment.txt) and 128 frames of 256 x 256 in batches of 32 -- three ways of scoring
the same video are timed, alternating in ONE process (the order rotated from repeat to repeat) after every shape has
been warmed up:

  (a) video.score_video(ref, render, dists, adists)                        two passes: the behaviour without this feature
  (b) video.score_video(ref, render, dists, adists, shared_pyramid=True)   one pyramid for both metrics
  (c) video.score_video(ref, render, None, adists)                         A-DISTS alone: the floor of (b)

DISTS is the shipped default (precision="auto": what (a) runs it in is printed); the frames live on the device before
the clock starts; every timing is a host clock around a call that ends in the scores' copy to the host plus a device
synchronise.  Printed per mode: ms per batch and pairs/s as median [min, max] over the repeats, then (b) - (c) against
(c)'s own spread, (a) - (b), and max |difference| of both per-frame score columns between (a) and (b).

Usage: python tools/gpu_pair_bench.py [--out FILE] [--repeats N] [--weights W ...] [--workload NAME:H:W:FRAMES:BATCH ...]
Needs a GPU: without one it prints the plan and fails (no fallback).  profiles/pair_scoring.txt is one such report."""
import os; os.environ.setdefault("NQA_VGG16_WEIGHTS", "synth:1234")  # dev tool: stand-in weights, asked for explicitly
import argparse
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])

WEIGHTS = ("synth:1234", "synth:1234:1.3", "synth:1234:1.6")
WORKLOADS = ("1080p:1080:1920:64:8", "256:256:256:128:32")


def parse_workload(s):
    try:
        name, h, w, n, b = s.split(":")
        h, w, n, b = int(h), int(w), int(n), int(b)
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected NAME:H:W:FRAMES:BATCH, got {s!r}")
    if min(h, w, n, b) <= 0:
        raise argparse.ArgumentTypeError(f"sizes must be positive: {s!r}")
    return name, h, w, n, b


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", help="also write the report to this file")
    ap.add_argument("--repeats", type=int, default=6, help="timed repeats of each mode per workload (alternating, the order "
                    "rotated from repeat to repeat)")
    ap.add_argument("--weights", nargs="+", default=list(WEIGHTS), help="VGG weight sets (vgg16_path values)")
    ap.add_argument("--workload", nargs="+", type=parse_workload, default=[parse_workload(s) for s in WORKLOADS],
                    help="NAME:H:W:FRAMES:BATCH")
    args = ap.parse_args(argv)
    if args.repeats < 1:
        ap.error("--repeats must be at least 1")
    return args


def spread(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def main(argv=None):
    args = parse_args(argv)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/gpu_pair_bench.py: weights {args.weights}; workloads "
        f"{[f'{n} {h}x{w}, {f} frames in batches of {b}' for n, h, w, f, b in args.workload]}; {args.repeats} alternating repeats")
    if not torch.cuda.is_available():
        raise SystemExit("gpu_pair_bench: no GPU -- this tool measures on the device and has no CPU path")
    from nerf_qa_amd import video
    from nerf_qa_amd.ADISTS import ADISTS
    from nerf_qa_amd.DISTS_pytorch import DISTS
    dev = torch.device("cuda:0")
    say(f"# {torch.cuda.get_device_name(dev)}; median [min, max] over the repeats; times are whole score_video calls "
        "(frames on the device beforehand, scores copied to the host, device synchronised)")
    for wname in args.weights:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            dists = DISTS(vgg16_path=wname).to(dev).eval()
            adists = ADISTS(vgg16_path=wname).to(dev).eval()
        for name, h, w, n, batch in args.workload:
            ref, ren = video.synthetic_frames(range(n), h, w, dev)
            modes = {
                "a two passes": lambda: video.score_video(ref, ren, dists, adists, batch_size=batch, return_frame_scores=True),
                "b shared pyramid": lambda: video.score_video(ref, ren, dists, adists, batch_size=batch,
                                                              return_frame_scores=True, shared_pyramid=True),
                "c A-DISTS alone": lambda: video.score_video(ref, ren, None, adists, batch_size=batch, return_frame_scores=True),
            }
            out = {}
            for _ in range(2):  # warm-up of every shape (the last batch included): calibration, workspaces, code objects
                for k, fn in modes.items():
                    out[k] = fn()
            torch.cuda.synchronize(dev)
            times = {k: [] for k in modes}
            order = list(modes.items())
            for r in range(args.repeats):
                for k, fn in order[r % 3:] + order[:r % 3]:  # (rotated: no mode always runs behind the same other one)
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize(dev)
                    times[k].append(time.perf_counter() - t0)
            nb = -(-n // batch)
            say(f"\n{wname}  {name}: {n} frames of {h}x{w} in {nb} batches of {batch}; DISTS auto -> "
                f"{dists.precision_for(h, w, dev)} in (a), pair precision {adists.precision_for(h, w)} in (b)")
            med = {}
            for k, ts in times.items():
                m, lo, hi = spread(ts)
                med[k] = (m, lo, hi)
                say(f"  ({k[0]}) {k[2:]:16s} {1e3 * m / nb:9.3f} ms/batch [{1e3 * lo / nb:.3f}, {1e3 * hi / nb:.3f}]   "
                    f"{n / m:9.1f} pairs/s [{n / hi:.1f}, {n / lo:.1f}]")
            (a, _, _), (b, _, _), (c, clo, chi) = med["a two passes"], med["b shared pyramid"], med["c A-DISTS alone"]
            say(f"  (b) - (c) = {1e3 * (b - c) / nb:+.3f} ms/batch; (c)'s own spread max - min = {1e3 * (chi - clo) / nb:.3f} ms/batch"
                f"   (a) - (b) = {1e3 * (a - b) / nb:+.3f} ms/batch   (a) / (b) = {a / b:.3f}")
            fa, fb = out["a two passes"]["_frame_scores"], out["b shared pyramid"]["_frame_scores"]
            say(f"  max |(a) - (b)| per frame: A-DISTS {np.abs(fa['A-DISTS'] - fb['A-DISTS']).max():.3e}   "
                f"DISTS {np.abs(fa['DISTS'] - fb['DISTS']).max():.3e}")
            del ref, ren
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
