"""Same-box A/B of two builds of the library, GPU box: `python bench.py <args>` as it stands, one fresh process per run, the
parent build (loaded through NQA_LIB) and this tree's build taken in turn so that clock drift hits both; median and
max - min per arm (the protocol of profiles/edge_tiles_ab_1080p.txt).  A difference counts only if it exceeds twice the
larger spread.
usage: python tools/gpu_lib_ab.py --parent-lib PATH [--runs 5] [-- bench.py arguments]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")

args = sys.argv[1:]
bench_args = args[args.index("--") + 1:] if "--" in args else []
args = args[:args.index("--")] if "--" in args else args
runs = int(args[args.index("--runs") + 1]) if "--runs" in args else 5
parent = os.path.abspath(args[args.index("--parent-lib") + 1])
if not os.path.exists(parent):
    sys.exit(f"no such library: {parent}")
ARMS = [("parent build", parent), ("this build  ", None)]
res = {name: [] for name, _ in ARMS}
for r in range(runs):
    for name, lib in (ARMS if r % 2 == 0 else ARMS[::-1]):
        env = dict(os.environ)
        env.pop("NQA_LIB", None)
        if lib:
            env["NQA_LIB"] = lib
        p = subprocess.run([sys.executable, BENCH, *bench_args], env=env, cwd=ROOT, stdout=subprocess.PIPE, text=True,
                           timeout=600)
        if p.returncode != 0:
            sys.exit(f"{name}: bench.py exited with {p.returncode}")
        line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
        res[name].append(line["ms_per_step"])
        print(f"{name}: step {line['ms_per_step']:7.3f} ms  {line['value']:.1f} {line['unit']}", flush=True)
print(f"bench.py {' '.join(bench_args) or '(default workload)'}, {runs} runs per arm, interleaved")
med = {name: sorted(ts)[len(ts) // 2] for name, ts in res.items()}
spread = {name: max(ts) - min(ts) for name, ts in res.items()}
for name, _ in ARMS:
    ts = res[name]
    print(f"median {name}: step {med[name]:.3f} ms, spread {spread[name]:.3f} ms ({min(ts):.3f} .. {max(ts):.3f})")
diff = med[ARMS[0][0]] - med[ARMS[1][0]]
print(f"parent - this: {diff:+.3f} ms ({(med[ARMS[0][0]] / med[ARMS[1][0]] - 1) * 100:+.2f} %); twice the larger spread "
      f"{2 * max(spread.values()):.3f} ms -> {'counts' if abs(diff) > 2 * max(spread.values()) else 'within the noise'}")
