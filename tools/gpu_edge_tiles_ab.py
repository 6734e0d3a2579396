"""Same-box A/B of the implicit GEMM's mixed grid (16-wide tiles down a right edge that fills at most half a 32-wide tile,
nqa_conv.hip conv3x3_igemm_mixed_kernel) against the plain grid (nqa_set_conv_variant + 256), GPU box: `python bench.py
<args>` as it stands, one fresh process per run, the arms taken in turn so that clock drift hits all of them; optionally a
third arm on another build of the library (--parent-lib: the parent commit's, loaded through NQA_LIB).
usage: python tools/gpu_edge_tiles_ab.py [--runs 5] [--parent-lib PATH] [-- bench.py arguments]
       python tools/gpu_edge_tiles_ab.py --child VARIANT [bench.py arguments]   (what each run executes)"""
import json
import os
import runpy
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")

if len(sys.argv) > 2 and sys.argv[1] == "--child":  # bench.py itself, with the calling (main) thread's variant set first
    sys.path.insert(0, ROOT)
    from nerf_qa_amd import ops
    ops.set_conv_variant(int(sys.argv[2]))
    sys.argv = [BENCH] + sys.argv[3:]
    runpy.run_path(BENCH, run_name="__main__")
    sys.exit(0)

args = sys.argv[1:]
bench_args = args[args.index("--") + 1:] if "--" in args else []
args = args[:args.index("--")] if "--" in args else args
runs = int(args[args.index("--runs") + 1]) if "--runs" in args else 5
parent = args[args.index("--parent-lib") + 1] if "--parent-lib" in args else None
ARMS = [("plain grid (+256)", 1 + 256, None), ("mixed grid (default)", 1, None)]
if parent:
    ARMS.insert(0, ("parent build      ", 1, parent))
res = {name: [] for name, _, _ in ARMS}
for r in range(runs):
    for name, variant, lib in (ARMS if r % 2 == 0 else ARMS[::-1]):
        env = dict(os.environ)
        if lib:
            env["NQA_LIB"] = lib
        p = subprocess.run([sys.executable, __file__, "--child", str(variant), *bench_args], env=env, cwd=ROOT,
                           stdout=subprocess.PIPE, text=True, timeout=600)
        if p.returncode != 0:
            sys.exit(f"{name}: bench.py exited with {p.returncode}")
        line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
        res[name].append((line["ms_per_step"], line["value"]))
        print(f"{name}: step {line['ms_per_step']:7.3f} ms  {line['value']:.1f} {line['unit']}", flush=True)
print(f"bench.py {' '.join(bench_args) or '(default workload)'}, {runs} runs per arm, interleaved")
med = lambda name: sorted(t[0] for t in res[name])[len(res[name]) // 2]  # noqa: E731
base = ARMS[0][0]
for name, _, _ in ARMS:
    ts = [t[0] for t in res[name]]
    print(f"median {name}: step {med(name):.3f} ms, spread {max(ts) - min(ts):.3f} ms ({min(ts):.3f} .. {max(ts):.3f}); "
          f"{(med(base) / med(name) - 1) * 100:+.2f} % vs {base.strip()}")
