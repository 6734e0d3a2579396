"""`python bench.py --gpus N` as the driver types it: with no launcher in the environment the script
starts torch.distributed.run itself as a child process and relays ONE JSON line.  Exercised on CPU with the
`stub` workload (gloo, no HIP kernel) so the launch, the barrier / max-over-ranks timing and the all-gather of
bench.py itself run at world size 2 without a GPU."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                          timeout=timeout, env=env, cwd=ROOT)


def test_gpus_2_launches_itself():
    r = _run(["--gpus", "2", "--steps", "3", "--warmup", "1", "--workload", "stub"])
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout  # exactly one JSON line, from rank 0
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["warmup"] == 1 and out["scaling"] == "weak"
    assert len(out["per_rank_pairs_per_s"]) == 2 and all(v > 0 for v in out["per_rank_pairs_per_s"])
    assert out["value"] > 0 and out["config"]["workload"] == "stub"


def test_single_rank_stub_and_child_failure_code():
    r = _run(["--steps", "2", "--warmup", "0", "--workload", "stub"])
    assert r.returncode == 0 and json.loads(r.stdout)["n_gpus"] == 1
    # a failing rank's exit code comes back through the launcher (no GPU here: the real workload refuses to start)
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0", "--only", "--no-cpu-baseline"],
             env_extra={"HIP_VISIBLE_DEVICES": "", "ROCR_VISIBLE_DEVICES": ""})
    assert r.returncode != 0 and not r.stdout.strip()


def test_dump_outputs_are_the_last_step_and_repeat(tmp_path):
    """--dump-outputs writes the last timed step's scores (every rank's, in rank order) as float32, and the same
    arguments give the same inputs, hence the same outputs, from run to run; --steps is the number of timed steps."""
    import numpy as np
    got = []
    for run, gpus in (("a", "1"), ("b", "1"), ("c", "2")):
        r = _run(["--gpus", gpus, "--steps", "3", "--warmup", "1", "--workload", "stub",
                  "--dump-outputs", str(tmp_path / run)])
        assert r.returncode == 0, r.stdout + r.stderr
        out = json.loads(r.stdout)
        assert out["steps"] == 3 and out["ms_per_step"] > 0
        got.append(np.load(tmp_path / run / "scores.npy"))
    a, b, c = got
    assert a.dtype == np.float32 and a.shape == (8,) and np.isfinite(a).all()
    assert np.array_equal(a, b)
    assert c.shape == (16,) and np.array_equal(c[:8], a) and not np.array_equal(c[8:], a)  # rank 1 seeds its own frames


def test_steps_must_be_positive():
    r = _run(["--steps", "0", "--workload", "stub"])
    assert r.returncode != 0 and "--steps" in r.stderr


@pytest.mark.gpu
def test_plain_line_is_the_headline_and_dumps_what_forward_returns(tmp_path):
    """A plain run prints the headline fields only (no companions, rooflines or CPU baseline: those are --full), and its
    dump is what DISTS.forward in its default precision returns for the same seeded frames."""
    import numpy as np
    import torch
    r = _run(["--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path)], timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    out = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out, k
    assert out["metric"] == "DISTS frame-pairs/s" and out["steps"] == 2 and out["value"] > 0
    assert abs(out["value"] - 8 * 1e3 / out["ms_per_step"]) < 0.01 * out["value"]
    assert not {"workloads", "roofline", "roofline_hbm", "kernel_ms_per_step", "cpu_baseline"} & set(out)
    got = np.load(tmp_path / "scores.npy")
    assert got.dtype == np.float32 and got.shape == (8,)

    from nerf_qa_amd.DISTS_pytorch import DISTS
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    dev = torch.device("cuda:0")
    model = DISTS(vgg16_path=bench.VGG).to(dev).eval()
    assert model.precision_for(1080, 1920) == out["dtype"]
    x, y = bench.synth_frames(8, 1080, 1920, dev, 1000)
    with torch.no_grad():
        want = model(x, y).cpu().numpy()
    assert np.abs(got - want).max() <= 1e-6, np.abs(got - want).max()


def test_rank_count_mismatch_is_refused():
    r = _run(["--gpus", "4", "--workload", "stub"], env_extra={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE=1" in r.stderr
