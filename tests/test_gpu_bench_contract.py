"""bench.py's one-line JSON contract on a small workload: the plain line (metric / value / ms_per_step ...) and its outputs
(--dump-outputs), and the --full line (roofline / cpu_baseline ...)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import apex_solver_amd as pkg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PLAIN = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
         "dtype", "data", "config")
REQUIRED = PLAIN + ("roofline", "cpu_baseline")
FULL_ONLY = ("roofline", "cpu_baseline", "factor", "stages_ms_per_step", "other_variants", "fallback_implicit", "other_workloads")


def run(*args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_ba_line():
    out = run("--workload", "ladybug-49", "--steps", "3", "--warmup", "1", "--full")
    for k in REQUIRED:
        assert k in out, k
    assert out["n_gpus"] == 1 and out["steps"] == 3 and out["warmup"] == 1 and out["higher_is_better"] is False
    assert out["dtype"] == "f64" and out["data"] == "synthetic" and out["vs_baseline"] is None and "workload" in out["config"]
    assert out["value"] == pytest.approx(out["ms_per_step"]) and out["value"] > 0
    r = out["roofline"]
    assert r["bound"] in ("hbm", "mfma") and r["peak"] == 8000.0 and r["frac"] == pytest.approx(r["achieved"] / r["peak"])
    c = out["cpu_baseline"]
    assert c["kind"] in ("port", "reference") and c["cores"] >= 1 and c["value"] > 0 and "sample" in c
    assert out["final_cost"] < out["initial_cost"]
    # round 5: the factorisation against ITS roof, the variant that really ran, and the fall-back figure that does not depend
    # on the state of the handle (one PCG iteration x the reference's cap) next to the observed one
    f = out["factor"]
    assert f["bound"] == "mfma" and f["peak"] == 78.6 and f["frac"] == pytest.approx(f["achieved"] / 78.6) and f["flops_per_factorisation"] > 0
    assert out["config"]["variant_used"] == "Sparse" and out["config"]["reason"] == ""
    fb = out["fallback_implicit"]
    assert fb["cap"] == 500 and fb["ms_per_pcg_iter"] > 0 and fb["bound_ms"] >= fb["ms_per_pcg_iter"] * 500 and len(fb["observed_iterations"]) == 2
    assert "other_workloads" not in out          # only the headline line carries them


def test_pose_graph_line():
    out = run("--workload", "sphere2500", "--scale", "0.04", "--steps", "3", "--warmup", "1", "--full")
    for k in REQUIRED:
        assert k in out, k
    assert out["roofline"]["bound"] == "mfma" and out["scaling"] == "weak" and out["final_cost"] < out["initial_cost"]


def test_plain_ba_line_and_its_outputs(tmp_path):
    """A plain run carries the headline and nothing that --full adds; --dump-outputs writes the parameters after the last timed
    step (float64), and a second run with the same arguments starts from the same inputs: its line agrees on the costs."""
    out = run("--workload", "ladybug-49", "--steps", "4", "--warmup", "1", "--dump-outputs", str(tmp_path / "a"))
    for k in PLAIN:
        assert k in out, k
    for k in FULL_ONLY:
        assert k not in out, k
    assert out["steps"] == 4 and out["warmup"] == 1 and out["value"] == pytest.approx(out["ms_per_step"]) and out["value"] > 0
    assert out["final_cost"] < out["initial_cost"]
    d = pkg.synthetic.make_named("ladybug-49")
    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("poses", "intrinsics", "points", "lm_history")}
    assert all(v.dtype == np.float64 for v in a.values())
    assert a["poses"].shape == (d.n_cam, 7) and a["intrinsics"].shape == (d.n_cam, 3) and a["points"].shape == (d.n_pt, 3)
    assert a["lm_history"].shape == (4, 2) and a["lm_history"][-1, 0] == out["final_cost"]
    assert not np.array_equal(a["points"], d.points)   # the steps moved the landmarks
    again = run("--workload", "ladybug-49", "--steps", "4", "--warmup", "1")
    assert again["initial_cost"] == out["initial_cost"]
    assert again["final_cost"] == pytest.approx(out["final_cost"], rel=1e-6)


def test_plain_pose_graph_outputs(tmp_path):
    out = run("--workload", "sphere2500", "--scale", "0.04", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert "roofline" not in out and "cpu_baseline" not in out and out["ms_per_step"] > 0
    poses, hist = np.load(tmp_path / "poses.npy"), np.load(tmp_path / "lm_history.npy")
    assert poses.dtype == np.float64 and poses.shape[1] == 7 and hist.shape == (3, 2) and hist[-1, 0] == out["final_cost"]


def test_two_ranks_fall_back_to_shared_memory_when_rccl_refuses():
    """`--gpus 2` with both ranks on the one GPU of the box (gloo bring-up mode): RCCL refuses the duplicate device, the ranks
    vote, and the run completes over the shared-memory transport -- the line says which transport carried it."""
    env = dict(os.environ, APEX_BENCH_PG="gloo")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--workload", "ladybug-1723", "--scale", "0.25", "--steps", "3",
                        "--warmup", "1", "--no-cpu-baseline", "--no-other-variants"], capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["scaling"] == "strong" and out["final_cost"] < out["initial_cost"]
    assert out["config"]["transport"].startswith("shm (RCCL communicator failed"), out["config"]["transport"]
