"""SE2 pose-graph measurement: make_manhattan(3500) and make_manhattan(10000) (the city10000 size), and beside each the SE3
make_sphere graph of the same vertex count from the same process.  Per workload: set-up seconds, ms per LM iteration, the
six stage times, and tile rows / tiles / levels from apexgpu_pg_info.  Writes profiles/se2_pose_graph_bench.txt.  Records
what was measured; gates nothing.

ms per LM iteration: apexgpu_pg_lm_optimize keeps no clock per iteration (its history holds costs and damping), so an
iteration is timed as the wall time of one whole call, which ends in a device synchronise, divided by its iteration count
-- accepted and rejected iterations alike (the accepted count is printed beside it) -- and the figure is the median over
five such calls of 12 iterations each from the same start, after a warm-up call.  Stage times come from a sixth call with
stage timing on (mean ms per call of each stage); timing serialises the stream, so they sum to more than the iteration.

    python tools/pose_graph2d_bench.py [--out profiles/se2_pose_graph_bench.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import apex_solver_amd as pkg                                                                   # noqa: E402
from apex_solver_amd.pose_graph import GpuSparseCholeskySolver, PoseGraphProblem               # noqa: E402
from apex_solver_amd.solver import LevenbergMarquardtConfig, LinearSolverType                  # noqa: E402


def one(name, data, iters=12):
    prob = PoseGraphProblem.pose_graph(data)
    t0 = time.perf_counter()
    s = GpuSparseCholeskySolver(0).initialize_structure(prob)
    s.set_parameters(data.poses)
    setup = time.perf_counter() - t0
    cfg = (LevenbergMarquardtConfig.new().with_linear_solver_type(LinearSolverType.SparseCholesky).with_max_iterations(iters)
           .with_cost_tolerance(0.0).with_parameter_tolerance(0.0).with_gradient_tolerance(0.0))
    s.lm_optimize(cfg)                                       # warm-up (graph capture, first-use allocations)
    per_iter = []
    for _ in range(5):                                       # per-iteration wall time of whole runs, untimed stages
        s.set_parameters(data.poses)
        t0 = time.perf_counter()
        res, hist, _ = s.lm_optimize(cfg)
        per_iter.append(1e3 * (time.perf_counter() - t0) / max(res.iterations, 1))
    accepted = int(hist[:, 3].sum())
    s.set_parameters(data.poses)
    s.enable_stage_timing(True); s.reset_stage_times()
    res, hist, _ = s.lm_optimize(cfg)
    st = s.stage_times()
    info = s.info()
    s.close()
    stages = {k: (ms / max(n, 1)) for k, (ms, n) in st.items()}
    return dict(name=name, n_v=data.n_v, n_e=data.n_e, setup_s=setup, ms_per_iter=float(np.median(per_iter)), iterations=res.iterations,
                accepted=accepted, stages=stages, info=info, final_cost=res.final_cost, initial_cost=res.initial_cost)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "se2_pose_graph_bench.txt"))
    a = ap.parse_args()
    rows = []
    for n, rings in ((3500, (50, 70)), (10000, (100, 100))):
        rows.append(one(f"SE2 make_manhattan({n})", pkg.synthetic.make_manhattan(n)))
        rows.append(one(f"SE3 make_sphere({rings[0]}, {rings[1]})", pkg.synthetic.make_sphere(*rings)))
    lines = ["SE2 pose graphs on one MI355X: tools/pose_graph2d_bench.py", "(ms per LM iteration: median of 5 runs of 12 iterations, wall time / iterations, after a warm-up run;",
             " stage times: mean ms per call inside one timed run -- timing serialises the stream, so the stages sum to more than the iteration)", ""]
    for r in rows:
        i = r["info"]
        lines.append(f"{r['name']}: {r['n_v']} vertices, {r['n_e']} edges, set-up {r['setup_s']:.3f} s, {r['ms_per_iter']:.3f} ms / LM iteration "
                     f"({r['iterations']} iterations, {r['accepted']} accepted, cost {r['initial_cost']:.4g} -> {r['final_cost']:.4g})")
        lines.append(f"    tile rows {i['tile_rows']}, tiles {i['tiles']} (of H itself {i['touched_tiles']}), levels {i['etree_levels']}, dof {i['total_dof']}")
        lines.append("    stages (ms / call): " + ", ".join(f"{k} {v:.3f}" for k, v in r["stages"].items()))
    txt = "\n".join(lines) + "\n"
    print(txt)
    with open(a.out, "w") as f:
        f.write(txt)


if __name__ == "__main__":
    main()
