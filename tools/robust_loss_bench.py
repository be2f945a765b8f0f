"""What the robust loss family costs on pose graphs: ms per LM iteration and the assemble / cost stage times on
make_sphere(50, 50) (SE3) and make_manhattan(3500) (SE2), with no loss, Huber through set_structure's huber_delta (both run the
huber_delta kernels), and Cauchy, Andrews and barron1 through apexgpu_pg_set_loss (the general-loss instantiations).  Writes
profiles/robust_loss_bench.txt.  Records what was measured; gates nothing.

With --parent-root DIR (a built checkout of the parent commit) the no-loss and Huber cases are measured on that build too,
alternating: one fresh process per build and round, parent first then this tree, --rounds times, so that drift of the machine
lands on both.  Each process: per case a warm-up LM call, then the wall time of five 12-iteration LM calls from the same start
divided by their iteration counts (median), then stage timing on (which serialises the stream) for one more call: mean ms
per call of the assemble and cost stages.  The file holds the median over the rounds and the spread (min .. max).

    python tools/robust_loss_bench.py [--parent-root DIR] [--rounds 5] [--out profiles/robust_loss_bench.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITERS = 12
LEGACY = ("none", "huber")
GENERAL = ("cauchy", "andrews", "barron1")


def child(root, cases):
    sys.path.insert(0, root)
    import apex_solver_amd as pkg
    from apex_solver_amd.pose_graph import GpuSparseCholeskySolver, PoseGraphProblem
    from apex_solver_amd.solver import LevenbergMarquardtConfig, LinearSolverType

    cfg = (LevenbergMarquardtConfig.new().with_linear_solver_type(LinearSolverType.SparseCholesky).with_max_iterations(ITERS)
           .with_cost_tolerance(0.0).with_parameter_tolerance(0.0).with_gradient_tolerance(0.0))
    out = {}
    for gname, data in (("sphere2500", pkg.synthetic.make_sphere(50, 50)), ("manhattan3500", pkg.synthetic.make_manhattan(3500))):
        for case in cases:
            if case in GENERAL:
                from apex_solver_amd.pose_graph import create_loss_function
                prob = PoseGraphProblem.pose_graph(data, loss=create_loss_function(case))
            else:
                prob = PoseGraphProblem.pose_graph(data, 1.345 if case == "huber" else None)
            prob.add_prior(f"x{int(data.ids[0])}")
            s = GpuSparseCholeskySolver(0).initialize_structure(prob)
            s.set_parameters(data.poses)
            s.lm_optimize(cfg)
            per_iter = []
            for _ in range(5):
                s.set_parameters(data.poses)
                t0 = time.perf_counter()
                res, _, _ = s.lm_optimize(cfg)
                per_iter.append(1e3 * (time.perf_counter() - t0) / max(res.iterations, 1))
            s.set_parameters(data.poses)
            s.enable_stage_timing(True); s.reset_stage_times()
            s.lm_optimize(cfg)
            st = s.stage_times()
            s.enable_stage_timing(False)
            out[f"{gname}/{case}"] = dict(ms=float(np.median(per_iter)), assemble=st["assemble"][0] / max(st["assemble"][1], 1),
                                          cost=st["cost"][0] / max(st["cost"][1], 1), final_cost=res.final_cost)
            s.close()
    print("RESULT " + json.dumps(out))


def run_child(root, cases):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, "--cases", ",".join(cases)], capture_output=True,
                       text=True, timeout=600)
    if p.returncode != 0:
        raise RuntimeError(f"child on {root} failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child"); ap.add_argument("--cases", default="")
    ap.add_argument("--parent-root"); ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "robust_loss_bench.txt"))
    a = ap.parse_args()
    if a.child:
        child(a.child, a.cases.split(","))
        return
    runs = {"parent": [], "this": []}
    for k in range(a.rounds):
        if a.parent_root:
            runs["parent"].append(run_child(os.path.abspath(a.parent_root), LEGACY))
        runs["this"].append(run_child(HERE, LEGACY + GENERAL))
        print(f"round {k + 1}/{a.rounds} done", flush=True)

    def cell(build, key, field):
        v = [r[key][field] for r in runs[build] if key in r]
        return f"{np.median(v):8.4f} ({min(v):.4f} .. {max(v):.4f})" if v else "       -"

    lines = ["robust loss family on pose graphs: 12-iteration LM runs, ms; median over %d alternating rounds (min .. max)" % a.rounds,
             "no loss / huber run the huber_delta kernels; cauchy / andrews / barron1 run the general-loss instantiations", ""]
    for field, title in (("ms", "ms per LM iteration (wall, timing off)"), ("assemble", "assemble stage, ms per call"), ("cost", "cost stage, ms per call")):
        lines.append(title)
        lines.append(f"{'graph/loss':<26}{'parent commit':>34}{'this tree':>34}")
        for key in sorted(runs["this"][0]):
            lines.append(f"{key:<26}{cell('parent', key, field):>34}{cell('this', key, field):>34}")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
