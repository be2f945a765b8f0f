"""What the robust loss family costs on bundle adjustment: ms per LM iteration and the stage times of assemble (camera and
landmark reduce), Schur pairs, back-substitution and cost on the ladybug-1723 and venice-1778 synthetic shapes, with no loss
and Huber through set_structure's huber_delta (the huber_delta kernels), and Cauchy, Tukey and barron1 through
apexgpu_set_loss (the general-loss instantiations).  Writes profiles/ba_loss_bench.txt.  Records what was
measured; gates nothing.

With --parent-root DIR (a built checkout of the parent commit) the no-loss and Huber cases are measured on that build too,
alternating: one fresh process per build and round, parent first then this tree, --rounds times, so that drift of the machine
lands on both.  Each process: per case a warm-up LM call, then the wall time of three 8-iteration LM calls from the same start
divided by their iteration counts (median), then stage timing on (which serialises the stream) for one more call: mean ms per
call of each stage.  The file holds the median over the rounds and the spread (min .. max).

    python tools/ba_loss_bench.py [--parent-root DIR] [--rounds 3] [--out profiles/ba_loss_bench.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITERS = 8
LEGACY = ("none", "huber")
GENERAL = ("cauchy", "tukey", "barron1")
SCALES = {"cauchy": 2.0, "tukey": 8.0, "barron1": 2.0}   # pixels: of the size of the shapes' residuals
STAGES = ("cam_reduce", "landmark_reduce", "schur_scatter", "back_substitute", "cost")


def child(root, cases):
    sys.path.insert(0, root)
    import apex_solver_amd as pkg
    from apex_solver_amd.solver import GpuSchurComplementSolver, LevenbergMarquardtConfig, Problem

    cfg = (LevenbergMarquardtConfig.new().with_max_iterations(ITERS).with_cost_tolerance(0.0).with_parameter_tolerance(0.0)
           .with_gradient_tolerance(0.0))
    out = {}
    for shape in ("ladybug-1723", "venice-1778"):
        data = pkg.synthetic.make_named(shape)
        for case in cases:
            if case in GENERAL:
                from apex_solver_amd.loss import create_loss_function
                prob = Problem.bundle_adjustment(data, loss=create_loss_function(case, SCALES[case]))
            else:
                prob = Problem.bundle_adjustment(data, huber_delta=1.0 if case == "huber" else None)
            s = GpuSchurComplementSolver(0).initialize_structure(prob)
            s.set_parameters(data.poses, data.intr, data.points)
            s.lm_optimize(cfg)
            per_iter = []
            for _ in range(3):
                s.set_parameters(data.poses, data.intr, data.points)
                t0 = time.perf_counter()
                res, _, _ = s.lm_optimize(cfg)
                per_iter.append(1e3 * (time.perf_counter() - t0) / max(res.iterations, 1))
            s.set_parameters(data.poses, data.intr, data.points)
            s.enable_stage_timing(True); s.reset_stage_times()
            s.lm_optimize(cfg)
            st = s.stage_times()
            s.enable_stage_timing(False)
            row = dict(ms=float(np.median(per_iter)), final_cost=res.final_cost)
            for name in STAGES:
                row[name] = st[name][0] / max(st[name][1], 1)
            out[f"{shape}/{case}"] = row
            s.close()
    print("RESULT " + json.dumps(out))


def run_child(root, cases):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, "--cases", ",".join(cases)], capture_output=True,
                       text=True, timeout=900)
    if p.returncode != 0:
        raise RuntimeError(f"child on {root} failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child"); ap.add_argument("--cases", default="")
    ap.add_argument("--parent-root"); ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "ba_loss_bench.txt"))
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

    lines = ["robust loss family on bundle adjustment: %d-iteration LM runs, ms; median over %d alternating rounds (min .. max)" % (ITERS, a.rounds),
             "no loss / huber run the huber_delta kernels; cauchy / tukey / barron1 run the general-loss instantiations", ""]
    titles = [("ms", "ms per LM iteration (wall, timing off)")] + [(n, f"{n} stage, ms per call") for n in STAGES]
    for field, title in titles:
        lines.append(title)
        lines.append(f"{'shape/loss':<26}{'parent commit':>34}{'this tree':>34}")
        for key in sorted(runs["this"][0]):
            lines.append(f"{key:<26}{cell('parent', key, field):>34}{cell('this', key, field):>34}")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
