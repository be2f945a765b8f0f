"""What edge information matrices cost on pose graphs (apexgpu_pg_set_information): ms per LM iteration and the
assemble / cost stage times on make_sphere(50, 50) (SE3) and make_manhattan(3500) (SE2) with the handle in three states --
(a) no information (the legacy | general instantiations, the code of a handle that never heard of Omega), (b) Omega = I and
(c) a dense random SPD Omega per edge (both the LossWeighted instantiations) -- each with no loss and with Cauchy.  Writes
profiles/information_bench.txt.  Records what was measured; gates nothing.

With --parent-root DIR (a built checkout of the parent commit) state (a) is measured on that build too, alternating: one fresh
process per build and round, --rounds times, the build that goes first changing from round to round, so that drift of the
machine and the order of the two land on both.  Each
process runs under its own time limit and a failed one ends the run.  Per case: a warm-up LM call, then the wall time of five
12-iteration LM calls from the same start divided by their iteration counts (median), then stage timing on (which serialises
the stream) for one more call: mean ms per call of the assemble and cost stages.  The file holds the median over the rounds
and the spread (min .. max).

    python tools/information_bench.py [--parent-root DIR] [--rounds 5] [--out profiles/information_bench.txt]
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
STATES = ("a-none", "b-identity", "c-random")
LOSSES = ("noloss", "cauchy")


def random_information(n_e, D, seed=11):
    """Q diag(sigma) Q^T per edge, sigma log-uniform in [0.25, 16]"""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n_e, D, D)))
    sigma = np.exp(rng.uniform(np.log(0.25), np.log(16.0), (n_e, D)))
    W = np.einsum("eik,ek,ejk->eij", Q, sigma, Q)
    return 0.5 * (W + W.transpose(0, 2, 1))


def child(root, states):
    sys.path.insert(0, root)
    import apex_solver_amd as pkg
    from apex_solver_amd.pose_graph import GpuSparseCholeskySolver, PoseGraphProblem, create_loss_function
    from apex_solver_amd.solver import LevenbergMarquardtConfig, LinearSolverType

    cfg = (LevenbergMarquardtConfig.new().with_linear_solver_type(LinearSolverType.SparseCholesky).with_max_iterations(ITERS)
           .with_cost_tolerance(0.0).with_parameter_tolerance(0.0).with_gradient_tolerance(0.0))
    out = {}
    for gname, data in (("sphere2500", pkg.synthetic.make_sphere(50, 50)), ("manhattan3500", pkg.synthetic.make_manhattan(3500))):
        D = 3 if data.manifold == "se2" else 6
        for state in states:
            for lname in LOSSES:
                prob = PoseGraphProblem.pose_graph(data, loss=create_loss_function("cauchy") if lname == "cauchy" else None)
                prob.add_prior(f"x{int(data.ids[0])}")
                s = GpuSparseCholeskySolver(0).initialize_structure(prob)
                if state == "b-identity":
                    s.set_information(np.broadcast_to(np.eye(D), (data.n_e, D, D)).copy())
                elif state == "c-random":
                    s.set_information(random_information(data.n_e, D))
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
                out[f"{gname}/{state}/{lname}"] = dict(ms=float(np.median(per_iter)), assemble=st["assemble"][0] / max(st["assemble"][1], 1),
                                                       cost=st["cost"][0] / max(st["cost"][1], 1), final_cost=res.final_cost)
                s.close()
    print("RESULT " + json.dumps(out))


def run_child(root, states):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, "--states", ",".join(states)], capture_output=True,
                       text=True, timeout=300)
    if p.returncode != 0:
        raise RuntimeError(f"child on {root} failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child"); ap.add_argument("--states", default="")
    ap.add_argument("--parent-root"); ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "information_bench.txt"))
    a = ap.parse_args()
    if a.child:
        child(a.child, a.states.split(","))
        return
    runs = {"parent": [], "this": []}
    for k in range(a.rounds):
        order = ("parent", "this") if k % 2 == 0 else ("this", "parent")   # who goes first alternates too
        for build in order:
            if build == "this":
                runs["this"].append(run_child(HERE, STATES))
            elif a.parent_root:
                runs["parent"].append(run_child(os.path.abspath(a.parent_root), STATES[:1]))
        print(f"round {k + 1}/{a.rounds} done", flush=True)

    def cell(build, key, field):
        v = [r[key][field] for r in runs[build] if key in r]
        return f"{np.median(v):8.4f} ({min(v):.4f} .. {max(v):.4f})" if v else "       -"

    lines = ["edge information matrices on pose graphs: 12-iteration LM runs, ms; median over %d alternating rounds (min .. max)" % a.rounds,
             "a-none: no information (legacy | general instantiations); b-identity: Omega = I; c-random: dense random SPD Omega (both LossWeighted)", ""]
    for field, title in (("ms", "ms per LM iteration (wall, timing off)"), ("assemble", "assemble stage, ms per call"), ("cost", "cost stage, ms per call")):
        lines.append(title)
        lines.append(f"{'graph/state/loss':<36}{'parent commit':>34}{'this tree':>34}")
        for key in sorted(runs["this"][0]):
            lines.append(f"{key:<36}{cell('parent', key, field):>34}{cell('this', key, field):>34}")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
