"""Levenberg-Marquardt, Gauss-Newton and Dog-Leg on pose graphs, measured side by side in one process: make_sphere(50, 50)
(2500 SE3 vertices) and make_manhattan(3500) (SE2), each with a prior on the first vertex as its gauge.  Writes
profiles/trust_region_bench.txt.  Records what was measured; gates nothing.

Whole loops: the wall time of one optimize call, which ends in a device synchronise, divided by its iteration count; the median
over five calls from the same start after a warm-up call (as tools/pose_graph2d_bench.py).  The LM figure is the yardstick: its
loop and kernels are what they were before Gauss-Newton and Dog-Leg existed.

Single Dog-Leg steps, fresh and reused apart: the wall time of apexgpu_pg_dogleg_step + eval_step + discard_step, each call
ending in its one host wait, median over 20 calls after two warm-up calls; fresh steps at the default radius and mu, reused
steps halving the radius each time from a fresh solve (every fifth call is that fresh solve and is not counted).  One LM step
(solve_augmented + step_stats + eval_step + discard_step) is timed the same way beside them.  Stage times: mean ms per call
with stage timing on, which serialises the stream, for 10 steps of each kind; a stage that never ran shows 0 calls.

    python tools/trust_region_bench.py [--out profiles/trust_region_bench.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import apex_solver_amd as pkg                                                                                   # noqa: E402
from apex_solver_amd.pose_graph import DogLegConfig, GaussNewtonConfig, GpuSparseCholeskySolver, PoseGraphProblem  # noqa: E402
from apex_solver_amd.solver import LevenbergMarquardtConfig, LinearSolverType                                  # noqa: E402

ITERS = 12


def loops(s, data):
    zero = dict(cost_tolerance=0.0, parameter_tolerance=0.0, gradient_tolerance=0.0)
    lm = (LevenbergMarquardtConfig.new().with_linear_solver_type(LinearSolverType.SparseCholesky).with_max_iterations(ITERS)
          .with_cost_tolerance(0.0).with_parameter_tolerance(0.0).with_gradient_tolerance(0.0))
    runs = (("LM", lambda: s.lm_optimize(lm)), ("GN", lambda: s.gn_optimize(GaussNewtonConfig(max_iterations=ITERS, **zero))),
            ("Dog-Leg", lambda: s.dogleg_optimize(DogLegConfig(max_iterations=ITERS, **zero))))
    out = {}
    for name, call in runs:
        s.set_parameters(data.poses)
        call()                                               # warm-up (graph capture, first-use allocations)
        per_iter = []
        for _ in range(5):
            s.set_parameters(data.poses)
            t0 = time.perf_counter()
            res, hist, _ = call()
            per_iter.append(1e3 * (time.perf_counter() - t0) / max(res.iterations, 1))
        reused = int(hist[:, 11].sum()) if name == "Dog-Leg" else 0
        out[name] = dict(ms=float(np.median(per_iter)), iterations=res.iterations, status=res.status, reused=reused,
                         cost=(res.initial_cost, res.final_cost))
    return out


def steps(s, data, timing):
    """ms per step (timing off) or the stage table (timing on) of LM, fresh and reused Dog-Leg steps"""
    cfg = DogLegConfig()
    n = 10 if timing else 20

    def lm_step():
        s.solve_augmented_equation(1e-3, want_step=False); s.step_stats(); s.eval_step(); s.discard_step()

    def fresh_step():
        s.dogleg_step(cfg.initial_mu, cfg.trust_region_radius); s.eval_step(); s.discard_step()

    out = {}
    for name, body in (("LM step", lm_step), ("Dog-Leg fresh", fresh_step)):
        s.set_parameters(data.poses)
        body(); body()
        s.reset_stage_times()
        t = []
        for _ in range(n):
            t0 = time.perf_counter(); body(); t.append(1e3 * (time.perf_counter() - t0))
        out[name] = s.stage_times() if timing else float(np.median(t))
    s.set_parameters(data.poses)
    t, radius = [], cfg.trust_region_radius
    first = True
    while len(t) < n:
        fresh_step(); radius = cfg.trust_region_radius            # the solve the next reused steps rebuild from
        if first:
            s.reset_stage_times(); first = False
        before = s.stage_times()
        for _ in range(4):
            radius *= 0.5
            t0 = time.perf_counter()
            s.dogleg_step(cfg.initial_mu, radius, reuse=True); s.eval_step(); s.discard_step()
            t.append(1e3 * (time.perf_counter() - t0))
        after = s.stage_times()
        if timing:   # the reused steps' share: totals after minus before (times() gives mean ms per call and the call count)
            acc = out.setdefault("Dog-Leg reused", {k: [0.0, 0] for k in after})
            for k in after:
                acc[k][0] += after[k][0] * after[k][1] - before[k][0] * before[k][1]
                acc[k][1] += after[k][1] - before[k][1]
    if timing:
        out["Dog-Leg reused"] = {k: (v[0] / max(v[1], 1), v[1]) for k, v in out["Dog-Leg reused"].items()}
    else:
        out["Dog-Leg reused"] = float(np.median(t[:n]))
    return out


def one(name, data):
    prob = PoseGraphProblem(data).add_prior(f"x{int(data.ids[0])}")
    s = GpuSparseCholeskySolver(0).initialize_structure(prob)
    s.set_parameters(data.poses)
    r = dict(name=name, n_v=data.n_v, n_e=data.n_e, loops=loops(s, data))
    s.apply_column_scaling(None)
    r["steps"] = steps(s, data, False)
    s.enable_stage_timing(True)
    r["stages"] = steps(s, data, True)
    s.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trust_region_bench.txt"))
    a = ap.parse_args()
    rows = [one("SE3 make_sphere(50, 50)", pkg.synthetic.make_sphere(50, 50)), one("SE2 make_manhattan(3500)", pkg.synthetic.make_manhattan(3500))]
    lines = ["LM, Gauss-Newton and Dog-Leg on one MI355X: tools/trust_region_bench.py",
             f"(loops: median of 5 calls of up to {ITERS} iterations, wall time / iterations, after a warm-up call; steps: median wall time of",
             " step + eval_step + discard_step over 20 calls, unscaled variables; stages: mean ms per call with stage timing on, (calls) beside it)", ""]
    for r in rows:
        lines.append(f"{r['name']}: {r['n_v']} vertices, {r['n_e']} edges, prior gauge")
        for k, v in r["loops"].items():
            extra = f", {v['reused']} reused" if k == "Dog-Leg" else ""
            lines.append(f"    {k:8s} loop  {v['ms']:.3f} ms / iteration ({v['iterations']} iterations, status {v['status']}{extra}, cost {v['cost'][0]:.4g} -> {v['cost'][1]:.4g})")
        for k, v in r["steps"].items():
            lines.append(f"    {k:15s} {v:.3f} ms / step")
        for k, st in r["stages"].items():
            lines.append(f"    stages of {k}: " + ", ".join(f"{n} {ms:.3f} ({c})" for n, (ms, c) in st.items()))
        lines.append("")
    txt = "\n".join(lines)
    print(txt)
    with open(a.out, "w") as f:
        f.write(txt)


if __name__ == "__main__":
    main()
