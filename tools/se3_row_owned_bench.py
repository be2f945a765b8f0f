#!/usr/bin/env python3
"""A/B of the SE3 pose-graph assembly: the atomic edge scatter (option "row_owned_assembly" 0, the default) against the
row-owned assembly (1), in one process and one visit, the settings interleaved run by run.

  python tools/se3_row_owned_bench.py [--large RINGS PER_RING] [--vgpr "text of the build remarks"] [--out FILE]

Workloads: make_sphere(50, 50) (sphere2500, BASELINE configs[1]) and one larger sphere.  Losses: none, Cauchy, Cauchy with
information matrices -- the three kernel policies.  Per (workload, loss, setting): 5 runs of 12 LM iterations from the same start
with the same damping schedule; reported are the median over the runs of the wall time per iteration (stage timers off) and of
the `assemble` stage per iteration (a second pass with the stage timers on), each with its min-max spread.  Three untimed
iterations precede every handle's first run.  Writes profiles/se3_row_owned_bench.txt."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import apex_solver_amd as pkg  # noqa: E402
from apex_solver_amd.pose_graph import GpuSparseCholeskySolver, PoseGraphProblem, create_loss_function  # noqa: E402

RUNS, ITERS = 5, 12


def information(n_e, seed=11):
    """symmetric positive definite 6 x 6 matrices with eigenvalues in [0.25, 4]"""
    rng = np.random.default_rng(seed)
    out = np.zeros((n_e, 6, 6))
    for e in range(n_e):
        Q, _ = np.linalg.qr(rng.standard_normal((6, 6)))
        W = (Q * np.exp(rng.uniform(np.log(0.25), np.log(4.0), 6))[None, :]) @ Q.T
        out[e] = 0.5 * (W + W.T)
    return out


def run(s, d, timed_stages):
    """ITERS LM iterations from the start; -> (ms per iteration, assemble ms per iteration or None)"""
    s.set_parameters(d.poses)
    lam = 1e-3
    cost = s.compute_cost()
    s.enable_stage_timing(timed_stages)
    s.reset_stage_times()
    t0 = time.perf_counter()
    for _ in range(ITERS):
        s.solve_augmented_equation(lam, want_step=False)
        s.step_stats()
        nc = s.eval_step()
        if cost - nc > 0:
            cost = nc; s.commit_step(); lam = max(lam / 3, 1e-12)
        else:
            s.discard_step(); lam *= 2
    ms = (time.perf_counter() - t0) * 1e3 / ITERS
    asm = None
    if timed_stages:
        t, n = s.stage_times()["assemble"]
        asm = t / max(n, 1)
    s.enable_stage_timing(False)
    return ms, asm, cost


def med(xs):
    return f"{statistics.median(xs):.4f} [{min(xs):.4f} .. {max(xs):.4f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--large", nargs=2, type=int, default=[100, 100])
    ap.add_argument("--vgpr", default="", help="the kernel-resource-usage remarks of the three k_pg6_assemble instantiations, as text")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "se3_row_owned_bench.txt"))
    a = ap.parse_args()
    lines = [f"# SE3 assembly A/B: option row_owned_assembly 0 (atomics) | 1 (row-owned); median [min .. max] over {RUNS} runs of {ITERS} LM iterations, ms",
             f"# registers: {a.vgpr}" if a.vgpr else "# registers: (not passed)"]
    records = []
    for rings, per in ((50, 50), tuple(a.large)):
        d = pkg.synthetic.make_sphere(rings, per)
        W = information(d.n_e)
        for loss_name, kw in (("none", {}), ("cauchy", dict(loss=create_loss_function("cauchy"))),
                              ("cauchy+info", dict(loss=create_loss_function("cauchy"), information=W))):
            prob = PoseGraphProblem.pose_graph(d, **kw)
            handles = {}
            for opt in (0, 1):
                s = GpuSparseCholeskySolver().with_option("row_owned_assembly", opt).initialize_structure(prob)
                s.set_parameters(d.poses)
                for _ in range(3):
                    s.solve_augmented_equation(1e-3, want_step=False); s.eval_step(); s.discard_step()
                handles[opt] = s
            wall = {0: [], 1: []}; asm = {0: [], 1: []}; cost = {}
            for _ in range(RUNS):                       # interleaved: drift of the machine hits both settings alike
                for opt in (0, 1):
                    wall[opt].append(run(handles[opt], d, False)[0])
                for opt in (0, 1):
                    _, t, c = run(handles[opt], d, True)
                    asm[opt].append(t); cost[opt] = c
            for opt in (0, 1):
                handles[opt].close()
                rec = dict(workload=d.name, n_v=d.n_v, n_e=d.n_e, loss=loss_name, row_owned=opt, ms_per_iter=statistics.median(wall[opt]),
                           ms_per_iter_range=[min(wall[opt]), max(wall[opt])], assemble_ms=statistics.median(asm[opt]),
                           assemble_ms_range=[min(asm[opt]), max(asm[opt])], final_cost=cost[opt])
                records.append(rec)
                lines.append(f"{d.name:>14} n_v {d.n_v:6d} n_e {d.n_e:6d}  {loss_name:<12} option {opt}: iteration {med(wall[opt])}  assemble {med(asm[opt])}  cost {cost[opt]:.9e}")
                print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
        for r in records:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
