"""Levenberg-Marquardt and Dog-Leg on bundle adjustment, measured side by side in one process on the ladybug-1723 and venice-1778
synthetic shapes (self-calibration, Huber 1, camera 0 as the gauge).  Writes profiles/ba_trust_region_bench.txt.  Records what was
measured; gates nothing.

Whole loops: the wall time of one optimize call, which ends in a device synchronise, divided by its iteration count; the median
over three calls from the same start after a warm-up call.  Single steps: the wall time of solve / dogleg_step + eval_step +
discard_step, each call ending in its one host wait, median over 12 calls after two warm-up calls; reused steps halve the radius
each time from a fresh solve (every fifth call is that fresh solve and is not counted).  Stage times: mean ms per call with stage
timing on, which serialises the stream; a stage that never ran shows 0 calls.  The Gram pass has no stage of its own: it is booked
under step_stats with the inner products, the combine and the blend, and a reused step runs the combine and the blend only, so
"dots + Gram" is the step_stats time of a fresh step minus that of a reused one; the Gram pass alone is the step_stats time of
apexgpu_jv_gram calls, which book their one kernel there.

--lm-only prints the LM figures alone and touches nothing newer than apexgpu_lm_optimize: the same file, copied into a checkout
of the parent commit, measures that commit in the same visit (--parent FILE pastes its output into the report).

    python tools/ba_trust_region_bench.py [--out profiles/ba_trust_region_bench.txt] [--parent parent_lm.txt] [--lm-only]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import apex_solver_amd as pkg                                                                                   # noqa: E402
from apex_solver_amd.solver import GpuSchurComplementSolver, LevenbergMarquardtConfig, OptimizationType, Problem  # noqa: E402

ITERS = 10
SHAPES = ("ladybug-1723", "venice-1778")


def lm_loop(s, d):
    lm = (LevenbergMarquardtConfig.new().with_max_iterations(ITERS).with_cost_tolerance(0.0).with_parameter_tolerance(0.0)
          .with_gradient_tolerance(0.0))
    return timed_loop(s, d, lambda: s.lm_optimize(lm))


def timed_loop(s, d, call):
    s.set_parameters(d.poses, d.intr, d.points)
    call()                                               # warm-up (graph capture, first-use allocations)
    per_iter = []
    for _ in range(3):
        s.set_parameters(d.poses, d.intr, d.points)
        t0 = time.perf_counter()
        res, hist, _ = call()
        per_iter.append(1e3 * (time.perf_counter() - t0) / max(res.iterations, 1))
    return dict(ms=float(np.median(per_iter)), iterations=res.iterations, status=res.status, hist=hist, cost=(res.initial_cost, res.final_cost))


def lm_step_ms(s, d, n=12):
    s.set_parameters(d.poses, d.intr, d.points)

    def body():
        s.solve_augmented_equation(1e-3, want_step=False); s.step_stats(); s.eval_step(); s.discard_step()
    body(); body()
    t = []
    for _ in range(n):
        t0 = time.perf_counter(); body(); t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t))


def dogleg_steps(s, d, cfg, timing):
    n = 8 if timing else 12

    def lm_step():
        s.solve_augmented_equation(1e-3, want_step=False); s.step_stats(); s.eval_step(); s.discard_step()

    def fresh_step():
        s.dogleg_step(cfg.initial_mu, cfg.trust_region_radius); s.eval_step(); s.discard_step()

    out = {}
    for name, body in (("LM step", lm_step), ("Dog-Leg fresh", fresh_step)):
        s.set_parameters(d.poses, d.intr, d.points)
        body(); body()
        s.reset_stage_times()
        t = []
        for _ in range(n):
            t0 = time.perf_counter(); body(); t.append(1e3 * (time.perf_counter() - t0))
        out[name] = s.stage_times() if timing else float(np.median(t))
    s.set_parameters(d.poses, d.intr, d.points)
    t, first = [], True
    acc = None
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
        if acc is None:
            acc = {k: [0.0, 0] for k in after}
        for k in after:   # the reused steps' share: totals after minus before (mean ms per call and the call count)
            acc[k][0] += after[k][0] * after[k][1] - before[k][0] * before[k][1]
            acc[k][1] += after[k][1] - before[k][1]
    out["Dog-Leg reused"] = {k: (v[0] / max(v[1], 1), v[1]) for k, v in acc.items()} if timing else float(np.median(t[:n]))
    return out


def one(shape, lm_only):
    d = pkg.synthetic.make_named(shape)
    prob = Problem.bundle_adjustment(d, OptimizationType.SelfCalibration)
    s = GpuSchurComplementSolver(0).initialize_structure(prob)
    r = dict(name=shape, n_cam=d.n_cam, n_pt=d.n_pt, n_obs=d.n_obs, lm=lm_loop(s, d), lm_step=lm_step_ms(s, d))
    if not lm_only:
        from apex_solver_amd.pose_graph import DogLegConfig
        zero = dict(cost_tolerance=0.0, parameter_tolerance=0.0, gradient_tolerance=0.0)
        cfg = DogLegConfig(max_iterations=ITERS, **zero)
        r["dl"] = timed_loop(s, d, lambda: s.dogleg_optimize(cfg))
        s.set_parameters(d.poses, d.intr, d.points)
        s.apply_column_scaling(1.0 / (1.0 + s.compute_column_norms()))   # (the reference's default for Dog-Leg; LM steps cost the same either way)
        r["steps"] = dogleg_steps(s, d, cfg, False)
        s.enable_stage_timing(True)
        r["stages"] = dogleg_steps(s, d, cfg, True)
        # the Gram pass alone: apexgpu_jv_gram books its kernel (and the sum of its partials) under step_stats and nothing else
        rng = np.random.default_rng(0)
        a, b = rng.normal(size=prob.total_dof), rng.normal(size=prob.total_dof)
        s.jv_gram(a, b)
        s.reset_stage_times()
        for _ in range(10):
            s.jv_gram(a, b)
        r["gram"] = s.stage_times()["step_stats"]
    s.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ba_trust_region_bench.txt"))
    ap.add_argument("--parent", default=None, help="the --lm-only output of the parent commit, pasted into the report")
    ap.add_argument("--lm-only", action="store_true")
    a = ap.parse_args()
    rows = [one(sh, a.lm_only) for sh in SHAPES]
    if a.lm_only:
        for r in rows:
            print(f"{r['name']}: LM loop {r['lm']['ms']:.3f} ms / iteration ({r['lm']['iterations']} iterations), LM step {r['lm_step']:.3f} ms / step")
        return
    lines = ["LM and Dog-Leg on bundle adjustment, one MI355X: tools/ba_trust_region_bench.py",
             f"(loops: median of 3 calls of up to {ITERS} iterations, wall time / iterations, after a warm-up call; steps: median wall time of",
             " step + eval_step + discard_step over 12 calls, Jacobi-scaled variables; stages: mean ms per call with stage timing on, (calls) beside it)", ""]
    for r in rows:
        lines.append(f"{r['name']}: {r['n_cam']} cameras, {r['n_pt']} landmarks, {r['n_obs']} observations, self-calibration, Huber 1")
        lines.append(f"    LM       loop  {r['lm']['ms']:.3f} ms / iteration ({r['lm']['iterations']} iterations, status {r['lm']['status']}, cost {r['lm']['cost'][0]:.6g} -> {r['lm']['cost'][1]:.6g})")
        for key, label in (("dl", "Dog-Leg  loop "),):
            v = r[key]; h = v["hist"]
            lines.append(f"    {label} {v['ms']:.3f} ms / iteration ({v['iterations']} iterations, status {v['status']}, {int(h[:, 11].sum())} reused, "
                         f"{int((h[:, 4] == 0).sum())} rejected, cost {v['cost'][0]:.6g} -> {v['cost'][1]:.6g})")
        for k, v in r["steps"].items():
            lines.append(f"    {k:15s} {v:.3f} ms / step")
        for k, st in r["stages"].items():
            lines.append(f"    stages of {k}: " + ", ".join(f"{n} {ms:.3f} ({c})" for n, (ms, c) in st.items()))
        fresh, reused = r["stages"]["Dog-Leg fresh"]["step_stats"][0], r["stages"]["Dog-Leg reused"]["step_stats"][0]
        lines.append(f"    dots + Gram pass: {fresh - reused:.3f} ms (step_stats of a fresh step {fresh:.3f} - of a reused step {reused:.3f})")
        lines.append(f"    Gram pass alone:  {r['gram'][0]:.3f} ms (k_ba_jv_gram + the sum of its partials between two events, mean of {r['gram'][1]} apexgpu_jv_gram calls)")
        lines.append("")
    if a.parent and os.path.exists(a.parent):
        lines += ["the parent commit, same visit (--lm-only from a checkout of it):"] + ["    " + l for l in open(a.parent).read().splitlines() if l.strip()] + [""]
    txt = "\n".join(lines)
    print(txt)
    with open(a.out, "w") as f:
        f.write(txt)


if __name__ == "__main__":
    main()
