"""Prior factors on camera poses and intrinsics in bundle adjustment (apexgpu_set_pose_priors / _set_intrinsic_priors),
measured in one process on the ladybug-1723 and venice-1778 synthetic shapes (self-calibration, Huber 1, camera 0 as the gauge).
Writes profiles/ba_prior_bench.txt.  Records what was measured; gates nothing.

ms per LM iteration: the wall time of one lm_optimize call (it ends in a device synchronise) divided by its iteration count; the
median and the spread (min .. max) over five calls from the same start after a warm-up call -- with no priors, with a pose prior
on every camera, with a pose and an intrinsics prior on every camera.  Stage times: mean ms per call with stage timing on (it
serialises the stream); the add-ons are booked under the stage of the kernel they extend (cam_reduce, cost, step_stats), so
their time is the difference of those stages between the runs with and without priors.

--no-priors prints the first figure alone and touches nothing newer than apexgpu_lm_optimize: the same file, copied into a
checkout of the parent commit, measures that commit in the same visit (--parent FILE pastes its output into the report).

    python tools/ba_prior_bench.py [--out profiles/ba_prior_bench.txt] [--parent parent.txt] [--no-priors]
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
STAGES = ("cam_reduce", "landmark_reduce", "step_stats", "cost")


def lm_ms(s, d, runs=5):
    lm = (LevenbergMarquardtConfig.new().with_max_iterations(ITERS).with_cost_tolerance(0.0).with_parameter_tolerance(0.0)
          .with_gradient_tolerance(0.0))
    s.set_parameters(d.poses, d.intr, d.points)
    s.lm_optimize(lm)                                    # warm-up (graph capture, first-use allocations)
    t = []
    for _ in range(runs):
        s.set_parameters(d.poses, d.intr, d.points)
        t0 = time.perf_counter()
        res, _, _ = s.lm_optimize(lm)
        t.append(1e3 * (time.perf_counter() - t0) / max(res.iterations, 1))
    return float(np.median(t)), float(min(t)), float(max(t)), res.iterations


def stages(s, d):
    lm = (LevenbergMarquardtConfig.new().with_max_iterations(ITERS).with_cost_tolerance(0.0).with_parameter_tolerance(0.0)
          .with_gradient_tolerance(0.0))
    s.enable_stage_timing(True)
    s.set_parameters(d.poses, d.intr, d.points)
    s.reset_stage_times()
    s.lm_optimize(lm)
    out = s.stage_times()
    s.enable_stage_timing(False)
    return out


def one(shape, no_priors):
    d = pkg.synthetic.make_named(shape)
    s = GpuSchurComplementSolver(0).initialize_structure(Problem.bundle_adjustment(d, OptimizationType.SelfCalibration))
    lines = [f"{shape}: {d.n_cam} cameras, {d.n_pt} landmarks, {d.n_obs} observations"]
    q = d.poses[:, 3:7] / np.linalg.norm(d.poses[:, 3:7], axis=1, keepdims=True)
    pose = [(c, np.r_[d.poses[c, :3], q[c]], 0.5, 2.0) for c in range(d.n_cam)]
    intr = [(c, d.intr[c], None, 0.1) for c in range(d.n_cam)]
    runs = (("no priors", [], []),) if no_priors else (("no priors", [], []), ("pose prior on every camera", pose, []),
                                                       ("pose + intrinsics prior on every camera", pose, intr))
    base = None
    for name, pp, ip in runs:
        if not no_priors:
            s.set_priors(pp, ip)
        med, lo, hi, it = lm_ms(s, d)
        st = stages(s, d)
        lines.append(f"  {name:42s} {med:7.3f} ms per LM iteration (min {lo:.3f} .. max {hi:.3f}, {it} iterations)")
        lines.append("    stages (mean ms per call, calls): " + "  ".join(f"{k} {st[k][0]:.4f} x{st[k][1]}" for k in STAGES if k in st))
        if base is None:
            base = st
        else:
            lines.append("    add-ons (stage time minus the no-prior run's, ms per call): " +
                         "  ".join(f"{k} {st[k][0] - base[k][0]:+.4f}" for k in STAGES if k in st))
    s.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ba_prior_bench.txt"))
    ap.add_argument("--parent", default=None)
    ap.add_argument("--no-priors", action="store_true")
    a = ap.parse_args()
    lines = []
    for shape in SHAPES:
        lines += one(shape, a.no_priors)
    if a.parent:
        lines += ["", "the parent commit, same visit (this file with --no-priors in a checkout of it):"] + ["  " + l.rstrip() for l in open(a.parent)]
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
