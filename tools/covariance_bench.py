#!/usr/bin/env python3
"""Marginal covariances by selected inversion of the tile factor against one factorisation, on the two flagship shapes:
the sphere2500 pose graph (synthetic.make_sphere(50, 50), as bench.py) and the final-13682 BA problem (synthetic.make_named,
as bench.py).  Per workload: one direct solve at lambda = 1e-3, the factorisation time from its stage timer alone (mean
per solve over five), the first covariance call (it allocates Z and builds the lists), then the median of five synchronised calls, the
tile products and their rate, the extra device memory and the time of every level group's three launches (root first).
With --landmarks (BA shapes: final-13682, ladybug-1723) the landmark pass instead: per call the kernel time with Z reused
(after a camera call on the same factor) and the wall time of a call that recomputes Z first, the observation pairs, the
bytes the pass adds, and both against one factorisation.
  python tools/covariance_bench.py [--workloads sphere2500,final-13682] [--landmarks] [--reps 5] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import apex_solver_amd as pkg  # noqa: E402
from apex_solver_amd.pose_graph import GpuSparseCholeskySolver, PoseGraphProblem  # noqa: E402
from apex_solver_amd.solver import GpuSchurComplementSolver, OptimizationType, Problem  # noqa: E402

TILE_FLOP = 2.0 * 144 ** 3
FP64_MFMA_PEAK = 78.6e12   # MI355X fp64 matrix peak (the figure behind bench.py's factor_mfma_frac)


def measure(s, cov_fn, factor_stage, stage_names, reps, lam=1e-3):
    s.set_option("covariance_timing", 1)
    s.enable_stage_timing(1 << (stage_names.index(factor_stage) + 1))   # the factorisation's stage alone (bench.py's stage_sum_ms)
    s.solve_augmented_equation(lam, want_step=False)   # (code objects loaded, graphs captured)
    s.reset_stage_times()
    for _ in range(5):
        s.solve_augmented_equation(lam, want_step=False)
    tot_ms, n_fac_calls = s.stage_times()[factor_stage]     # (total over the calls, and their number)
    factor_ms = tot_ms / max(n_fac_calls, 1)
    s.enable_stage_timing(False)
    s.solve_augmented_equation(lam, want_step=False)   # the factor the covariance inverts (no stage events around it)
    t0 = time.perf_counter()
    cov_fn()
    first_ms = (time.perf_counter() - t0) * 1e3
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        cov_fn()        # (synchronises: the blocks are on the host when it returns)
        times.append((time.perf_counter() - t0) * 1e3)
    info = s.info()
    st = s.covariance_stats(group_cap=int(info["etree_levels"]) + 8)
    n_prod = st["y_products"] + st["zoff_products"] + st["zdiag_products"]
    n_fac = info["n_update"] + info["n_trsm"] + info["n_potrf"]
    cov_ms = float(np.median(times))
    g = st["group_ms"]
    top = sorted(range(len(g)), key=lambda i: -g[i])[:5]
    return dict(cov_ms_median=round(cov_ms, 3), cov_ms_all=[round(t, 3) for t in times], cov_first_call_ms=round(first_ms, 3),
                factor_ms=round(factor_ms, 3), ratio_cov_over_factor=round(cov_ms / factor_ms, 2) if factor_ms > 0 else None,
                cov_tile_products=n_prod, factor_tile_ops=n_fac, products_y_zoff_zdiag=[st["y_products"], st["zoff_products"], st["zdiag_products"]],
                cov_tflops=round(n_prod * TILE_FLOP / (cov_ms * 1e-3) / 1e12, 2),
                cov_fp64_mfma_frac=round(n_prod * TILE_FLOP / (cov_ms * 1e-3) / FP64_MFMA_PEAK, 3),
                extra_device_gb=round(st["extra_bytes"] / 1e9, 3), tiles=info["tiles"], level_groups=st["level_groups"],
                group_ms_sum=round(sum(g), 3), group_ms=[round(x, 3) for x in g],
                slowest_groups=[dict(group=i, ms=round(g[i], 3)) for i in top])


def run_pose_graph(reps):
    d = pkg.synthetic.make_sphere(50, 50)
    prob = PoseGraphProblem.pose_graph(d)
    s = GpuSparseCholeskySolver(0).initialize_structure(prob)
    s.set_parameters(d.poses)
    r = measure(s, s.pose_covariance_blocks, "factor", pkg.capi.PG_STAGE_NAMES, reps)
    s.close()
    return r


def run_ba(reps):
    d = pkg.synthetic.make_named("final-13682")
    prob = Problem.bundle_adjustment(d, OptimizationType.SelfCalibration, 1.0)
    s = GpuSchurComplementSolver(0).initialize_structure(prob)
    s.set_parameters(d.poses, d.intr, d.points)
    r = measure(s, s.camera_covariance_blocks, "factor", pkg.capi.STAGE_NAMES, reps)
    s.close()
    return r


def measure_landmarks(s, reps, lam=1e-3):
    s.set_option("covariance_timing", 1)
    stage_names = pkg.capi.STAGE_NAMES
    s.enable_stage_timing(1 << (stage_names.index("factor") + 1))
    s.solve_augmented_equation(lam, want_step=False)
    s.reset_stage_times()
    for _ in range(5):
        s.solve_augmented_equation(lam, want_step=False)
    tot_ms, n_fac_calls = s.stage_times()["factor"]
    factor_ms = tot_ms / max(n_fac_calls, 1)
    s.enable_stage_timing(False)
    s.solve_augmented_equation(lam, want_step=False)
    t0 = time.perf_counter()
    s.landmark_covariance_blocks()             # first call: Z computed, lists and output allocated
    first_ms = (time.perf_counter() - t0) * 1e3
    reused, recompute_wall, cam_ms = [], [], []
    for _ in range(reps):
        s.solve_augmented_equation(lam, want_step=False)
        t0 = time.perf_counter()
        s.landmark_covariance_blocks()         # Z of the new factor computed first (no camera gather)
        recompute_wall.append((time.perf_counter() - t0) * 1e3)
        assert s.landmark_covariance_stats()["recomputed_z"]
        t0 = time.perf_counter()
        s.camera_covariance_blocks()
        cam_ms.append((time.perf_counter() - t0) * 1e3)
        s.landmark_covariance_blocks()         # Z reused: the landmark kernels alone
        st = s.landmark_covariance_stats()
        assert not st["recomputed_z"]
        reused.append(st["landmark_ms"])
    lm_ms = float(np.median(reused))
    return dict(landmark_ms_z_reused=round(lm_ms, 3), landmark_ms_all=[round(t, 3) for t in reused],
                landmark_call_ms_z_recomputed=round(float(np.median(recompute_wall)), 3),
                camera_call_ms=round(float(np.median(cam_ms)), 3), first_call_ms=round(first_ms, 3),
                factor_ms=round(factor_ms, 3), ratio_landmark_over_factor=round(lm_ms / factor_ms, 3) if factor_ms > 0 else None,
                pairs=st["pairs"], landmark_extra_gb=round(st["extra_bytes"] / 1e9, 4),
                z_extra_gb=round(s.covariance_stats()["extra_bytes"] / 1e9, 3), n_pt=s._h.n_pt)


def run_ba_landmarks(name, reps):
    d = pkg.synthetic.make_named(name)
    prob = Problem.bundle_adjustment(d, OptimizationType.SelfCalibration, 1.0)
    s = GpuSchurComplementSolver(0).initialize_structure(prob)
    s.set_parameters(d.poses, d.intr, d.points)
    r = measure_landmarks(s, reps)
    s.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="sphere2500,final-13682")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--landmarks", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for w in a.workloads.split(","):
        if a.landmarks:
            r = run_ba_landmarks(w, a.reps)
        else:
            r = run_pose_graph(a.reps) if w == "sphere2500" else run_ba(a.reps)
        line = json.dumps(dict(workload=w, lam=1e-3, **r))
        print(line, flush=True)
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
