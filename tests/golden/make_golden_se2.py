"""Writes tests/golden/se2_manhattan_40.npz from the numpy reference (tests/np_ref_se2.py): inputs, r, J, H, g, the step at
lambda = 1 and the LM history of make_manhattan(40) with the first vertex fixed.  Run from the repository root:
    python tests/golden/make_golden_se2.py

The reference evaluates its trigonometry through numpy's long double; the fixture is reproduced to 1e-14 only where that is
the x86 80-bit type (np.finfo(np.longdouble).nmant == 63), which is where it was written."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import apex_solver_amd as pkg   # noqa: E402
import np_ref_se2 as ref        # noqa: E402

LM = dict(max_iterations=30, cost_tolerance=1e-4, parameter_tolerance=1e-4, damping=1e-3)


def build():
    d = pkg.synthetic.make_manhattan(40)
    names = sorted(f"x{i}" for i in d.ids)
    col = np.array([3 * names.index(f"x{i}") for i in d.ids], dtype=np.int64)
    fix = np.zeros((d.n_v, 3), np.uint8); fix[0] = 1
    p = ref.Problem(d.poses, d.e_from, d.e_to, d.meas, col, fix)
    r, J = p.edge_blocks()
    H, g = p.normal_equations()
    step, _ = p.solve(1.0)
    lm = ref.Problem(d.poses, d.e_from, d.e_to, d.meas, col, fix).lm_optimize(**LM)
    return dict(ids=d.ids, poses=d.poses, e_from=d.e_from, e_to=d.e_to, meas=d.meas, pose_col=col, fix=fix, r=r, J=J, H=H, g=g,
                step_lambda_1=step, cost=p.cost(), initial_cost=lm["initial_cost"], lm_history=lm["history"], lm_status=lm["status"], lm_iterations=lm["iterations"],
                lm_final_cost=lm["final_cost"])


if __name__ == "__main__":
    np.savez_compressed(os.path.join(HERE, "se2_manhattan_40.npz"), **build())
