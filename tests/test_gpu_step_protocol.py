"""The trial-step protocol (step_stats, eval_step, commit_step, discard_step) that TileBackend runs once for the bundle-adjustment
handle and the two pose-graph handles, through the Python surface of the C ABI (needs a real MI355X: `pytest -m gpu`).

Every public sequence once per handle, at the smallest fixtures of the suites that cover the paths in depth (ba6x40, pg_sphere_8x12,
the 40-vertex Manhattan graph of test_gpu_se2_parity.py):

    solve, step_stats; eval_step; discard_step, get_parameters; solve; eval_step; commit_step

with "eager_step_eval" 1 (the answers are posted at the solve's wait) and 0 (each call enqueues and waits itself).

Bounds.  BA and SE2 assemble in a fixed order of summation: the statistics and trial costs of the two modes are the same bits.
SE3 scatters its edges with fp64 atomics: rtol 1e-11, the bound of test_gpu_parity.py's eager test; its solves run at lambda = 1e4,
where cond(H + lambda I) is of order one, so that the order of the atomic additions (2^-53 relative per addition) stays far below it.
After a discard the parameters are x (+) d (+) (-d), not a snapshot: poses against tests/manifold_ref.py at the suite's retraction
tolerance (rtol 1e-13 + atol 1e-15, test_gpu_fixed_dofs.py), points and intrinsics (p + d) - d in the same bits."""
import functools
import os

import numpy as np
import pytest

import apex_solver_amd as pkg
import manifold_ref as mr
from apex_solver_amd.capi import LinAlgError
from apex_solver_amd.pose_graph import GpuSparseCholeskySolver, PoseGraphProblem
from apex_solver_amd.solver import GpuSchurComplementSolver, OptimizationType, Problem

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
HANDLES = ["ba", "se3", "se2"]
LAMBDA = {"ba": 1e-3, "se3": 1e4, "se2": 1e-3}
POSE_RTOL, POSE_ATOL = 1e-13, 1e-15
EAGER_RTOL = {"ba": 0.0, "se3": 1e-11, "se2": 0.0}


def cols(col, w):
    return np.asarray(col)[:, None] + np.arange(w)[None]


class Handle:
    """one handle of either class behind the calls the sequence needs; params() is a tuple of arrays"""

    def __init__(self, kind, eager):
        self.kind = kind
        if kind == "ba":
            g = np.load(os.path.join(HERE, "golden", "ba6x40_selfcal.npz"))
            d = pkg.synthetic.BAProblemData(poses=g["poses0"], intr=g["intr0"], points=g["points0"], cam_idx=g["cam_idx"],
                                            pt_idx=g["pt_idx"], obs_uv=g["obs_uv"], name="golden")
            self.prob = Problem.bundle_adjustment(d, OptimizationType.SelfCalibration, 1.0)
            self.s = GpuSchurComplementSolver(0).with_option("eager_step_eval", eager).initialize_structure(self.prob)
            self.start = (d.poses, d.intr, d.points)
        else:
            if kind == "se3":
                g = np.load(os.path.join(HERE, "golden", "pg_sphere_8x12.npz"))
                d = pkg.synthetic.PoseGraphData(ids=g["ids"], poses=g["poses0"], e_from=g["e_from"], e_to=g["e_to"], meas=g["meas"])
                self.prob = PoseGraphProblem(d, None, fix=g["fix"].copy())
            else:
                d = pkg.synthetic.make_manhattan(40)
                self.prob = PoseGraphProblem.pose_graph(d)
            self.s = GpuSparseCholeskySolver(0).with_option("eager_step_eval", eager).initialize_structure(self.prob)
            self.start = (d.poses,)
        self.s.set_parameters(*self.start)

    def params(self):
        p = self.s.get_parameters()
        return tuple(np.array(x) for x in p) if self.kind == "ba" else (np.array(p),)

    def solve(self):
        return np.array(self.s.solve_augmented_equation(LAMBDA[self.kind]))

    def there_and_back(self, p, step):
        """x (+) d (+) (-d) under the fixed-DOF masks, on the host"""
        prob = self.prob
        if self.kind == "ba":
            lay = prob.layout
            dd = np.where(prob.fix_pose.astype(bool), 0.0, step[cols(lay.pose_col, 6)])
            di = np.where(prob.fix_intr.astype(bool), 0.0, step[cols(lay.intr_col, 3)])
            dp = np.where(prob.fix_pt.astype(bool), 0.0, step[cols(lay.pt_col, 3)])
            return mr.se3_plus(mr.se3_plus(p[0], dd).astype(np.float64), -dd), (p[1] + di) - di, (p[2] + dp) - dp
        dof = prob.dof
        dd = np.where(prob.fix.astype(bool), 0.0, step[cols(prob.pose_col, dof)])
        plus = mr.se3_plus if self.kind == "se3" else mr.se2_plus
        return (plus(plus(p[0], dd).astype(np.float64), -dd),)


def refused(call, text):
    with pytest.raises(LinAlgError) as e:
        call()
    assert e.value.kind == "InvalidState" and str(e.value) == "InvalidState: " + text, str(e.value)


@functools.lru_cache(maxsize=None)
def sequence(kind, eager):
    """the whole sequence on one handle, wrong-state calls in between; what it saw"""
    h = Handle(kind, eager)
    s = h.s
    out = {}
    for call in (s.step_stats, s.eval_step):
        refused(call, "no step computed")
    for call in (s.commit_step, s.discard_step):
        refused(call, "no trial point")
    p0 = h.params()
    step = h.solve()
    out["stats"] = s.step_stats()
    refused(s.commit_step, "no trial point")       # (the statistics alone make no trial point)
    refused(s.discard_step, "no trial point")
    out["trial_cost"] = s.eval_step()
    assert s.step_stats() == out["stats"]          # (asked again behind eval_step: the same answer)
    s.discard_step()
    refused(s.discard_step, "no trial point")
    refused(s.step_stats, "no step computed")      # (the step went with the trial point)
    back = h.params()
    out["back"], out["want_back"], out["moved"] = back, h.there_and_back(p0, step), float(np.abs(step).max())
    step2 = h.solve()
    out["stats2"] = s.step_stats()
    out["trial_cost2"] = s.eval_step()
    s.commit_step()
    refused(s.commit_step, "no trial point")       # commit twice
    refused(s.eval_step, "no step computed")
    out["cost_after_commit"] = s.compute_cost()
    out["committed"] = h.params()
    out["p0"], out["step"], out["step2"] = p0, step, step2
    s.close()
    return out


def close(a, b, rtol):
    return np.array_equal(a, b) if rtol == 0.0 else np.allclose(a, b, rtol=rtol, atol=0.0)


@pytest.mark.parametrize("kind", HANDLES)
def test_answers_at_the_wait_are_the_answers_on_request(kind):
    e1, e0 = sequence(kind, 1), sequence(kind, 0)
    rtol = EAGER_RTOL[kind]
    for key in ("stats", "trial_cost", "stats2", "trial_cost2"):
        a, b = np.asarray(e1[key], dtype=np.float64), np.asarray(e0[key], dtype=np.float64)
        print(kind, key, a, b, "worst relative difference", float(np.max(np.abs(a - b) / np.abs(b))))
        assert close(a, b, rtol), (kind, key, a, b)
    for e in (e1, e0):
        assert all(np.isfinite(v) and v > 0.0 for v in (*e["stats"], e["trial_cost"], *e["stats2"], e["trial_cost2"]))
        assert e["cost_after_commit"] == pytest.approx(e["trial_cost2"], rel=1e-12)   # (the trial cost is the cost there)


@pytest.mark.parametrize("eager", [1, 0], ids=["eager", "on-request"])
@pytest.mark.parametrize("kind", HANDLES)
def test_discard_is_the_inverse_retraction(kind, eager):
    e = sequence(kind, eager)
    assert e["moved"] > 1e-9   # (a step that moves something)
    poses, want = e["back"][0], np.asarray(e["want_back"][0]).astype(np.float64)
    print(kind, eager, "poses worst |gpu - ref|", float(np.abs(poses - want).max()), "vs the start", float(np.abs(poses - e["p0"][0]).max()))
    assert np.allclose(poses, want, rtol=POSE_RTOL, atol=POSE_ATOL)
    for got, ref in zip(e["back"][1:], e["want_back"][1:]):   # BA: intrinsics and points
        assert np.array_equal(got, ref)
    # and the commit of the second solve landed on another point than the one the discard restored
    assert not np.array_equal(e["committed"][0], e["back"][0])


@pytest.mark.parametrize("eager", [1, 0], ids=["eager", "on-request"])
@pytest.mark.parametrize("kind", ["se3", "se2"])
def test_dogleg_step_answers_and_the_lm_solve_behind_it(kind, eager):
    """step_stats / eval_step behind a Dog-Leg step answer from its DoglegStepInfo; an LM solve behind that answers for itself."""
    lone = Handle(kind, eager)
    lone.solve()
    lm_stats, lm_trial = lone.s.step_stats(), lone.s.eval_step()
    lone.s.close()
    h = Handle(kind, eager)
    s = h.s
    mu, radius = 1e-4, 0.5 * lm_stats[1]   # (half the damped LM step's length: the Dog-Leg step is cut to it, another step than LM's)
    o = s.dogleg_step(mu, radius)
    assert s.step_stats() == (o["gradient_norm"], o["step_norm"], o["predicted_reduction"])
    trial = s.eval_step()
    s.discard_step()
    r = s.dogleg_step(mu, 0.5 * radius, reuse=True)   # a reused step posts its own answers
    assert r["reused"] and r["step_norm"] < o["step_norm"]
    assert s.step_stats() == (r["gradient_norm"], r["step_norm"], r["predicted_reduction"])
    trial_r = s.eval_step()
    s.commit_step()
    assert s.compute_cost() == pytest.approx(trial_r, rel=1e-12) and trial_r != trial
    # LM behind Dog-Leg on the same handle, from the start again: its own statistics and trial cost
    s.set_parameters(*h.start)
    s.dogleg_step(mu, radius)
    h.solve()
    got, got_trial = s.step_stats(), s.eval_step()
    s.close()
    print(kind, eager, "LM behind Dog-Leg", got, got_trial, "lone", lm_stats, lm_trial, "Dog-Leg", o)
    assert close(np.array(got), np.array(lm_stats), EAGER_RTOL[kind]) and close(got_trial, lm_trial, EAGER_RTOL[kind])
    assert got[1] != o["step_norm"] and got[2] != o["predicted_reduction"] and got_trial != trial
