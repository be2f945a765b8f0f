"""The premises of tests/test_gpu_trust_region.py, on the numpy loops alone (no GPU): the chosen starts make the reference
Dog-Leg run walk through every branch, with no decision on its threshold; Gauss-Newton descends from its start; and the
exactly singular two-vertex graph fails numpy's Cholesky."""
import numpy as np
import pytest

import np_ref_trust_region as tr
import tr_cases as tc
from apex_solver_amd.pose_graph import PoseGraphProblem
from apex_solver_amd.synthetic import PoseGraphData


@pytest.mark.parametrize("man", ["se2", "se3"])
def test_dogleg_reference_run_takes_every_branch(man):
    o = tc.dogleg_reference(man, False)
    R = o["history"]
    assert set(R[:, 9]) == {0.0, 1.0, 2.0}                      # GaussNewton, SteepestDescent, DogLeg
    rej = np.nonzero(R[:-1, 4] == 0)[0]
    assert rej.size and (R[rej + 1, 11] == 1).any()              # a rejection, then a reused step
    radius = np.concatenate([[o["radius0"]], R[:, 1]])
    assert ((np.diff(radius) > 0) & (R[:, 3] > 0.75)).any()      # a good step that grew the radius
    assert o["margins"].min() > 1e-6
    assert tc.dogleg_reference(man, True)["margins"].min() > 1e-6


@pytest.mark.parametrize("man", ["se2", "se3"])
def test_gauss_newton_reference_run_descends(man):
    for scaling in (False, True):
        o = tc.gauss_newton_reference(man, scaling)
        assert o["status"] in (1, 2, 3, 4) and o["iterations"] >= 3 and o["final_cost"] < 0.5 * o["initial_cost"]


@pytest.mark.parametrize("man", ["se2", "se3"])
def test_two_identity_vertices_have_an_exactly_singular_hessian(man):
    prob, P = singular_case(man)
    H, _ = P.normal_equations()
    I = np.eye(prob.dof)
    assert np.array_equal(H, np.block([[I, -I], [-I, I]]))        # exact in fp64: the second pivot is 0
    assert tr.solve_damped(H, np.zeros(H.shape[0]), 0.0) is None
    assert tr.gauss_newton(P)["status"] == 100


def singular_case(man):
    ident = np.zeros((2, 3)) if man == "se2" else np.tile([0.0, 0, 0, 1, 0, 0, 0], (2, 1))
    d = PoseGraphData(ids=np.arange(2, dtype=np.int64), poses=ident.copy(), e_from=np.array([0], np.uint32),
                      e_to=np.array([1], np.uint32), meas=ident[:1].copy(), name="singular")
    prob = PoseGraphProblem(d)   # no prior, no fixed DOF: the gauge is free
    return prob, tc.numpy_problem(prob, d.poses)
