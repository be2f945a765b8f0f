"""The loss family on the bundle-adjustment front end, as far as it goes without a device: the exported symbols, the shared
names, and the Problem that carries a loss."""
import ctypes as C

import pytest

import apex_solver_amd as pkg
from apex_solver_amd import capi, loss, pose_graph, solver
from apex_solver_amd.solver import OptimizationType, Problem


def test_library_exports_the_ba_loss_calls():
    L = capi.load()
    for name in ("apexgpu_set_loss", "apexgpu_get_loss"):
        assert name in capi.SYMBOLS and hasattr(L, name)
    # no handle: InvalidState, not a crash
    k = C.c_int(); p = (C.c_double * 2)()
    assert L.apexgpu_set_loss(None, capi.LOSS_CAUCHY, 1.0, 0.0) == -6
    assert L.apexgpu_get_loss(None, C.byref(k), C.byref(p)) == -6


def test_both_front_ends_share_the_loss_names():
    assert loss.Loss is pose_graph.Loss is solver.Loss
    assert loss.create_loss_function is pose_graph.create_loss_function is solver.create_loss_function
    assert loss.create_loss_function("Cauchy") == loss.Loss(capi.LOSS_CAUCHY, 2.3849)


def test_problem_carries_the_loss():
    d = pkg.synthetic.make_problem(6, 40, 3, 5, config_id=3)
    cauchy = loss.create_loss_function("cauchy")
    p = Problem.bundle_adjustment(d, loss=cauchy)
    assert p.loss == cauchy and p.huber_delta == 1.0 and p.fix_pose[0].all()
    assert Problem.bundle_adjustment(d).loss is None and Problem(d).loss is None
    assert Problem(d, OptimizationType.BundleAdjustment, None, loss=cauchy).loss == cauchy
    with pytest.raises(capi.LinAlgError):   # before initialize_structure
        solver.GpuSchurComplementSolver(0).set_loss(cauchy)
