"""The option "row_owned_assembly" on SE3 pose-graph handles, end to end: run-to-run reproducibility to the bit, the goldens and
the optimiser loops against the references the default assembly is held to (the goldens, the oracle, the numpy restatements --
never the default path itself), prior blocks that arrive shuffled, covariances, fixed-DOF masks, and what the option accepts.
tests/test_gpu_se3_row_crafted.py checks the assembly itself block by block."""
import os

import numpy as np
import pytest

import apex_solver_amd as pkg
import fixed_masks as fm
import np_ref_loss as nl
import pg_asm_cases as pc
import tr_cases as tc
from apex_solver_amd import capi
from apex_solver_amd.pose_graph import (DogLegConfig, GaussNewtonConfig, GpuSparseCholeskySolver, PoseGraphProblem, create_loss_function,
                                        se3_as_vector)
from apex_solver_amd.solver import LevenbergMarquardt, LevenbergMarquardtConfig, LinearSolverType
from oracle import pg_oracle as po
from test_gpu_covariance import check_pg, pg_fixture
from test_gpu_pg_parity import STEP_FORWARD_BOUND, problem_from_fixture, rel

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
OPT = "row_owned_assembly"


def row_solver(prob=None, poses=None, **opts):
    s = GpuSparseCholeskySolver().with_option(OPT, 1)
    for k, v in opts.items():
        s.with_option(k, v)
    if prob is not None:
        s.initialize_structure(prob)
        s.set_parameters(prob.data.poses if poses is None else poses)
    return s


def golden(name):
    return np.load(os.path.join(HERE, "golden", name + ".npz"))


# ---- 2. run-to-run reproducibility ------------------------------------------------------------------------------------------------
def _repro_problem(weighted):
    g = golden("pg_sphere_8x12")
    d = pkg.synthetic.PoseGraphData(ids=g["ids"], poses=g["poses0"], e_from=g["e_from"], e_to=g["e_to"], meas=g["meas"])
    kw = dict(loss=create_loss_function("cauchy"), information=pc.ig_information(d)) if weighted else {}
    prob = PoseGraphProblem(d, **kw)
    for dof in range(6):
        prob.fix_variable(f"x{int(d.ids[3])}", dof)                           # one fixed vertex
    prob.add_prior(f"x{int(d.ids[0])}", huber_delta=1.0)
    prob.add_prior(f"x{int(d.ids[40])}")
    prob.add_prior(f"x{int(d.ids[0])}", data=se3_as_vector(d.poses[1]), huber_delta=0.05)
    return prob


def _one_run(prob, loop):
    s = row_solver(prob)
    if loop == "lm":
        res, hist, _ = s.lm_optimize(LevenbergMarquardtConfig(max_iterations=6))
    else:
        res, hist, _ = s.dogleg_optimize(DogLegConfig(max_iterations=6, trust_region_radius=1.0))
    out = (res.iterations, hist.copy(), s.get_parameters().copy()) + tuple(x.copy() for x in s.get_hessian(1e-3))
    s.close()
    return out


@pytest.mark.parametrize("loop,weighted", [("lm", False), ("lm", True), ("dogleg", False)], ids=["lm-none", "lm-cauchy-info", "dogleg-none"])
def test_two_fresh_handles_give_the_same_bits(loop, weighted):
    prob = _repro_problem(weighted)
    a, b = _one_run(prob, loop), _one_run(prob, loop)
    assert a[0] == b[0] and a[0] >= 2
    assert a[1][0, 0] > a[1][-1, 0]                                           # the run descended: there is something to compare
    for x, y, what in zip(a[1:], b[1:], ("history", "parameters", "H", "g")):
        assert np.array_equal(x, y), what
    assert not np.array_equal(a[2], prob.data.poses)


# ---- 3. goldens and loops ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pg_sphere_8x12", "pg_sphere_10x10_huber"])
def test_golden_iterations_row_owned(name):
    g = golden(name)
    prob = problem_from_fixture(g)
    s = row_solver(prob, g["poses0"])
    assert abs(s.compute_cost() - float(g["initial_cost"])) <= 1e-12 * float(g["initial_cost"])
    for it in range(int(g["iters"])):
        s.set_parameters(g[f"it{it}_poses"])
        lam = float(g[f"it{it}_lambda"])
        step = s.solve_augmented_equation(lam)
        assert rel(s.get_gradient(), g[f"it{it}_grad"]) < 1e-12
        assert rel(step, g[f"it{it}_step"]) < STEP_FORWARD_BOUND
        gn, sn, pred = s.step_stats()
        assert abs(pred - float(g[f"it{it}_pred"])) <= 1e-9 * abs(pred)
        assert abs(sn - np.linalg.norm(g[f"it{it}_step"])) <= 1e-9 * sn
        nc = s.eval_step()
        assert abs(nc - float(g[f"it{it}_new_cost"])) <= 1e-9 * nc
        s.discard_step()
    s.close()


@pytest.mark.parametrize("name", ["pg_sphere_8x12", "pg_sphere_10x10_huber"])
def test_golden_lm_history_row_owned(name):
    g = golden(name)
    prob = problem_from_fixture(g)
    cfg = LevenbergMarquardtConfig.new().with_max_iterations(10).with_linear_solver_type(LinearSolverType.SparseCholesky)
    res = LevenbergMarquardt.with_config(cfg).optimize(prob, solver=row_solver())
    assert res.status.value == int(g["lm_status"]) and res.iterations == int(g["lm_iterations"])
    H = g["lm_history"]
    assert np.allclose(res.history[:, 3], H[:, 3])                       # accept / reject pattern
    assert np.allclose(res.history[:, 0], H[:, 0], rtol=1e-7)            # cost after each iteration
    assert np.allclose(res.history[:, 1], H[:, 1], rtol=1e-5)            # damping
    assert abs(res.final_cost - float(g["lm_final_cost"])) <= 1e-7 * res.final_cost


def test_lm_with_prior_gauge_matches_the_oracle_loop_row_owned():
    d = pkg.synthetic.make_sphere(10, 12, config_id=9)
    prob = PoseGraphProblem(d).add_prior(f"x{int(d.ids[0])}", huber_delta=1.0)
    ref = po.PgOracle.from_problem(prob).lm_optimize(po.lm_config(max_iterations=30))
    cfg = LevenbergMarquardtConfig.new().with_max_iterations(30).with_linear_solver_type(LinearSolverType.SparseCholesky)
    res = LevenbergMarquardt.with_config(cfg).optimize(prob, solver=row_solver())
    assert res.status.value == ref["status"] and res.iterations == ref["iterations"]
    assert np.array_equal(res.history[:, 3], ref["history"][:, 3])       # accept / reject decisions
    assert abs(res.initial_cost - ref["initial_cost"]) <= 1e-12 * ref["initial_cost"]
    assert abs(res.final_cost - ref["final_cost"]) <= 1e-7 * ref["final_cost"]
    assert res.final_cost < 0.5 * res.initial_cost


@pytest.mark.parametrize("scaling", [False, True], ids=["plain", "jacobi-scaling"])
def test_dogleg_history_against_the_numpy_loop_row_owned(scaling):
    ref = tc.dogleg_reference("se3", scaling)
    assert ref["margins"].min() > 1e-6
    prob, p0 = tc.problem("se3")
    s = row_solver(prob, p0)
    res, H, c = s.dogleg_optimize(DogLegConfig(max_iterations=tc.DL_ITERS, trust_region_radius=ref["radius0"], use_jacobi_scaling=scaling))
    R = ref["history"]
    assert (res.status, res.iterations) == (ref["status"], ref["iterations"])
    assert np.array_equal(H[:, [4, 9, 11]], R[:, [4, 9, 11]])   # accepted, step type, reused
    assert np.array_equal(H[:, 2], R[:, 2])                     # mu
    np.testing.assert_allclose(H[:, 0], R[:, 0], rtol=1e-7)
    np.testing.assert_allclose(H[:, 1], R[:, 1], rtol=1e-7)
    assert c.trust_region_radius == pytest.approx(ref["radius"], rel=1e-7) and c.mu == ref["mu"]
    s.close()


@pytest.mark.parametrize("scaling", [False, True], ids=["plain", "jacobi-scaling"])
def test_gauss_newton_history_against_the_numpy_loop_row_owned(scaling):
    ref = tc.gauss_newton_reference("se3", scaling)
    prob, _ = tc.problem("se3")
    s = row_solver(prob, ref["start"])
    res, H, _ = s.gn_optimize(GaussNewtonConfig(max_iterations=6, use_jacobi_scaling=scaling))
    R = ref["history"]
    assert (res.status, res.iterations) == (ref["status"], ref["iterations"])
    np.testing.assert_allclose(H[:, 0], R[:, 0], rtol=1e-7)
    np.testing.assert_allclose(H[:, [4, 5]], R[:, [4, 5]], rtol=1e-6, atol=1e-10 * R[0, 4])
    assert (H[:, 3] == 1).all()
    s.close()


# ---- 4. priors --------------------------------------------------------------------------------------------------------------------
def test_shuffled_priors_with_three_on_one_vertex():
    d = pkg.synthetic.make_sphere(6, 10)
    rng = np.random.default_rng(12)
    prob = PoseGraphProblem(d, huber_delta=0.7)
    where = [41, 7, 41, 0, 59, 41, 7]                                         # three on vertex 41, not adjacent, among others
    deltas = [None, 0.05, 1e3, 0.05, None, 0.05, 1e3]
    for v, dl in zip(where, deltas):
        x = se3_as_vector(d.poses[v]); x[:3] += 0.3 * rng.standard_normal(3); x[3:] += 0.05 * rng.standard_normal(4)
        prob.add_prior(f"x{int(d.ids[v])}", data=x, huber_delta=dl)
    assert [q[0] for q in prob.priors] == where
    s = row_solver(prob)
    pres_np, psc_np = nl.Se3LossProblem.from_problem(prob).prior_blocks()
    assert (psc_np < 1.0).any() and (psc_np == 1.0).any()
    pres = s.get_prior_residual()
    assert np.abs(pres - pres_np).max() <= 1e-13                              # the caller's order (the blocks differ by ~0.3)
    assert np.abs(pres[0] - pres[2]).max() > 1e-2
    o = po.PgOracle.from_problem(prob)
    c, _, _ = o.linearize()
    assert rel(pres, o.prior_residuals()) < 1e-13 and abs(s.compute_cost() - c) <= 1e-12 * c
    lam = 1e-4
    H, g = (x.copy() for x in s.get_hessian(lam))
    Ho, go = o.normal_equations()
    Ho += lam * np.eye(Ho.shape[0])
    assert rel(H, Ho) < 1e-12 and rel(g, go) < 1e-12
    col = prob.pose_col[41]
    assert rel(H[col:col + 6, col:col + 6], Ho[col:col + 6, col:col + 6]) < 1e-12 and rel(g[col:col + 6], go[col:col + 6]) < 1e-12
    # n = 0 removes them: the matrix of the same graph without priors, to the bit of a handle that never had any
    s.set_priors([])
    H0, g0 = (x.copy() for x in s.get_hessian(lam))
    bare = PoseGraphProblem(d, huber_delta=0.7)
    ob = po.PgOracle.from_problem(bare)
    ob.linearize()
    Hb, gb = ob.normal_equations()
    assert rel(H0, Hb + lam * np.eye(Hb.shape[0])) < 1e-12 and rel(g0, gb) < 1e-12
    assert np.abs(H0[col:col + 6, col:col + 6] - H[col:col + 6, col:col + 6]).max() > 0.5   # (three blocks of sc^2 <= 1 each left)
    t = row_solver(bare)
    Ht, gt = t.get_hessian(lam)
    assert np.array_equal(H0, Ht) and np.array_equal(g0, gt)
    s.close(); t.close()


# ---- 5. covariance and masks ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "jacobi"])
@pytest.mark.parametrize("name,prior", [("pg_sphere_8x12", False), ("pg_sphere_10x10_huber", True)])
def test_marginal_covariances_row_owned(name, prior, scaled):
    prob = pg_fixture(name, prior)
    s = row_solver(prob)
    if scaled:
        s.apply_column_scaling(1.0 / (1.0 + s.compute_column_norms()))
    for lam in (1e4, 1e-3):
        check_pg(s, prob, lam)
    s.close()


def test_fixed_components_keep_their_bits_after_a_committed_step():
    d = pkg.synthetic.make_sphere(12, 16, id_stride=3)
    fix = fm.pg_asymmetric(d.n_v, seed=63)
    fix[0, :] = 1; fix[100, :] = 1
    prob = fm.pg_apply_to_problem(PoseGraphProblem(d), fix)
    s = row_solver(prob)
    step = s.solve_augmented_equation(1e-3).copy()
    assert np.isfinite(step).all() and np.linalg.norm(step) > 0
    s.eval_step(); s.commit_step()
    got = s.get_parameters()
    full = fix.astype(bool).all(axis=1)
    assert full.sum() >= 2 and np.array_equal(got[full], d.poses[full])
    # a fixed tangent component: the applied step has nothing there (t' = t + R V rho moves t unless all of rho is fixed, so
    # the stored doubles of a partly fixed vertex may change; its tangent step in the fixed columns may not)
    applied = tc.applied_step(prob, d.poses, got)
    mask = tc.mask_vector(prob)
    assert np.abs(applied[mask]).max() <= 1e-12 and np.abs(applied[~mask]).max() > 1e-6
    free = ~full
    assert (np.abs(got[free] - d.poses[free]).max(axis=1) > 0).all()
    o = po.PgOracle.from_problem(prob)
    o.apply_step(step, 1.0)
    assert np.abs(got - o.get_params()).max() < 1e-9
    s.close()


# ---- 6. option semantics ----------------------------------------------------------------------------------------------------------
def _kind(call, *a):
    with pytest.raises(capi.LinAlgError) as e:
        call(*a)
    return e.value.kind


def _restructure(s):
    """apexgpu_pg_set_structure again on the same handle, with what initialize_structure gave it"""
    prob, h = s.problem, s._h
    d = prob.data
    ef = np.ascontiguousarray(d.e_from, dtype=np.uint32); et = np.ascontiguousarray(d.e_to, dtype=np.uint32)
    meas = np.ascontiguousarray(d.meas, dtype=np.float64)
    fix = np.ascontiguousarray(prob.fix, dtype=np.uint8); col = np.ascontiguousarray(prob.pose_col, dtype=np.int64)
    delta = -1.0 if prob.huber_delta is None else float(prob.huber_delta)
    h.check(h.L.apexgpu_pg_set_structure(h.h, capi.ptr(ef), capi.ptr(et), capi.ptr(meas), capi.ptr(col), capi.ptr(fix), delta))
    s.set_parameters(d.poses)


def test_option_values_and_names():
    d3 = pkg.synthetic.make_sphere(4, 6)
    s = GpuSparseCholeskySolver().initialize_structure(PoseGraphProblem(d3))
    s.set_option(OPT, 1); s.set_option(OPT, 0); s.set_option(OPT, 1)         # an SE3 handle takes both
    invalid = _kind(s.set_option, OPT, 2)
    assert _kind(s.set_option, OPT, -1) == invalid
    assert _kind(s.set_option, "row_owned_assembl", 1) == invalid and _kind(s.set_option, "row_owned_assemblyy", 1) == invalid
    assert _kind(s.set_option, "raw_owned_assembly", 1) == invalid
    s.close()
    c2 = pc.build("loops", "se2")
    s = GpuSparseCholeskySolver().initialize_structure(PoseGraphProblem(c2.d))
    s.set_parameters(c2.d.poses)
    H, g = (x.copy() for x in s.get_hessian(0.5))
    s.set_option(OPT, 1)                                                      # accepted, and nothing changes
    assert _kind(s.set_option, OPT, 0) == invalid
    _restructure(s)
    H1, g1 = s.get_hessian(0.5)
    assert np.array_equal(H, H1) and np.array_equal(g, g1)
    s.close()
    q = np.random.default_rng(2).standard_normal((5, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    m = np.random.default_rng(3).standard_normal((4, 4)); m /= np.linalg.norm(m, axis=1, keepdims=True)
    so3 = pkg.synthetic.PoseGraphData(ids=np.arange(5, dtype=np.int64), poses=q, e_from=np.arange(4, dtype=np.uint32),
                                      e_to=np.arange(1, 5, dtype=np.uint32), meas=m)
    s = GpuSparseCholeskySolver().initialize_structure(PoseGraphProblem(so3, manifold="so3"))
    s.set_option(OPT, 1)
    assert _kind(s.set_option, OPT, 0) == invalid
    s.close()
    with pytest.raises(capi.LinAlgError):                                     # refused before the structure as well
        GpuSparseCholeskySolver().with_option(OPT, 0).initialize_structure(PoseGraphProblem(c2.d))


def test_option_is_read_at_set_structure():
    """The 257 parallel edges: the row-owned matrix R is one fixed set of bits.  A handle structured under 0 and then given 1
    still scatters with atomics -- another order of the 257 sums and of every vertex's, so it does not return R -- until the
    next set_structure, after which it returns R itself, twice."""
    p = pc.policy("multi", "se3", "huber")
    c = pc.build("multi", "se3")
    r = row_solver(p.prob)
    R, gR = (x.copy() for x in r.get_hessian(pc.LAM))
    r.set_option(OPT, 0)                                                      # (and the other way round: still row-owned)
    R2, gR2 = r.get_hessian(pc.LAM)
    assert np.array_equal(R, R2) and np.array_equal(gR, gR2)
    r.close()
    s = GpuSparseCholeskySolver().initialize_structure(p.prob)
    s.set_parameters(c.d.poses)
    s.set_option(OPT, 1)
    A, gA = (x.copy() for x in s.get_hessian(pc.LAM))
    assert np.abs(A - R).max() <= 1e-9 * np.abs(R).max()
    assert not (np.array_equal(A, R) and np.array_equal(gA, gR))              # not in force yet
    _restructure(s)
    for _ in range(2):
        B, gB = s.get_hessian(pc.LAM)
        assert np.array_equal(B, R) and np.array_equal(gB, gR)
    s.close()
