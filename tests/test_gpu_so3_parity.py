"""SO3 pose graphs (rotation averaging) on the device, through the C ABI, against the long-double reference tests/so3_ref.py
(needs a real MI355X: `pytest -m gpu`).

Tolerances are those tests/test_gpu_se2_parity.py applies to the same quantities: r, J, J^T J, J^T r, cost <= 1e-12 relative,
prior residuals 1e-13, the step rel < 1e-10 where cond(H + lambda I) <= 1e5 (asserted on the reference's matrix; the step is
compared with a long-double solve of the reference's own H + lambda I), retractions rtol = atol = 1e-13."""
import ctypes as C

import numpy as np
import pytest

import so3_ref as sr
from apex_solver_amd import capi
from apex_solver_amd.pose_graph import GpuSparseCholeskySolver, PoseGraphProblem

pytestmark = pytest.mark.gpu

SHAPES = ("nv47", "nv48", "nv49", "nv97", "ne255", "ne256", "ne257", "loop", "multi", "isolated", "hub_lo", "hub_hi", "cross")


def rel(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def solver(prob, poses=None, **opts):
    s = GpuSparseCholeskySolver(0)
    for k, v in opts.items():
        s.with_option(k, v)
    s.initialize_structure(prob)
    s.set_parameters(prob.data.poses if poses is None else poses)
    return s


def test_handle_reports_its_manifold():
    d = sr.crafted("nv47")
    s = solver(PoseGraphProblem(d, manifold="so3"))
    out = (C.c_int * 3)()
    assert s._h.L.apexgpu_pg_manifold(s._h.h, C.byref(out)) == 0 and list(out) == [capi.MANIFOLD_SO3, 4, 3]
    assert s.info()["total_dof"] == 141 and s.get_parameters().shape == (47, 4)
    assert np.array_equal(s.get_parameters(), d.poses)                  # stored as given
    s.close()


@pytest.mark.parametrize("n_v,n_e", [(-1, 0), (0, 0), (4, -1)])
def test_bad_sizes_are_refused_at_set_structure(n_v, n_e):
    """with a device the handle is made (the sizes are checked when the structure is built, as for SE3 and SE2) and
    apexgpu_pg_set_structure answers INVALID_INPUT"""
    h = capi.PgHandle(n_v, n_e, 0, capi.MANIFOLD_SO3)
    z32 = np.zeros(4, np.uint32); meas = np.zeros((4, 4)); meas[:, 0] = 1.0; col = np.arange(4, dtype=np.int64) * 3
    with pytest.raises(capi.LinAlgError) as e:
        h.check(h.L.apexgpu_pg_set_structure(h.h, capi.ptr(z32), capi.ptr(z32), capi.ptr(meas), capi.ptr(col), None, -1.0))
    assert e.value.kind == "InvalidInput"
    h.close()


@pytest.mark.parametrize("shape", SHAPES)
def test_parity_with_the_reference(shape):
    d = sr.crafted(shape)
    opts = {}
    if shape == "cross":      # both directions across a tile boundary: stated on the caller's order, which the device keeps with the dissection off
        t = d.e_from.astype(int) // sr.VPT - d.e_to.astype(int) // sr.VPT
        assert (t > 0).any() and (t < 0).any()
        opts["nested_dissection"] = 0
    prob = PoseGraphProblem(d, manifold="so3").add_prior("x0", huber_delta=None)
    prob.add_prior(f"x{d.n_v - 1}", data=d.poses[d.n_v - 1] * 0.95 + 0.05, huber_delta=0.05)
    if shape == "isolated":                                            # a vertex no edge touches needs its own prior to be solvable
        prob.add_prior("x3").add_prior("x9")
    s = solver(prob, **opts)
    P = sr.So3Problem.from_problem(prob)
    r, J = P.edge_blocks()
    gr, gJ = s.get_residual(), s.get_jacobian_blocks()
    pr, _ = P.prior_blocks()
    print(shape, "r", rel(gr, r), "J", rel(gJ, J), "prior", rel(s.get_prior_residual(), pr))
    assert rel(gr, r) < 1e-12 and rel(gJ, J) < 1e-12
    assert rel(s.get_prior_residual(), pr) < 1e-13
    for lam in (0.0, 0.5):
        Hr, gr_, cost = P.dense(lam)
        H, g = s.get_hessian(lam)
        H2, g2 = s.get_hessian(lam)
        assert np.array_equal(H, H2) and np.array_equal(g, g2)          # two assemblies of one state: the same bits
        assert np.array_equal(H, H.T)
        print(shape, lam, "H", rel(H, sr.f64(Hr)), "g", rel(g, sr.f64(gr_)))
        assert rel(H, sr.f64(Hr)) < 1e-12 and rel(g, sr.f64(gr_)) < 1e-12
    c1, c2 = s.compute_cost(), s.compute_cost()
    assert c1 == c2 and c1 == pytest.approx(float(cost), rel=1e-12)
    for lam in (0.5, 10.0):
        Hr, gr_, _ = P.dense(0.0)
        cond = np.linalg.cond(sr.f64(Hr) + lam * np.eye(P.n))
        assert cond <= 1e5, cond
        want = sr.f64(sr.solve_ld(sr.f64(Hr), sr.f64(gr_), lam))
        step = s.solve_augmented_equation(lam)
        print(shape, lam, "cond", cond, "step", rel(step, want))
        assert rel(step, want) < 1e-10 and rel(s.get_gradient(), sr.f64(gr_)) < 1e-12
    s.close()


def test_un_normalised_input_and_small_and_large_residuals():
    """the per-edge cases of the host test on the device: every edge joins its own two vertices"""
    import manifold_ref as mr
    from test_so3_device_math_host import cases, literal_fp64

    cs = cases()
    k0, k1, m = (np.array([x[i] for x in cs]) for i in range(3))
    angle = np.array([x[3] for x in cs])
    d = mr.graph_of(dict(k0=k0, k1=k1, meas=m, angle=angle))
    s = solver(PoseGraphProblem(d, manifold="so3"))
    ro, Jo = sr.so3_between(k0, k1, m)
    e_r, e_J = mr.err(s.get_residual(), ro), mr.err(s.get_jacobian_blocks(), Jo)
    lit = [literal_fp64(k0[k], k1[k], m[k]) for k in range(len(cs))]
    o_r, o_J = mr.err(np.array([x[0] for x in lit]), ro), mr.err(np.array([x[1] for x in lit]), Jo)
    mr.report("so3 device", angle, r=e_r, J=e_J, r_fp64=o_r, J_fp64=o_J)
    below = mr.band_of(angle) < 4
    assert e_r[below].max() < 1e-13 and e_J[below].max() < 1e-12
    assert mr.referee(e_r[~below], o_r[~below], mr.FLOOR_R)[0] and mr.referee(e_J[~below], o_J[~below], mr.FLOOR_J)[0]
    s.close()


# ---- retraction, masks, the trial-step protocol --------------------------------------------------------------------------------
def test_commit_step_is_so3_plus_per_vertex_and_masks_hold():
    d = sr.crafted("nv97")
    prob = PoseGraphProblem(d, manifold="so3").add_prior("x0")
    prob.fix[5, :] = 1                                                  # fully fixed
    prob.fix[7, 1] = 1; prob.fix[60, 0] = 1; prob.fix[60, 2] = 1        # partially fixed
    poses = d.poses * np.linspace(0.9, 1.1, d.n_v)[:, None]             # stored un-normalised: the retraction keeps them so
    s = solver(prob, poses)
    p0 = s.get_parameters()
    assert np.array_equal(p0, poses)
    step = s.solve_augmented_equation(0.5).copy()
    P = sr.So3Problem.from_problem(prob, poses=p0)
    dd = np.where(prob.fix.astype(bool), 0.0, step[P.cols()])
    s.eval_step(); s.discard_step()
    assert np.array_equal(s.get_parameters(), p0)                       # a rejected trial step restores the parameters bit for bit
    step2 = s.solve_augmented_equation(0.5).copy()
    assert np.array_equal(step, step2)
    trial = s.eval_step(); s.commit_step()
    got = s.get_parameters()
    want = sr.f64(sr.so3_plus(p0, dd))
    print("retraction worst", np.abs(got - want).max())
    assert np.allclose(got, want, rtol=1e-13, atol=1e-13)
    assert np.array_equal(got[5], p0[5])                                # a fully fixed vertex keeps its bits
    assert not np.array_equal(got[6], p0[6])
    # a partially fixed vertex moves only in its free DOF: Log(x^-1 x') has zeros where the mask is set
    for v, fixed in ((7, [1]), (60, [0, 2])):
        back = sr.f64(sr.so3_log(sr._qmul(sr._qconj(sr.so3_from_vec(p0[v])), sr.so3_from_vec(got[v]))))[0]
        assert np.abs(back[fixed]).max() < 1e-15 and np.abs(np.delete(back, fixed)).max() > 1e-6
    P.poses = want
    assert trial == pytest.approx(P.cost(), rel=1e-12)
    s.close()


def test_rejected_step_restores_the_parameters_bit_for_bit():
    """A rejected trial step leaves an SO3 handle's parameters with the bits they had: the trial point lives in the other
    parameter set, so taking the step back is leaving the current set alone (TileBackend::keeps_current_on_discard).  SE3 and SE2 keep
    the reference's trial (+) (-step) (tests/test_gpu_step_protocol.py)."""
    d = sr.crafted("nv97")
    prob = PoseGraphProblem(d, manifold="so3").add_prior("x0")
    s = solver(prob)
    p0 = s.get_parameters()
    s.solve_augmented_equation(0.5)
    s.eval_step(); s.discard_step()
    p1 = s.get_parameters()
    print("vertices that moved", int((p1 != p0).any(axis=1).sum()), "of", d.n_v, "worst |p1 - p0|", np.abs(p1 - p0).max())
    s.close()
    assert np.array_equal(p1, p0)


def test_lm_runs_are_bit_reproducible():
    import apex_solver_amd as pkg
    from apex_solver_amd.solver import LevenbergMarquardt, LevenbergMarquardtConfig, LinearSolverType

    d = pkg.synthetic.make_rotation_graph(200, 6, 0.05, 2)
    prob = PoseGraphProblem.pose_graph(d, huber_delta=0.1)
    cfg = LevenbergMarquardtConfig.new().with_linear_solver_type(LinearSolverType.SparseCholesky).with_max_iterations(8)
    runs = [LevenbergMarquardt.with_config(cfg).optimize(prob) for _ in range(2)]
    assert np.array_equal(runs[0].history, runs[1].history) and np.array_equal(runs[0].parameters[0], runs[1].parameters[0])
    assert runs[0].final_cost < runs[0].initial_cost
