"""Per-DOF fixed variables (Problem::fix_variable, src/core/problem.rs:609-616; applied at problem.rs:185-197, 275-284: the
DOF stays in the linear system and is zeroed in the step when the step is applied) on the CPU: the two references the GPU
tests lean on -- the oracles' apply_step and the numpy restatements np_ref.retract / np_ref_pg.retract -- against each other
under the mask patterns of tests/fixed_masks.py (the same ones tests/test_gpu_fixed_dofs.py sets on the device), and the name
parsing of the two fix_variable mirrors.  The two restatements share no code (quaternions in C against rotation matrices in
numpy), so a mask dropped by either one shows as a difference of the size of the step."""
import numpy as np
import pytest

import apex_solver_amd as pkg
import fixed_masks as fm
import np_ref
import np_ref_pg
from apex_solver_amd.pose_graph import PoseGraphProblem
from apex_solver_amd.solver import OptimizationType, Problem

# numpy restatement against the oracle, poses: the matrix route (R Exp(theta), matrix -> quaternion, R V rho) is some tens of
# roundings of quantities of the size of the pose; 1e-12 relative / 1e-13 absolute is > 100 eps and eight orders below the
# steps applied here (1e-2 .. 1e-1), which is what a dropped mask would show
POSE_RTOL, POSE_ATOL = 1e-12, 1e-13

N_CAM, N_PT = 23, 300


def _ba_setup(oracle, m, seed):
    d = pkg.synthetic.make_problem(N_CAM, N_PT, 3, 6, config_id=77)
    lay = pkg.layout.reference_column_layout(d.n_cam, d.n_pt)
    o = oracle.OracleProblem(d.n_cam, d.n_pt, d.cam_idx, d.pt_idx, d.obs_uv, lay.intr_col, lay.pose_col, lay.pt_col,
                             mode="selfcal", huber_delta=1.0, fix_pose=m["pose"], fix_intr=m["intr"], fix_pt=m["pt"])
    o.set_params(d.poses, d.intr, d.points)
    rng = np.random.default_rng(seed)
    step = 0.05 * rng.standard_normal(lay.total_dof)
    return d, lay, o, step


def _unit(q):
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


BA_PATTERNS = {
    "random30": lambda: fm.random_mask(N_CAM, N_PT, seed=1),
    "asymmetric": lambda: fm.asymmetric(N_CAM, N_PT, seed=2),
    "one_pose_dof": lambda: fm.single(N_CAM, N_PT, "pose", N_CAM // 2, 4),
    "one_intr_dof": lambda: fm.single(N_CAM, N_PT, "intr", N_CAM - 1, 1),
    "one_pt_dof": lambda: fm.single(N_CAM, N_PT, "pt", N_PT - 1, 2),
    "all_landmarks": lambda: fm.all_of(N_CAM, N_PT, "pt"),
    "all_intrinsics": lambda: fm.all_of(N_CAM, N_PT, "intr"),
}


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("pattern", sorted(BA_PATTERNS))
def test_np_retract_matches_ba_oracle_apply_step(oracle, pattern, sign):
    m = BA_PATTERNS[pattern]()
    d, lay, o, step = _ba_setup(oracle, m, seed=11)
    norm = o.apply_step(step, sign)
    po, io, lo = o.get_params()
    pn, i_n, ln = np_ref.retract(d.poses, d.intr, d.points, step, lay, fix_pose=m["pose"], fix_intr=m["intr"], fix_pt=m["pt"], sign=sign)
    # intrinsics and points are ONE fp64 addition of sign * step (exact for sign = +-1): the same bits in both, and the input's
    # bits where the DOF is masked
    assert np.array_equal(io, i_n) and np.array_equal(lo, ln)
    fi, fp = m["intr"].astype(bool), m["pt"].astype(bool)
    assert np.array_equal(io[fi], d.intr[fi]) and np.array_equal(lo[fp], d.points[fp])
    si = sign * step[lay.intr_col[:, None] + np.arange(3)[None]]; sp_ = sign * step[lay.pt_col[:, None] + np.arange(3)[None]]
    assert np.array_equal(io[~fi], (d.intr + si)[~fi]) and np.array_equal(lo[~fp], (d.points + sp_)[~fp])
    assert (io[~fi] != d.intr[~fi]).all() and (lo[~fp] != d.points[~fp]).all()      # ... and every free DOF did move
    # poses: translation as is, rotation as a unit quaternion (the oracle stores the raw product)
    assert np.allclose(po[:, :3], pn[:, :3], rtol=POSE_RTOL, atol=POSE_ATOL)
    assert np.allclose(_unit(po[:, 3:]), pn[:, 3:], rtol=POSE_RTOL, atol=POSE_ATOL)
    # the returned norm is step.norm_l2() of the UNMASKED step (ora_apply_step), whatever is fixed
    assert norm == pytest.approx(np.linalg.norm(step), rel=1e-13)
    assert sum(fm.count(m).values()) > 0


@pytest.mark.parametrize("kind", ["pose", "intr", "pt"])
def test_each_ba_mask_matters_to_both_restatements(oracle, kind):
    """The comparison above has teeth for every one of the three masks: leaving one out of either side moves the result by
    the size of the step (so a restatement that drops a mask cannot pass it)."""
    m = fm.random_mask(N_CAM, N_PT, seed=1)
    d, lay, o, step = _ba_setup(oracle, m, seed=11)
    o.apply_step(step, 1.0)
    full = dict(zip(("pose", "intr", "pt"), o.get_params()))
    kw = {f"fix_{k}": (None if k == kind else m[k]) for k in m}
    dropped_np = dict(zip(("pose", "intr", "pt"), np_ref.retract(d.poses, d.intr, d.points, step, lay, **kw)))
    mm = dict(m); mm[kind] = np.zeros_like(m[kind])
    _, _, o2, _ = _ba_setup(oracle, mm, seed=11)
    o2.apply_step(step, 1.0)
    dropped_or = dict(zip(("pose", "intr", "pt"), o2.get_params()))
    for other in (dropped_np, dropped_or):
        a, b = full[kind], other[kind]
        if kind == "pose":
            a, b = a[:, :3], b[:, :3]
        assert np.abs(a - b).max() > 1e-3
    # and the numpy restatement without the mask is the oracle without the mask
    assert np.array_equal(dropped_np["intr"], dropped_or["intr"]) and np.array_equal(dropped_np["pt"], dropped_or["pt"])


def test_fully_masked_pose_is_the_zero_tangent_step(oracle):
    """All six DOF of a pose fixed: what comes back is se3_plus(pose, 0) -- the input's bits (q * (1, 0, 0, 0) and t + R 0 are
    exact), not a re-normalised or re-derived pose."""
    m = fm.empty(N_CAM, N_PT)
    cams = [0, 7, N_CAM - 1]
    for c in cams:
        m["pose"][c, :] = 1
    d, lay, o, step = _ba_setup(oracle, m, seed=12)
    poses = d.poses.copy(); poses[:, 3:] *= (1 + 1e-9 * np.arange(N_CAM))[:, None]      # un-normalised, as after a retraction
    o.set_params(poses, d.intr, d.points)
    o.apply_step(step, 1.0)
    po = o.get_params()[0]
    for c in cams:
        z = np.empty(7)
        oracle.lib().ora_se3_plus(np.ascontiguousarray(poses[c]), np.zeros(6), z)
        assert np.array_equal(po[c], z) and np.array_equal(po[c], poses[c])
    free = np.setdiff1d(np.arange(N_CAM), cams)
    assert (np.abs(po[free] - poses[free]).max(axis=1) > 1e-4).all()


# ---- pose graph -----------------------------------------------------------------------------------------------------------------
def _pg_setup(fix, seed):
    from oracle import pg_oracle as po

    d = pkg.synthetic.make_sphere(6, 9, id_stride=3)
    prob = PoseGraphProblem(d, fix=fix.copy())
    o = po.PgOracle.from_problem(prob)
    rng = np.random.default_rng(seed)
    step = 0.05 * rng.standard_normal(6 * d.n_v)
    return d, prob, o, step


PG_PATTERNS = {
    "random30": lambda n: fm.pg_random(n, seed=3),
    "asymmetric": lambda n: fm.pg_asymmetric(n, seed=4),
    "one_dof_middle": lambda n: fm.pg_single(n, n // 2, 4),
    "one_dof_last": lambda n: fm.pg_single(n, n - 1, 0),
}


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("pattern", sorted(PG_PATTERNS))
def test_np_retract_matches_pg_oracle_apply_step(pattern, sign):
    fix = PG_PATTERNS[pattern](54)
    d, prob, o, step = _pg_setup(fix, seed=13)
    o.apply_step(step, sign)
    po_ = o.get_params()
    pn = np_ref_pg.retract(d.poses, step, prob.pose_col, fix=fix, sign=sign)
    assert np.allclose(po_[:, :3], pn[:, :3], rtol=POSE_RTOL, atol=POSE_ATOL)
    assert np.allclose(_unit(po_[:, 3:]), pn[:, 3:], rtol=POSE_RTOL, atol=POSE_ATOL)
    # dropping the mask on the numpy side is visible at the size of the step
    pd = np_ref_pg.retract(d.poses, step, prob.pose_col, fix=None, sign=sign)
    assert not np.allclose(po_[:, :3], pd[:, :3], rtol=1e-6, atol=1e-6) or not np.allclose(_unit(po_[:, 3:]), pd[:, 3:], rtol=1e-6, atol=1e-6)


def test_fully_masked_vertex_is_the_zero_tangent_step():
    from oracle import pg_oracle as po

    fix = fm.pg_empty(54)
    fix[[0, 20, 53], :] = 1
    d, prob, o, step = _pg_setup(fix, seed=14)
    o.apply_step(step, 1.0)
    p = o.get_params()
    for v in (0, 20, 53):
        z = po.call("pgo_se3_plus", np.ascontiguousarray(d.poses[v]), np.zeros(6), out_shape=(7,))
        assert np.array_equal(p[v], d.poses[v]) and np.array_equal(p[v], np.ravel(z))
    free = np.setdiff1d(np.arange(54), [0, 20, 53])
    assert (np.abs(p[free] - d.poses[free]).max(axis=1) > 1e-4).all()


# ---- fix_variable: names to rows and columns ---------------------------------------------------------------------------------
def test_ba_fix_variable_names_hit_the_right_row_and_column(oracle):
    """`pose_{i:04}`, `intr_{i:04}`, `pt_{j:05}` (bin/bundle_adjustment.rs naming), indices of 1000 and more included: exactly
    one byte of exactly one mask is set, and it is the DOF whose global column the layout gives -- a step that is nonzero in
    that one column alone leaves the oracle's parameters untouched, and moves them without the mask."""
    d = pkg.synthetic.make_problem(1030, 1300, 3, 3, config_id=78)
    cases = [("pose", 12, 4, "pose_0012"), ("pose", 1003, 1, "pose_1003"), ("intr", 7, 2, "intr_0007"), ("intr", 1029, 0, "intr_1029"),
             ("pt", 5, 1, "pt_00005"), ("pt", 1000, 2, "pt_01000"), ("pt", 1299, 0, "pt_01299")]
    for kind, idx, dof, name in cases:
        prob = Problem(d, OptimizationType.SelfCalibration, 1.0)
        prob.fix_variable(name, dof)
        masks = {"pose": prob.fix_pose, "intr": prob.fix_intr, "pt": prob.fix_pt}
        want = fm.single(d.n_cam, d.n_pt, kind, idx, dof)
        for k in masks:
            assert np.array_equal(masks[k], want[k]), (name, k)
        lay = prob.layout
        col = {"pose": lay.pose_col, "intr": lay.intr_col, "pt": lay.pt_col}[kind][idx] + dof
        step = np.zeros(lay.total_dof); step[col] = 0.25
        for fixed in (True, False):
            mk = masks if fixed else fm.empty(d.n_cam, d.n_pt)
            o = oracle.OracleProblem(d.n_cam, d.n_pt, d.cam_idx, d.pt_idx, d.obs_uv, lay.intr_col, lay.pose_col, lay.pt_col,
                                     mode="selfcal", huber_delta=1.0, fix_pose=mk["pose"], fix_intr=mk["intr"], fix_pt=mk["pt"])
            o.set_params(d.poses, d.intr, d.points)
            o.apply_step(step, 1.0)
            same = all(np.array_equal(a, b) for a, b in zip(o.get_params(), (d.poses, d.intr, d.points)))
            assert same == fixed, (name, fixed)
    # Problem.bundle_adjustment is fix_variable("pose_0000", 0..5)
    g = Problem.bundle_adjustment(d)
    assert np.array_equal(g.fix_pose, fm.with_gauge(fm.empty(d.n_cam, d.n_pt))["pose"]) and not g.fix_intr.any() and not g.fix_pt.any()
    # fixed_masks.apply_to_problem goes through the names and reproduces the arrays
    small = pkg.synthetic.make_problem(N_CAM, N_PT, 3, 6, config_id=77)
    m = fm.random_mask(N_CAM, N_PT, seed=1)
    p = fm.apply_to_problem(Problem(small), m)
    assert np.array_equal(p.fix_pose, m["pose"]) and np.array_equal(p.fix_intr, m["intr"]) and np.array_equal(p.fix_pt, m["pt"])
    for bad in ("cam_0001", "x12", "landmark_00001", "pose_5000"):
        with pytest.raises((KeyError, ValueError, IndexError)):
            Problem(d).fix_variable(bad, 0)


def test_pg_fix_variable_names_hit_the_right_row_and_column():
    """`x<id>` names the vertex by its ID: with strided ids (0, 3, 6, ...) the row is id / 3 and the columns are those of the
    sorted-NAME order ("x1002" sorts before "x3"), which pose_graph_columns gives."""
    from oracle import pg_oracle as po

    d = pkg.synthetic.make_sphere(20, 30, id_stride=3)           # ids 0 .. 1797
    assert d.ids[1] == 3 and d.ids.max() >= 1000
    for row, dof in ((1, 2), (334, 5), (599, 0), (17, 3)):
        prob = PoseGraphProblem(d)
        prob.fix_variable(f"x{int(d.ids[row])}", dof)
        assert np.array_equal(prob.fix, fm.pg_single(d.n_v, row, dof))
        step = np.zeros(6 * d.n_v); step[prob.pose_col[row] + dof] = 0.25
        for fixed in (True, False):
            o = po.PgOracle(d.e_from, d.e_to, d.meas, prob.pose_col, prob.fix if fixed else None, None, d.poses)
            o.apply_step(step, 1.0)
            assert np.array_equal(o.get_params(), d.poses) == fixed
    assert int(d.ids[334]) >= 1000
    assert np.array_equal(PoseGraphProblem.pose_graph(d).fix, np.vstack([np.ones((1, 6), np.uint8), fm.pg_empty(d.n_v - 1)]))
    m = fm.pg_random(d.n_v, seed=5)
    assert np.array_equal(fm.pg_apply_to_problem(PoseGraphProblem(d), m).fix, m)
    for bad in ("x1", "x1798", "y3", "pose_0003"):               # 1 is no id under stride 3; 1798 is past the last one
        with pytest.raises((KeyError, ValueError)):
            PoseGraphProblem(d).fix_variable(bad, 0)
