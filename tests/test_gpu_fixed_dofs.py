"""Per-DOF fixed variables on every device path that applies a step (needs a real MI355X: `pytest -m gpu`).

A fixed DOF (Problem::fix_variable, src/core/problem.rs:609-616) stays in the linear system and is zeroed in the step when
the step is applied (problem.rs:185-197, 275-284).  The masks arrive in the caller's numbering and live on the device in the
internal one (cameras: nested dissection / border-last order; landmarks: the rank-local order of a tree-sharded handle;
pose-graph vertices: the tile permutation), and five kernels read them: k_retract_cams<6|9>, k_retract_points (sign +1 and
the sign -1 of discard_step), the eager write of the trial points inside k_back_substitute, and k_pg_retract.

The reference in every case is the oracle APPLYING THE DEVICE'S OWN EXPORTED STEP under the same masks, so the conditioning
of the solve does not enter: points and intrinsics are one fp64 addition (bit equality), poses are se3_plus of the masked
tangent (the tolerance of tests/test_device_math_host.py::test_se3_plus_matches_oracle), the trial cost is compute_cost at
identical parameters (1e-13).  The mask patterns come from tests/fixed_masks.py, which tests/test_fixed_dofs_host.py checks on
the CPU (oracle against a numpy restatement).

Which form of the back-substitution runs where (the handle does not tell; csrc/ba_kernels.hip, rec_form_ok): a solve in the
BundleAdjustment and SelfCalibration modes always reads the projection records its own assembly has just written (the record
form, k_back_substitute<DC, false, true>), first solve, solve after a commit and solve after a discard alike; the modes with
constant blocks (OnlyLandmarks, LandmarksAndIntrinsics, ...) run the non-record form (k_back_substitute<DC, false, false>).
Both are run below with "eager_step_eval" 1 (the kernel writes the trial points itself) and 0 (k_retract_points does)."""
import numpy as np
import pytest

import apex_solver_amd as pkg
import fixed_masks as fm
from apex_solver_amd.pose_graph import GpuSparseCholeskySolver, PoseGraphProblem
from apex_solver_amd.solver import (GpuSchurComplementSolver, LevenbergMarquardt, LevenbergMarquardtConfig, LinearSolverType,
                                    OptimizationType, Problem, SchurVariant)
from test_gpu_parity import STEP_FORWARD_BOUND, _custom, rel

pytestmark = pytest.mark.gpu

OT = {"ba": OptimizationType.BundleAdjustment, "selfcal": OptimizationType.SelfCalibration,
      "only_landmarks": OptimizationType.OnlyLandmarks, "pose_and_intrinsics": OptimizationType.PoseAndIntrinsics,
      "landmarks_and_intrinsics": OptimizationType.LandmarksAndIntrinsics}
SE3_RTOL, SE3_ATOL = 1e-13, 1e-15       # tests/test_device_math_host.py::test_se3_plus_matches_oracle
COST_RTOL = 1e-13                        # compute_cost at identical parameters (test_gpu_parity.py)
ATOMIC_ASSEMBLY_BOUND = 1e-13            # test_device_built_pair_list_is_the_host_list: blocks that add atomically


def device(d, m, mode="selfcal", variant=SchurVariant.Sparse, options=None, shard=None):
    prob = fm.apply_to_problem(Problem(d, OT[mode], 1.0), m)
    s = GpuSchurComplementSolver(0).with_variant(variant)
    if shard:
        s.with_shard(*shard)
    for k, v in (options or {}).items():
        s.with_option(k, v)
    s.initialize_structure(prob)
    s.set_parameters(d.poses, d.intr, d.points)
    return prob, s


def oracle_of(ora, d, prob, mode, params=None):
    lay = prob.layout
    o = ora.OracleProblem(d.n_cam, d.n_pt, d.cam_idx, d.pt_idx, d.obs_uv, lay.intr_col, lay.pose_col, lay.pt_col, mode=mode,
                          huber_delta=1.0, fix_pose=prob.fix_pose, fix_intr=prob.fix_intr, fix_pt=prob.fix_pt)
    o.set_params(*(params or (d.poses, d.intr, d.points)))
    return o


def cols(col, w):
    return col[:, None] + np.arange(w)[None]


def check_applied(ora, d, prob, mode, step, got, start=None, tag="", exact=True):
    """`got` = the device's parameters after its step `step` was applied from `start`: against the oracle applying the same
    step under the same masks, and against the plain statement of the masked addition.  exact=False (Jacobi scaling): the
    device holds the unscaled step d, exports y = d / s and the caller forms y * s -- two roundings away from d (relative
    2^-52 at most), then the addition rounds once: |got - (p + y s)| <= 2^-52 (|d| + |p + d|); masked DOF stay bit-exact."""
    start = start or (d.poses, d.intr, d.points)
    o = oracle_of(ora, d, prob, mode, start)
    norm = o.apply_step(step, 1.0)
    po, io, lo = o.get_params()
    pg, ig, lg = got
    lay = prob.layout
    fi, fp, fq = prob.fix_intr.astype(bool), prob.fix_pt.astype(bool), prob.fix_pose.astype(bool)
    di, dp = step[cols(lay.intr_col, 3)], step[cols(lay.pt_col, 3)]
    bad_pose = np.abs(pg - po) - (SE3_ATOL + SE3_RTOL * np.abs(po))
    print(tag, "masked DOF", fm.count({"pose": prob.fix_pose, "intr": prob.fix_intr, "pt": prob.fix_pt}),
          "pose worst |gpu - oracle|", float(np.abs(pg - po).max()), "worst excess over the se3_plus tolerance", float(bad_pose.max()),
          "points differing from the oracle", int((lg != lo).sum()), "intrinsics differing", int((ig != io).sum()))
    # points and intrinsics: p where masked, p + d where not, the same bits
    assert np.array_equal(lg[fp], start[2][fp]) and np.array_equal(ig[fi], start[1][fi])
    if exact:
        assert np.array_equal(lg[~fp], (start[2] + dp)[~fp]) and np.array_equal(ig[~fi], (start[1] + di)[~fi])
        assert np.array_equal(lg, lo) and np.array_equal(ig, io)
    else:
        for g_, p_, d_, f_, o_ in ((lg, start[2], dp, fp, lo), (ig, start[1], di, fi, io)):
            want = p_ + d_
            print(tag, "worst |got - (p + d)| in units of the two-rounding bound", float((np.abs(g_ - want) / (2.0 ** -52 * (np.abs(d_) + np.abs(want))))[~f_].max()))
            assert (np.abs(g_ - want) <= 2.0 ** -52 * (np.abs(d_) + np.abs(want)))[~f_].all()
            assert (np.abs(g_ - o_) <= 2.0 ** -52 * (np.abs(d_) + np.abs(want))).all()
    # poses: se3_plus of the masked tangent; a pose with all six DOF fixed comes back with its own bits (q * (1, 0, 0, 0) and
    # t + R 0 are exact in any evaluation order), as from the oracle
    assert np.allclose(pg, po, rtol=SE3_RTOL, atol=SE3_ATOL), float(bad_pose.max())
    full = fq.all(axis=1)
    assert np.array_equal(pg[full], po[full]) and np.array_equal(pg[full], start[0][full])
    return o, norm


def full_case(ora, d, m, mode="selfcal", variant=SchurVariant.Sparse, options=None, lam=1e-3, bitwise=True, scaling=False, tag=""):
    """Everything one handle can show about a mask: the step and its statistics are those of the unmasked problem, a rejected
    step comes back, an accepted one lands where the oracle puts it, the trial cost is the cost there."""
    prob, s = device(d, m, mode, variant, options)
    _, s0 = device(d, fm.empty(d.n_cam, d.n_pt), mode, variant, options)
    scal = None
    if scaling:
        scal = 1.0 / (1.0 + s0.compute_column_norms())
        s.apply_column_scaling(scal); s0.apply_column_scaling(scal)
    y = s.solve_augmented_equation(lam).copy()
    y0 = s0.solve_augmented_equation(lam).copy()
    s0.close()
    # ---- the step is the unmasked one
    print(tag, mode, variant.name, options, "step under the mask vs without: rel", rel(y, y0), "bitwise", np.array_equal(y, y0))
    if bitwise:
        assert np.array_equal(y, y0)
    else:
        assert rel(y, y0) < ATOMIC_ASSEMBLY_BOUND
    ex, _ = s.export_step()
    assert np.array_equal(ex, y)
    step = y if scal is None else s.apply_inverse_scaling(y)      # what is applied: the UNSCALED step
    gn, sn, pred = s.step_stats()
    assert sn == pytest.approx(np.linalg.norm(step), rel=1e-8)    # |step| of the unmasked step (tolerance: test_gpu_parity.py)
    # ---- reject round trip: the inverse retraction under the same mask
    s.eval_step(); s.discard_step()
    pg, ig, lg = s.get_parameters()
    fi, fp = prob.fix_intr.astype(bool), prob.fix_pt.astype(bool)
    assert np.array_equal(ig[fi], d.intr[fi]) and np.array_equal(lg[fp], d.points[fp])
    o = oracle_of(ora, d, prob, mode)
    o.apply_step(step, 1.0); o.apply_step(step, -1.0)
    po, io, lo = o.get_params()
    assert rel(pg, po) < 1e-12 and rel(lg, lo) < 1e-12 and rel(ig, io) < 1e-12      # test_rejected_step_round_trip
    assert np.abs(lg - d.points).max() < 1e-12
    # a following solve: the same step (the parameters moved by roundings only; two solves of such neighbours are held to the
    # forward bound every step comparison of test_gpu_parity.py uses)
    y2 = s.solve_augmented_equation(lam).copy()
    print(tag, "step after the round trip vs before", rel(y2, y))
    assert rel(y2, y) < STEP_FORWARD_BOUND
    # ---- accept: from the parameters the round trip left, the step of THIS solve
    start = (pg, ig, lg)
    step2 = y2 if scal is None else s.apply_inverse_scaling(y2)
    trial = s.eval_step()
    s.commit_step()
    got = s.get_parameters()
    o2, norm = check_applied(ora, d, prob, mode, step2, got, start, tag, exact=scal is None)
    assert s.compute_cost() == pytest.approx(trial, rel=COST_RTOL)
    o2.set_params(*got)
    ocost = o2.residuals()[0]
    print(tag, "trial cost rel", abs(trial - ocost) / ocost)
    assert trial == pytest.approx(ocost, rel=COST_RTOL)
    s.close()
    return got


def ragged(n_cam=320):
    """Landmarks with 0, 1 and far more than 8 observations (the chunked path), a duplicated camera, and 300 ordinary ones."""
    rng = np.random.default_rng(9)
    lists = [[], [3], [5, 5, 9], list(range(64)), list(range(65)), list(range(40, 169)), list(range(200)), [7, 8, 7, 8, 100]]
    lists += [sorted(rng.choice(n_cam, size=int(rng.integers(2, 12)), replace=False).tolist()) for _ in range(300)]
    return _custom(n_cam, len(lists), lists), lists


# ---- single DOF of one variable ------------------------------------------------------------------------------------------------
SINGLES = [("pose", "mid", 4), ("pose", "last", 1), ("intr", "mid", 1), ("intr", "last", 2), ("pt", "last", 2), ("pt", "mid", 0)]


@pytest.mark.parametrize("kind,where,dof", SINGLES, ids=[f"{k}-{w}-{a}" for k, w, a in SINGLES])
def test_single_fixed_dof(oracle, kind, where, dof):
    """One byte in one mask, on top of the gauge; 300 cameras (not a multiple of 256), 7001 landmarks (not one of 128): a
    shifted, permuted or transposed index fixes another DOF, which the bit comparison of every parameter shows."""
    d = pkg.synthetic.make_problem(300, 7001, 3, 8, config_id=311)
    n = d.n_cam if kind != "pt" else d.n_pt
    idx = n - 1 if where == "last" else n // 2 + 3
    m = fm.with_gauge(fm.single(d.n_cam, d.n_pt, kind, idx, dof))
    full_case(oracle, d, m, tag=f"single {kind}[{idx},{dof}]")


@pytest.mark.parametrize("mode", ["selfcal", "ba"])
def test_single_fixed_dof_of_ragged_landmarks(oracle, mode):
    """One coordinate each of a landmark nobody sees, one seen once, one seen by 200 cameras (chunked), one seen twice by the
    same camera and the last one; duplicated cameras and the 200-camera blocks add atomically: the step under the mask is
    held to that rounding bound instead of bit equality."""
    d, lists = ragged()
    m = fm.with_gauge(fm.empty(d.n_cam, d.n_pt))
    for l, a in ((0, 1), (1, 2), (6, 0), (2, 1), (d.n_pt - 1, 2)):
        m["pt"][l, a] = 1
    assert len(lists[0]) == 0 and len(lists[1]) == 1 and len(lists[6]) > 8
    full_case(oracle, d, m, mode=mode, bitwise=False, tag="ragged")


# ---- asymmetric and dense patterns ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["asymmetric", "random30", "all_landmarks", "all_intrinsics"])
@pytest.mark.parametrize("mode", ["selfcal", "ba"])
def test_mask_patterns(oracle, mode, pattern):
    d = pkg.synthetic.make_problem(130, 4000 + 37, 3, 9, config_id=312)
    m = {"asymmetric": lambda: fm.asymmetric(d.n_cam, d.n_pt, seed=21), "random30": lambda: fm.random_mask(d.n_cam, d.n_pt, seed=22),
         "all_landmarks": lambda: fm.all_of(d.n_cam, d.n_pt, "pt"), "all_intrinsics": lambda: fm.all_of(d.n_cam, d.n_pt, "intr")}[pattern]()
    full_case(oracle, d, fm.with_gauge(m), mode=mode, tag=pattern)


@pytest.mark.parametrize("hubs_last", [1, 0])
@pytest.mark.parametrize("nd", [1, 0])
def test_masks_on_hub_and_border_cameras(oracle, hubs_last, nd):
    """The "-hub" generator: cameras seen from anywhere go last in the internal order ("hubs_last" 1) and nested dissection
    permutes the rest, so the internal camera order is far from the caller's.  Asymmetric masks on the cameras with the most
    observations (the hubs), on a handful of others and on the landmarks the hubs see."""
    d = pkg.synthetic.make_problem(640, 16000, 3, 8, config_id=97, window=16, hub_frac=0.04, hub_obs_prob=0.04, long_range_prob=3e-4)
    per_cam = np.bincount(d.cam_idx, minlength=d.n_cam)
    hubs = np.argsort(-per_cam)[:12]
    others = np.array([1, 17, 333, 639])
    pts = np.unique(d.pt_idx[np.isin(d.cam_idx, hubs[:3])])[:50]
    m = fm.with_gauge(fm.on_variables(d.n_cam, d.n_pt, cams=np.concatenate([hubs, others]), pts=pts, seed=5))
    prob, s = device(d, m, options={"hubs_last": hubs_last, "nested_dissection": nd})
    print("hub cameras", s.setup_times()["hub_cameras"], "levels", s.info()["etree_levels"])
    if hubs_last:
        assert s.setup_times()["hub_cameras"] > 0
    s.close()
    full_case(oracle, d, m, options={"hubs_last": hubs_last, "nested_dissection": nd}, tag=f"hub hubs_last={hubs_last} nd={nd}")


# ---- the paths that write the trial point --------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [SchurVariant.Sparse, SchurVariant.Iterative, SchurVariant.Implicit], ids=lambda v: v.name)
@pytest.mark.parametrize("mode", ["selfcal", "only_landmarks"], ids=["record-form", "non-record-form"])
def test_eager_and_on_request_paths_commit_the_same_point(oracle, mode, variant):
    """ "eager_step_eval" 1: k_back_substitute writes the trial points under fix_pt itself and k_retract_cams runs behind it;
    0: eval_step runs k_retract_cams and k_retract_points.  Record form (SelfCalibration) and non-record form (OnlyLandmarks)
    of the back-substitution (module docstring), first solve and the solve after a committed step, each Schur variant; every
    point against the oracle from the handle's own exported step, masked DOF untouched in all of them, and the two paths
    against each other."""
    d = pkg.synthetic.make_problem(14, 900 + 5, 3, 8, config_id=33)
    m = fm.with_gauge(fm.random_mask(d.n_cam, d.n_pt, seed=31))
    out = {}
    for eager in (1, 0):
        prob, s = device(d, m, mode, variant, options={"eager_step_eval": eager})
        if variant == SchurVariant.Implicit:
            s.with_cg_params(500, 1e-9)
        start = (d.poses, d.intr, d.points)
        seq = []
        for k in range(2):          # k = 0: the first solve of the handle; k = 1: the solve after a committed step
            step = s.solve_augmented_equation(1e-3).copy()
            assert np.array_equal(s.export_step()[0], step)
            trial = s.eval_step(); s.commit_step()
            got = s.get_parameters()
            o, _ = check_applied(oracle, d, prob, mode, step, got, start, tag=f"eager={eager} {mode} {variant.name} solve {k}")
            o.set_params(*got)
            assert trial == pytest.approx(o.residuals()[0], rel=COST_RTOL)
            seq.append((step, got)); start = got
        fp, fi, fq = prob.fix_pt.astype(bool), prob.fix_intr.astype(bool), prob.fix_pose.astype(bool)
        assert np.array_equal(start[2][fp], d.points[fp]) and np.array_equal(start[1][fi], d.intr[fi])      # after two steps
        assert np.array_equal(start[0][fq.all(axis=1)], d.poses[fq.all(axis=1)])
        out[eager] = seq
        s.close()
    # the same first step either way (the option changes who applies it, not the solve), so the same committed point
    if variant == SchurVariant.Sparse:
        assert np.array_equal(out[1][0][0], out[0][0][0])
        for a, b in zip(out[1][0][1], out[0][0][1]):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("mode", ["only_landmarks", "pose_and_intrinsics", "landmarks_and_intrinsics"])
def test_masks_inside_the_optimised_blocks_of_the_partial_modes(oracle, mode):
    d = pkg.synthetic.make_problem(40, 2000 + 11, 3, 7, config_id=521)
    m = fm.with_gauge(fm.asymmetric(d.n_cam, d.n_pt, seed=41))
    full_case(oracle, d, m, mode=mode, lam=1e-2, tag=mode)


def test_masks_under_jacobi_scaling(oracle):
    """The solve returns the SCALED step; the mask applies to the unscaled one (apply_inverse_scaling, then the retraction)."""
    d = pkg.synthetic.make_problem(40, 2000 + 11, 3, 7, config_id=240)
    m = fm.with_gauge(fm.asymmetric(d.n_cam, d.n_pt, seed=42))
    full_case(oracle, d, m, scaling=True, tag="jacobi scaling")


# ---- the LM loop ---------------------------------------------------------------------------------------------------------------
def test_lm_loop_under_an_asymmetric_mask(oracle):
    """apexgpu_lm_optimize against the oracle's loop with the same masks: status, iteration count, accept pattern, costs and
    damping within the tolerances of test_golden_lm_history / test_lm_converges_like_reference_integration_test; every masked
    DOF of the final parameters is the initial value's bits (rejected steps included: the inverse retraction is masked too)."""
    d = pkg.synthetic.make_problem(21, 1100, 3, 8, config_id=21)
    m = fm.with_gauge(fm.asymmetric(d.n_cam, d.n_pt, seed=51, n_pose=5, n_intr=6, n_ptv=60))
    prob = fm.apply_to_problem(Problem(d, OptimizationType.SelfCalibration, 1.0), m)
    res = LevenbergMarquardt.with_config(LevenbergMarquardtConfig().with_max_iterations(12)).optimize(prob)
    o = oracle_of(oracle, d, prob, "selfcal")
    ores = o.optimize(oracle.LMConfig.default(max_iterations=12))
    print(res.status, res.iterations, res.final_cost, "| oracle", ores.status, ores.iterations, ores.final_cost)
    assert res.status.name == ores.status and res.iterations == ores.iterations
    assert np.array_equal(res.history[:, 3], ores.history[:, 3])
    assert np.allclose(res.history[:, 0], ores.history[:, 0], rtol=1e-7)
    assert np.allclose(res.history[:, 1], ores.history[:, 1], rtol=1e-4)
    assert res.final_cost == pytest.approx(ores.final_cost, rel=1e-6) and res.final_cost < res.initial_cost
    pg, ig, lg = res.parameters
    fq, fi, fp = m["pose"].astype(bool), m["intr"].astype(bool), m["pt"].astype(bool)
    assert np.array_equal(ig[fi], d.intr[fi]) and np.array_equal(lg[fp], d.points[fp])
    assert np.array_equal(pg[0], d.poses[0])                     # all six DOF fixed: the pose itself
    assert (ig[~fi] != d.intr[~fi]).all() and (lg[~fp] != d.points[~fp]).mean() > 0.99
    # and the unmasked loop goes elsewhere
    res0 = LevenbergMarquardt.with_config(LevenbergMarquardtConfig().with_max_iterations(12)).optimize(Problem.bundle_adjustment(d))
    assert not np.array_equal(res0.parameters[2][fp], d.points[fp])


# ---- pose graph ----------------------------------------------------------------------------------------------------------------
def pg_case(d, fix, nd=None, priors=False, tag=""):
    from oracle import pg_oracle as po

    def build(fx):
        prob = fm.pg_apply_to_problem(PoseGraphProblem(d, huber_delta=0.7 if priors else None), fx)
        if priors:
            prob.add_prior(f"x{int(d.ids[0])}", huber_delta=1.0)
            prob.add_prior(f"x{int(d.ids[77])}", huber_delta=None)
        s = GpuSparseCholeskySolver()
        if nd is not None:
            s.with_option("nested_dissection", nd)
        s.initialize_structure(prob)
        s.set_parameters(d.poses)
        return prob, s

    prob, s = build(fix)
    _, s0 = build(fm.pg_empty(d.n_v))
    step = s.solve_augmented_equation(1e-3).copy()
    step0 = s0.solve_augmented_equation(1e-3).copy()
    s0.close()
    print(tag, "pose-graph step under the mask vs without: rel", rel(step, step0), "bitwise", np.array_equal(step, step0))
    assert rel(step, step0) < ATOMIC_ASSEMBLY_BOUND               # (the edge blocks of H add atomically: no fixed order)
    assert s.step_stats()[1] == pytest.approx(np.linalg.norm(step), rel=1e-8)
    # reject round trip (test_rejected_step_and_fixed_vertex: 1e-9), then the same solve again
    s.eval_step(); s.discard_step()
    p1 = s.get_parameters()
    assert np.abs(p1 - d.poses).max() < 1e-9
    full = fix.astype(bool).all(axis=1)
    assert np.array_equal(p1[full], d.poses[full])
    step2 = s.solve_augmented_equation(1e-3).copy()
    assert rel(step2, step) < 1e-8                                # (the forward bound of the pose-graph step comparisons)
    trial = s.eval_step(); s.commit_step()
    got = s.get_parameters()
    o = po.PgOracle.from_problem(prob)
    o.set_params(p1)
    o.apply_step(step2, 1.0)
    ref = o.get_params()
    excess = np.abs(got - ref) - (SE3_ATOL + SE3_RTOL * np.abs(ref))
    print(tag, "masked DOF", int(fix.sum()), "worst |gpu - oracle|", float(np.abs(got - ref).max()), "excess over the se3_plus tolerance", float(excess.max()))
    assert np.allclose(got, ref, rtol=SE3_RTOL, atol=SE3_ATOL)
    assert np.array_equal(got[full], ref[full]) and np.array_equal(got[full], d.poses[full])
    o.set_params(got)
    assert trial == pytest.approx(o.residuals()[0], rel=COST_RTOL)
    s.close()
    return step, got


PG_MASKS = {"single-middle": lambda n: fm.pg_single(n, n // 2 + 1, 4), "single-last": lambda n: fm.pg_single(n, n - 1, 0),
            "asymmetric": lambda n: fm.pg_asymmetric(n, seed=61), "random30": lambda n: fm.pg_random(n, seed=62)}


@pytest.mark.parametrize("priors", [False, True], ids=["gauge-by-damping", "priors"])
@pytest.mark.parametrize("pattern", sorted(PG_MASKS))
def test_pose_graph_fixed_dofs(pattern, priors):
    """600 vertices with strided ids (25 tiles, not a multiple of 24 vertices per tile row, nested dissection active): the
    tile permutation is far from the identity and the names `x<id>` are not the rows.  Nested dissection off: the same step
    bits are not required (another elimination order), the same committed point within the step's forward bound is."""
    d = pkg.synthetic.make_sphere(20, 30, id_stride=3)
    fix = PG_MASKS[pattern](d.n_v)
    if pattern == "asymmetric":
        fix[5, :] = 1                                             # and one vertex, not the first, with all six DOF
    step, got = pg_case(d, fix, priors=priors, tag=f"pg {pattern}")
    step_n, got_n = pg_case(d, fix, nd=0, priors=priors, tag=f"pg {pattern} nd=0")
    assert rel(step_n, step) < 1e-8 and np.abs(got_n - got).max() < 1e-8 * max(1.0, np.abs(got).max())
    full = fix.astype(bool).all(axis=1)
    assert np.array_equal(got_n[full], got[full])


def test_pose_graph_lm_loop_under_a_mask():
    from oracle import pg_oracle as po

    d = pkg.synthetic.make_sphere(12, 16, id_stride=3)
    fix = fm.pg_asymmetric(d.n_v, seed=63)
    fix[0, :] = 1; fix[100, :] = 1
    prob = fm.pg_apply_to_problem(PoseGraphProblem(d), fix)
    cfg = LevenbergMarquardtConfig.new().with_max_iterations(30).with_linear_solver_type(LinearSolverType.SparseCholesky)
    res = LevenbergMarquardt.with_config(cfg).optimize(prob)
    ref = po.PgOracle.from_problem(prob).lm_optimize(po.lm_config(max_iterations=30))
    assert res.status.value == ref["status"] and res.iterations == ref["iterations"]
    H = ref["history"]
    assert np.array_equal(res.history[:, 3], H[:, 3])
    assert np.allclose(res.history[:, 0], H[:, 0], rtol=1e-7) and np.allclose(res.history[:, 1], H[:, 1], rtol=1e-4)
    assert abs(res.final_cost - ref["final_cost"]) <= 1e-6 * ref["final_cost"] and res.final_cost < res.initial_cost
    p = res.parameters[0]
    assert np.array_equal(p[0], d.poses[0]) and np.array_equal(p[100], d.poses[100])
    # a fixed translation DOF of a vertex whose rotation is free: t' = t + R V rho with rho_a = 0 still moves t unless all
    # of rho is fixed -- so only fully fixed vertices are bit-identical; the others follow the oracle's loop
    free = ~fix.astype(bool).all(axis=1)
    assert (np.abs(p[free] - d.poses[free]).max(axis=1) > 0).all()


# ---- sharded handles -----------------------------------------------------------------------------------------------------------
def _lockstep_case(oracle, d, world, tree):
    lam = 1e-3
    m = fm.with_gauge(fm.empty(d.n_cam, d.n_pt))
    # which landmarks a rank owns is decided by the library: a first set of handles tells, then every rank's range gets its
    # own asymmetric pattern (first, last and a middle landmark of the range, different DOF subsets)
    probe = [device(d, m, shard=(r, world), options={"tree_sharding": tree})[1] for r in range(world)]
    owned = np.stack([s.owned_landmarks() for s in probe])
    for s in probe:
        s.close()
    assert (owned.sum(0) == 1).all()
    for r in range(world):
        mine = np.nonzero(owned[r])[0]
        assert mine.size >= 3
        for k, l in enumerate((mine[0], mine[mine.size // 2], mine[-1])):
            m["pt"][l] = fm._subset(3 * r + k, 3)
    m["intr"][d.n_cam // 2] = (0, 1, 0); m["pose"][d.n_cam - 1] = (1, 0, 0, 0, 1, 0)
    prob, s1 = device(d, m)
    s1.solve_augmented_equation(lam)
    s1.eval_step(); s1.commit_step()
    p1 = s1.get_parameters()
    s1.close()
    ranks = [device(d, m, shard=(r, world), options={"tree_sharding": tree})[1] for r in range(world)]
    GpuSchurComplementSolver.lockstep_solve(ranks, lam)
    lay = prob.layout
    fp = m["pt"].astype(bool)
    nc = lay.cam_dof
    cam0 = ranks[0].export_step()[0][:nc]
    cam_only = np.zeros(lay.total_dof); cam_only[:nc] = cam0
    o = oracle_of(oracle, d, prob, "selfcal")
    o.apply_step(cam_only, 1.0)
    po, io, _ = o.get_params()
    for r, s in enumerate(ranks):
        assert np.array_equal(s.owned_landmarks(), owned[r])
        step = s.export_step()[0]
        assert np.array_equal(step[:nc], cam0)                             # (the camera step is replicated bit for bit)
        s.eval_step(); s.commit_step()
        pg, ig, lg = s.get_parameters()
        own = owned[r]
        dp = step[cols(lay.pt_col, 3)]
        want = np.where(fp, d.points, d.points + dp)
        assert np.array_equal(lg[own], want[own]), r                       # p where masked, p + d elsewhere: the rank's own step
        assert np.array_equal(lg[own][fp[own]], p1[2][own][fp[own]])      # masked: the single handle's bits
        assert rel(lg[own] - d.points[own], p1[2][own] - d.points[own]) < 1e-8   # (the lockstep step bound of test_gpu_configs.py)
        # every rank applies the same masked camera step
        assert np.array_equal(ig, io) and np.allclose(pg, po, rtol=SE3_RTOL, atol=SE3_ATOL)
        s.close()


@pytest.mark.parametrize("tree", [1, 0], ids=["tree-sharded", "range-sharded"])
def test_fixed_landmarks_on_two_lockstep_ranks(oracle, tree):
    """Landmark shards of one problem in this process (with_shard(r, 2), apexgpu_debug_lockstep_solve).  The lockstep helper
    drives the SOLVE only; eval_step / commit_step are then called on every rank's handle by itself, which is enough here: a
    rank retracts with its own landmark steps and the replicated camera step, and only its owned landmarks are compared.
    Tree sharding renumbers the landmarks rank-locally: this is where the mask's landmark permutation is not the identity."""
    d = pkg.synthetic.make_problem(640, 16000, 3, 7, config_id=310)
    _lockstep_case(oracle, d, 2, tree)


def test_fixed_landmarks_on_eight_lockstep_ranks(oracle):
    """venice-1778, the shape test_venice_1778_full_size_lockstep_8_ranks shards eight ways, at its full size: its samples
    (0.3, 0.5, 0.75 were tried) are refused an eight-way distributed plan ("the plan is not distributed").  Eight tree-sharded
    ranks, three fixed landmarks with different DOF subsets in every rank's range."""
    d = pkg.synthetic.make_named("venice-1778")
    _lockstep_case(oracle, d, 8, 1)
