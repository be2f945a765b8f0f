"""The numpy side of Dog-Leg on bundle adjustment (tests/np_ref_ba_tr.py), on the CPU: BaProblem's normal equations are the
oracle's, the six-sums form of the step is the vector form, and the numpy Dog-Leg runs the device test compares with keep every
decision away from its threshold."""
import numpy as np
import pytest

import np_ref
import np_ref_ba_tr as bt
import np_ref_trust_region as tr


def rel(a, b):
    return float(np.linalg.norm(np.ravel(a) - np.ravel(b)) / max(np.linalg.norm(np.ravel(b)), 1e-300))


@pytest.mark.parametrize("name", ["ba6x40_selfcal", "ba6x40_ba"])
def test_normal_equations_are_the_oracles(name):
    """H = J^T J from the golden's (the C oracle's) Jacobian blocks, g its gradient: 1e-12, the bound test_oracle_golden.py holds
    the oracle to against numpy."""
    d, opt, delta, g = bt.golden_data(name)
    P = bt.BaProblem(d, opt, bt.huber(delta), bt.gauge(d))
    H, grad = P.normal_equations()
    selfcal = name.endswith("selfcal")
    J = np_ref.sparse_jacobian(g["it0_Jpose"], g["it0_Jpt"], g["it0_Jintr"], d.cam_idx.astype(int), d.pt_idx.astype(int), P.lay, selfcal=selfcal)
    Ho = (J.T @ J).toarray()
    print(name, "H", rel(H, Ho), "g", rel(grad, g["it0_grad"]), "cost", abs(P.cost() / float(g["initial_cost"]) - 1))
    assert rel(H, Ho) < 1e-12 and rel(grad, g["it0_grad"]) < 1e-12
    assert P.cost() == pytest.approx(float(g["initial_cost"]), rel=1e-13)
    assert np.array_equal(P.lay.pose_col, g["pose_col"]) and np.array_equal(P.lay.pt_col, g["pt_col"])


@pytest.mark.parametrize("scaling", [False, True], ids=["plain", "jacobi-scaling"])
def test_combine_is_the_vector_form_for_every_step_type(scaling):
    d, opt, delta, _ = bt.golden_data("ba6x40_selfcal")
    P = bt.BaProblem(d, opt, bt.huber(delta), bt.gauge(d))
    tr._init_scaling(P, scaling)
    H, g = P.normal_equations()
    mu = bt.mu_for_condition(H)
    h = tr.solve_damped(H, g, mu)
    alpha, p_c = tr.cauchy_point(H, g)
    hn, pn = np.linalg.norm(h), np.linalg.norm(p_c)
    assert np.linalg.cond(H + mu * np.eye(P.n)) <= 1e5 and pn < hn
    sums = tr.sums_of(H, g, h)
    for radius, typ in ((2.0 * hn, tr.GAUSS_NEWTON), (0.5 * pn, tr.STEEPEST_DESCENT), (0.5 * (pn + hn), tr.DOG_LEG)):
        step, t, beta = tr.dog_leg_step(-g, p_c, h, radius)
        c = tr.combine(*sums, radius)
        assert t == typ == c["type"]
        assert rel(c["c_g"] * (-g) + c["c_h"] * h, step) < 1e-12
        assert c["alpha"] == pytest.approx(alpha, rel=1e-12) and c["beta"] == pytest.approx(beta, rel=1e-9, abs=1e-300)
        assert c["step_norm"] == pytest.approx(np.linalg.norm(step), rel=1e-12)
        assert c["predicted_reduction"] == pytest.approx(tr.predicted_reduction(step, g, H), rel=1e-9)


@pytest.mark.parametrize("case", list(bt.HISTORY_CASES))
def test_numpy_dogleg_runs_stay_clear_of_every_threshold(case):
    ref = bt.dogleg_reference(case)
    R = ref["history"]
    print(case, ref["status"], ref["iterations"], "margin", ref["margins"].min(), "types", R[:, 9], "accepted", R[:, 4], "reused", R[:, 11])
    assert ref["margins"].min() > 1e-6
    assert R[-1, 0] < R[0, 0] < ref["initial_cost"]
    assert len(set(R[:, 9])) >= 2   # more than one step type in every run


def test_the_runs_together_show_every_branch():
    R = np.concatenate([bt.dogleg_reference(c)["history"] for c in bt.HISTORY_CASES])
    assert set(R[:, 9]) == {0.0, 1.0, 2.0}
    assert (R[:, 4] == 0).any() and (R[:, 11] == 1).any()          # a rejection, a reused step
    assert ((R[:, 11] == 1) & (R[:, 4] == 1)).any()                # ... and a reused step that was accepted


def test_custom_structure_has_the_shapes_the_kernels_can_trip_on():
    d = bt.custom_data()
    n = np.bincount(d.pt_idx)
    assert n.min() == 1 and n.max() > 256 and d.n_obs % 64 != 0 and d.n_obs > 256


def test_why_the_unscaled_loss_free_run_keeps_mu_in_pixels():
    """The premise of np_ref_ba_tr.MU, on the numpy matrix alone: at the defaults that run's mu sinks below 1e-6 while
    lambda_max(H) is 1.1e6 px^2, cond(H + mu I) > 1e12 -- beyond what two fp64 solves of one system can agree on to the
    history test's 1e-7 -- and inside MU's range the condition number stays below 2e8 (1.3e-8 in a step)."""
    P, scaling = bt.history_problem("ba-noloss-plain")
    assert not scaling
    H, _ = P.normal_equations()
    lam_max = float(np.linalg.eigvalsh(H)[-1])
    default = tr.dog_leg(P, trust_region_radius=bt.dogleg_reference("ba-noloss-plain")["radius0"], use_jacobi_scaling=False,
                         max_iterations=bt.DL_ITERS)
    mu_low = float(default["history"][:, 2].min())
    print("lambda_max", lam_max, "lowest default mu", mu_low, "cond", np.linalg.cond(H + mu_low * np.eye(P.n)))
    assert mu_low < 1e-6 and np.linalg.cond(H + mu_low * np.eye(P.n)) > 1e12
    assert np.linalg.cond(H + bt.MU["ba-noloss-plain"]["min_mu"] * np.eye(P.n)) < 2e8
    assert bt.dogleg_reference("ba-noloss-plain")["history"][:, 2].min() >= bt.MU["ba-noloss-plain"]["min_mu"]
