"""Pins the numpy SE2 reference (tests/np_ref_se2.py) itself.  No GPU needed.

Known answers are the reference's own unit tests transcribed as data (crates/apex-manifolds/src/se2.rs tests, TOLERANCE =
1e-12 there); the analytic Jacobians are checked against central differences of r under the right-plus retraction; the
golden tests/golden/se2_manhattan_40.npz (written by tests/golden/make_golden_se2.py) is reproduced to 1e-14 relative."""
import os

import numpy as np
import pytest

import np_ref_se2 as ref

PI = np.pi
TOL = 1e-12     # se2.rs:778
HERE = os.path.dirname(os.path.abspath(__file__))


def v(x, y, th):
    return np.array([x, y, th], dtype=np.float64)


def test_identity_and_vector_form():
    assert np.array_equal(ref.vec(ref.mat(v(0, 0, 0))), v(0, 0, 0))                # test_se2_identity
    assert np.array_equal(ref.vec(ref.mat(v(4, 2, 0))), v(4, 2, 0))                # test_se2_from_xy_angle
    assert np.abs(ref.vec(ref.mat(v(1, 2, PI / 4))) - v(1, 2, PI / 4)).max() < TOL


def test_inverse():
    i = ref.vec(ref.inv(ref.mat(v(1, 1, PI))))                                     # test_se2_inverse: (1, 1, -pi)
    assert abs(i[0] - 1) < TOL and abs(i[1] - 1) < TOL and abs(abs(i[2]) - PI) < TOL
    e = ref.vec(ref.mat(v(1, 1, PI)) @ ref.inv(ref.mat(v(1, 1, PI))))
    assert np.abs(e).max() < TOL


def test_compose():
    c = ref.vec(ref.mat(v(1, 1, PI / 2)) @ ref.mat(v(2, 2, PI / 2)))              # test_se2_compose: (-1, 3, pi)
    assert abs(c[0] + 1) < TOL and abs(c[1] - 3) < TOL and abs(abs(c[2]) - PI) < TOL


def test_exp_log():
    t = v(4, 2, PI)                                                                # test_se2_exp_log
    assert np.abs(ref.log(ref.exp(t)) - t).max() < 1e-12 * 4
    assert np.abs(ref.vec(ref.exp(v(0, 0, 0)))).max() < TOL and np.abs(ref.log(ref.mat(v(0, 0, 0)))).max() < TOL
    for th in (1e-9, 1e-6, 0.99e-5, 1.01e-5, 1e-3):                                # both sides of the small-angle branch
        t = v(0.3, -0.7, th)
        assert np.abs(ref.log(ref.exp(t)) - t).max() < 1e-13


def test_between_and_adjoint():
    a = ref.mat(v(1, 1, PI))
    assert np.abs(ref.vec(ref.inv(a) @ a)).max() < TOL                             # test_se2_between
    A = ref.adjoint(ref.mat(v(1.5, -2.0, 0.3)))                                    # se2.rs:317-328
    c, s = np.cos(0.3), np.sin(0.3)
    assert np.allclose(A, [[c, -s, -2.0], [s, c, -1.5], [0, 0, 1]], rtol=0, atol=1e-15)
    # Adj(a b) = Adj(a) Adj(b); Adj(a^-1) = Adj(a)^-1
    b = ref.mat(v(-0.4, 0.9, -1.1)); a = ref.mat(v(1.5, -2.0, 0.3))
    assert np.abs(ref.adjoint(a @ b) - ref.adjoint(a) @ ref.adjoint(b)).max() < TOL
    assert np.abs(ref.adjoint(ref.inv(a)) @ ref.adjoint(a) - np.eye(3)).max() < TOL


def test_rplus_rminus_and_jacobian_pairs():
    x = v(1, 1, PI / 2); t = v(1, 1, PI / 2)
    y = ref.plus(x, t)                                                             # x * Exp(t)
    assert np.abs(ref.minus(y, x) - t).max() < TOL
    assert np.array_equal(ref.plus(x, np.zeros(3)), x)
    for th in (1e-9, 3e-6, 1e-3, 0.1, 1.0, 3.0, -2.5):
        t = v(1.0, 2.0, th)
        bound = 1e-9 if not 1e-5 <= abs(th) < 1e-3 else None                       # (Jr as coded: see test_se2_device_math_host)
        if bound:
            assert np.abs(ref.right_jacobian(t) @ ref.right_jacobian_inv(t) - np.eye(3)).max() < bound
    # Jr^-1 is continuous across the threshold (the regrouped form agrees with the Taylor branch where both hold)
    lo, hi = ref.right_jacobian_inv(v(0.7, -1.3, 0.999e-5)), ref.right_jacobian_inv(v(0.7, -1.3, 1.001e-5))
    assert np.abs(lo - hi).max() < 1e-7


def test_between_factor_known_answers():
    # between_factor.rs SE2 tests: identical poses and identity measurement -> zero residual, Jacobians (I, -I)
    r, J = ref.between_linearize(v(0, 0, 0), v(0, 0, 0), v(0, 0, 0))
    assert np.array_equal(r, np.zeros(3)) and np.array_equal(J[:, :3], np.eye(3)) and np.allclose(J[:, 3:], -np.eye(3), atol=0)
    # k1 = k0 * m^-1... the measured k0 -> k1 transform satisfied exactly: (k1^-1 k0) m = identity
    k0 = v(0.5, -0.2, 0.7); m = v(1.0, 0.3, -0.4)
    k1 = ref.vec(ref.mat(k0) @ ref.mat(m))
    r, _ = ref.between_linearize(k0, k1, m)
    assert np.abs(r).max() < TOL
    assert ref.between_linearize(v(0, 0, 0), v(1, 0, 0), v(0, 0, 0))[1].shape == (3, 6)   # the doc example's dimensions


def test_more_transcribed_known_answers():
    """se2.rs tests :1056-1300 with their numbers and tolerances."""
    i = ref.vec(ref.inv(ref.mat(v(0.7, 2.3, PI / 3))))                              # test_se2_inverse_detailed, 1e-10
    assert abs(i[0] + 2.341858428704209) < 1e-10 and abs(i[1] + 0.543782217350893) < 1e-10 and abs(i[2] + PI / 3) < 1e-10
    i0 = ref.inv(ref.mat(v(0, 0, 0)))
    assert np.abs(ref.vec(i0)).max() < TOL and abs(i0[0, 0] - 1) < TOL and abs(i0[1, 0]) < TOL   # real 1, imag 0
    c = ref.plus(v(1, 1, PI / 2), v(0, 0, 0))                                       # test_se2_rplus_zero
    assert np.abs(c - v(1, 1, PI / 2)).max() < TOL
    c = ref.plus(v(1, 1, PI / 2), v(1, 1, PI / 2))                                  # test_se2_rplus: angle pi
    assert abs(abs(c[2]) - PI) < TOL
    lp = ref.vec(ref.exp(v(1, 1, PI / 2)) @ ref.mat(v(1, 1, PI / 2)))               # test_se2_lplus: Exp(t) * x, angle pi
    assert abs(abs(lp[2]) - PI) < TOL
    assert np.abs(ref.minus(v(0, 0, 0), v(0, 0, 0))).max() < TOL                    # test_se2_rminus_zero
    assert abs(ref.minus(v(1, 1, PI), v(2, 2, PI / 2))[2] - PI / 2) < TOL           # test_se2_rminus
    lm = ref.log(ref.mat(v(1, 1, PI)) @ ref.inv(ref.mat(v(2, 2, PI / 2))))          # test_se2_lminus: Log(a b^-1)
    assert abs(lm[2] - PI / 2) < TOL
    assert abs(abs(ref.log(ref.mat(v(1, 1, PI)))[2]) - PI) < TOL                    # test_se2_lift
    b = ref.vec(ref.inv(ref.mat(v(1, 1, PI))) @ ref.mat(v(2, 2, PI / 2)))           # test_se2_between_detailed: (-1, -1, -pi/2)
    assert np.abs(b - v(-1, -1, -PI / 2)).max() < TOL
    a = ref.mat(v(1, 1, PI / 2)) @ np.array([1.0, 1.0, 1.0])                        # test_se2_act_detailed: (0, 2)
    assert abs(a[0]) < TOL and abs(a[1] - 2) < TOL
    a = ref.mat(v(1, 1, -PI / 2)) @ np.array([1.0, 1.0, 1.0])                       # (2, 0)
    assert abs(a[0] - 2) < TOL and abs(a[1]) < TOL
    e = ref.exp(v(4, 2, PI))                                                        # test_se2_tangent_retract(_jac)
    assert abs(e[0, 0] - np.cos(PI)) < TOL and abs(e[1, 0] - np.sin(PI)) < TOL and abs(abs(ref.vec(e)[2]) - PI) < TOL
    assert ref.right_jacobian(v(4, 2, PI)).shape == (3, 3)
    t = v(1e-8, 2e-8, 1e-9)                                                         # test_se2_small_angle_approximations
    assert np.linalg.norm(ref.log(ref.exp(t)) - t) < TOL
    for g1, g2, g3 in ((v(0.3, -0.8, 2.9), v(-0.5, 0.1, -1.7), v(0.9, 0.9, 0.4)),): # test_se2_consistency (fixed draws), 1e-10
        l = ref.vec((ref.mat(g1) @ ref.mat(g2)) @ ref.mat(g3)); r = ref.vec(ref.mat(g1) @ (ref.mat(g2) @ ref.mat(g3)))
        assert np.linalg.norm(l[:2] - r[:2]) < 1e-10 and abs(l[2] - r[2]) < 1e-10
    p = ref.plus(v(0.3, -0.8, 2.9), v(1e-12, 1e-12, 1e-12))                         # test_se2_is_approx: |x (-) x'| < 1e-10
    assert np.abs(ref.minus(p, v(0.3, -0.8, 2.9))).max() < 1e-10


def test_between_factor_reference_cases():
    """between_factor.rs:381-439 (forward differences, FD_EPSILON 1e-6, Frobenius norm of the difference < 1e-5) and
    :568-583 (finiteness) on the reference's own inputs."""
    m, pi_, pj = v(1.0, 0.0, 0.1), v(0, 0, 0), v(0.95, 0.05, 0.12)
    r, J = ref.between_linearize(pi_, pj, m)
    assert J.shape == (3, 6)
    eps = 1e-6
    Jfd = np.zeros((3, 6))
    for a in range(3):
        d = np.zeros(3); d[a] = eps
        Jfd[:, a] = (ref.between_linearize(ref.plus(pi_, d), pj, m)[0] - r) / eps
        Jfd[:, 3 + a] = (ref.between_linearize(pi_, ref.plus(pj, d), m)[0] - r) / eps
    assert np.linalg.norm(J - Jfd) < 1e-5
    r, J = ref.between_linearize(v(50, -100, 1.5), v(150, -300, -1.5), v(100, -200, PI))
    assert np.isfinite(r).all() and np.isfinite(J).all()
    r, _ = ref.between_linearize(v(0, 0, 0), v(0, 0, 0), v(0, 0, 0))                # test_between_factor_se2_identity, 1e-9
    assert np.linalg.norm(r) < 1e-9


def test_prior_factor():
    p = ref.Problem(np.array([[1.0, 2.0, 0.5]]), [], [], np.zeros((0, 3)), np.array([0]), np.zeros((1, 3), np.uint8),
                    priors=[(0, np.array([0.5, 2.5, 0.25]), None)])
    r, J = p.jacobian()
    assert np.array_equal(r, [0.5, -0.5, 0.25]) and np.array_equal(J, np.eye(3))
    p.priors = [(0, np.array([0.5, 2.5, 0.25]), 0.1)]
    r2, J2 = p.jacobian()
    sc = np.sqrt(0.1 / np.sqrt(0.5625))
    assert np.allclose(r2, sc * r, rtol=1e-15) and np.allclose(J2, sc * np.eye(3), rtol=1e-15)


def _fd(k0, k1, m, h):
    Jn = np.zeros((3, 6))
    for a in range(3):
        e = np.zeros(3); e[a] = h
        Jn[:, a] = (ref.between_linearize(ref.plus(k0, e), k1, m)[0] - ref.between_linearize(ref.plus(k0, -e), k1, m)[0]) / (2 * h)
        Jn[:, 3 + a] = (ref.between_linearize(k0, ref.plus(k1, e), m)[0] - ref.between_linearize(k0, ref.plus(k1, -e), m)[0]) / (2 * h)
    return Jn


def test_analytic_jacobians_against_central_differences():
    """O(1) inputs, h = 1e-6: truncation h^2 |r'''| ~ 1e-12, rounding 1e-16 / h ~ 1e-10; bound 1e-8 (two decades)."""
    rng = np.random.default_rng(11)
    worst = 0.0
    cases = []
    for _ in range(30):
        cases.append((v(*rng.uniform(-2, 2, 2), rng.uniform(-PI + 0.01, PI - 0.01)), v(*rng.uniform(-2, 2, 2), rng.uniform(-PI + 0.01, PI - 0.01)),
                      v(*rng.uniform(-1, 1, 2), rng.uniform(-1, 1))))
    cases.append((v(1, 2, PI - 0.01), v(-1, 0.5, -PI + 0.01), v(0.2, 0.1, 0.3)))
    for th in (1e-9, 2e-6, 3e-5, 1e-3):                                            # residual angle inside / outside the branch
        k1 = v(0.3, -0.2, 0.4)
        cases.append((ref.plus(k1, v(0.4, -0.3, th)), k1, v(0, 0, 0)))
    for k0, k1, m in cases:
        _, J = ref.between_linearize(k0, k1, m)
        worst = max(worst, np.abs(_fd(k0, k1, m, 1e-6) - J).max())
    print("worst |J - central difference|", worst)
    assert worst < 1e-8


def test_golden_is_reproduced():
    import sys
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_golden_se2 as mk

    g = np.load(os.path.join(HERE, "golden", "se2_manhattan_40.npz"))
    now = mk.build()
    for k in g.files:
        a, b = np.asarray(now[k], dtype=np.float64), np.asarray(g[k], dtype=np.float64)
        assert a.shape == b.shape, k
        if a.size:
            assert np.abs(a - b).max() <= 1e-14 * max(np.abs(b).max(), 1e-300), k
    # the golden run converged (cost or parameter tolerance) and met the reference's 85 % improvement
    assert int(g["lm_status"]) in (2, 3) and float(g["lm_final_cost"]) < 0.15 * float(g["initial_cost"])
    assert float(g["initial_cost"]) == pytest.approx(float(g["cost"]), rel=1e-15)
