"""The SO3 reference (tests/so3_ref.py) against itself.  No GPU needed.  Finite differences in the reference solver's own style
(crates/apex-manifolds/src/so3.rs:1354-1415: central, right-plus, step 1e-6, bound 1e-7), round trips, and the two invariances
of a quaternion's representation (sign, norm)."""
import numpy as np

import so3_ref as sr
from so3_ref import LD


def _triples(n=12, seed=5):
    rng = np.random.default_rng(seed)
    return sr.random_rotations(rng, n), sr.random_rotations(rng, n), sr.random_rotations(rng, n)


def test_jacobians_against_central_differences_under_right_plus():
    k0, k1, m = _triples()
    r, J = sr.so3_between(k0, k1, m)
    h = 1e-6
    worst = 0.0
    for which, cols in ((0, slice(0, 3)), (1, slice(3, 6))):
        for a in range(3):
            d = np.zeros((len(k0), 3)); d[:, a] = h
            ks = [k0, k1]
            kp, km = list(ks), list(ks)
            kp[which] = sr.f64(sr.so3_plus(ks[which], d)); km[which] = sr.f64(sr.so3_plus(ks[which], -d))
            rp, _ = sr.so3_between(kp[0], kp[1], m); rm, _ = sr.so3_between(km[0], km[1], m)
            fd = (rp - rm) / (2 * h)
            worst = max(worst, float(np.abs(fd - J[:, :, cols][:, :, a]).max()))
    print("worst |fd - J|", worst)
    assert worst < 1e-7


def test_log_of_exp_and_plus_of_log_round_trip():
    rng = np.random.default_rng(6)
    th = rng.standard_normal((40, 3))
    th = th / np.linalg.norm(th, axis=1, keepdims=True) * rng.uniform(0, np.pi - 1e-3, 40)[:, None]
    th[:6] *= np.array([1e-9, 1e-7, 5e-6, 0.99e-5, 1.01e-5, 2e-5])[:, None] / np.linalg.norm(th[:6], axis=1, keepdims=True)
    back = sr.so3_log(sr.so3_exp(th))
    assert float(np.abs(back - th).max()) < 1e-16 * 8          # long double both ways
    R, S = sr.random_rotations(rng, 40), sr.random_rotations(rng, 40)
    RS = sr._qmul(sr._qconj(sr._ld(R)), sr._ld(S))
    T = sr.so3_plus(R, sr.f64(sr.so3_log(RS)))                # the fp64 rounding of the tangent bounds this one
    sign = np.sign((T * S).sum(-1))[:, None]
    assert float(np.abs(T * sign - S).max()) < 1e-15


def test_q_and_minus_q_give_the_same_block():
    k0, k1, m = _triples(seed=7)
    r, J = sr.so3_between(k0, k1, m)
    for flip in ((-1, 1, 1), (1, -1, 1), (1, 1, -1), (-1, -1, 1)):
        r2, J2 = sr.so3_between(flip[0] * k0, flip[1] * k1, flip[2] * m)
        # the composed quaternion changes sign with an odd number of flips: Log's cos < 0 arm gives the same rotation vector
        assert float(np.abs(r2 - r).max()) < 1e-17 and float(np.abs(J2 - J).max()) < 1e-17


def test_scaled_input_gives_the_result_of_the_normalised_one():
    k0, k1, m = _triples(seed=8)
    r, J = sr.so3_between(k0, k1, m)
    for s in (1 + 1e-3, 1 - 1e-3):
        for which in range(3):
            trip = [k0, k1, m]
            trip[which] = trip[which] * s
            r2, J2 = sr.so3_between(*trip)
            # q * s is itself rounded to fp64: each component moves by up to 2^-53 relative, so the rotation by up to
            # 2 * 2^-53 rad and r, J by a small multiple of that -- 1e-15 is ten such roundings, not the 2^-64 of the arithmetic
            assert float(np.abs(r2 - r).max()) < 1e-15 and float(np.abs(J2 - J).max()) < 1e-15


def test_prior_rows_and_plus_zero():
    rng = np.random.default_rng(9)
    q = sr.random_rotations(rng, 3) * 1.01
    data = sr.random_rotations(rng, 3)
    r, sc = sr.so3_prior(q, data, [None, 0.1, 1e3])
    raw = sr.so3_from_vec(q) - sr._ld(data)
    assert r.shape == (3, 4) and sc[0] == 1 and sc[2] == 1 and 0 < sc[1] < 1
    assert np.array_equal(r[0], raw[0]) and float(np.abs(r[1] - raw[1] * sc[1]).max()) == 0.0
    assert np.array_equal(sr.f64(sr.so3_plus(q, np.zeros((3, 3)))), q)      # q (+) 0 keeps the stored bits


def test_dense_problem_agrees_with_its_blocks():
    from apex_solver_amd.pose_graph import PoseGraphProblem

    d = sr.crafted("loop")
    prob = PoseGraphProblem(d, manifold="so3").add_prior("x0", huber_delta=None).add_prior("x5", data=d.poses[5] * 0.9)
    P = sr.So3Problem.from_problem(prob)
    H, g, cost = P.dense(0.5)
    Hn, gn = P.normal_equations()
    assert np.abs(sr.f64(H) - (Hn + 0.5 * np.eye(P.n))).max() < 1e-13 * np.abs(Hn).max()
    assert np.abs(sr.f64(g) - gn).max() < 1e-13 * max(1.0, np.abs(gn).max())
    assert abs(float(cost) - P.cost()) < 1e-13 * P.cost()
    assert Hn[15, 15] > 0 and np.count_nonzero(Hn[15:18, :15]) == 0         # vertex 5: a self-loop and a prior only
