"""tests/ba_prior_ref.py against itself and against np_ref.py.  No GPU needed.

The premises of tests/test_gpu_ba_priors.py: that the reference with no priors IS np_ref, that its prior rows are the factor of
src/factors/prior_factor.rs:93-105 behind the linearizer's truncation (sparse.rs:201-204), a known answer, the Huber scale, and
that the block check the device test uses notices the two mistakes a device path could make.
"""
import numpy as np

import ba_prior_ref as br
import np_ref
import np_ref_ba_tr as bt
from apex_solver_amd.solver import OptimizationType


def golden(name="ba6x40_selfcal", **kw):
    d, opt, delta, _ = bt.golden_data(name)
    return br.PriorBaProblem(d, opt, bt.huber(delta), bt.gauge(d), **kw), delta


def test_without_priors_the_reference_is_np_ref():
    """exactly: np_ref's own blocks where no loss is set (its Huber is spelled differently from the loss family's), and the
    BaProblem it extends under the golden's Huber"""
    for name in ("ba6x40_selfcal", "ba6x40_ba"):
        d, opt, delta, _ = bt.golden_data(name)
        P = br.PriorBaProblem(d, opt, None, bt.gauge(d))
        r, J = P.jacobian()
        rt, cost, Jp, Jl, Ji = np_ref.jacobian_blocks(d.poses, d.intr, d.points, P.ci, P.pi, d.obs_uv, 0)
        J0 = np_ref.sparse_jacobian(Jp, Jl, Ji, P.ci, P.pi, P.lay, selfcal=P.selfcal)
        assert np.array_equal(r, rt.ravel()) and (J != J0).nnz == 0
        P, _ = golden(name)
        B = bt.BaProblem(d, P.opt, P.loss, P.masks)
        (r, J), (rb, Jb) = P.jacobian(), B.jacobian()
        assert np.array_equal(r, rb) and (J != Jb).nnz == 0 and P.cost() == B.cost()
        assert all(x.size == 0 for x in P.prior_residuals())


def test_prior_jacobian_against_central_differences_under_right_plus():
    """The intrinsics block (an Rn variable) and the translation rows of a pose block at R = I ARE derivatives of the residual
    under the retraction, weight included; the seventh row has no column.  The rotation rows of the reference's factor are
    the identity as well (prior_factor.rs:100), which is NOT the derivative of the quaternion (that is w/2 at R = I): restated
    as coded, and pinned here so that nobody "fixes" it on one side only."""
    P, _ = golden()
    poses, intr, pts = (x.copy() for x in P.params)
    c, w = 3, 2.5
    poses[c, 3:7] = [1.0, 0.0, 0.0, 0.0]
    P.params = (poses, intr, pts)
    P.pose_priors = [(c, np.array([0.1, -0.2, 0.3, 0.9, 0.1, 0.0, 0.2]), None, w)]
    P.intr_priors = [(c, intr[c] + np.array([3.0, 0.01, -0.02]), None, w)]
    _, J = P.jacobian()
    Jp = J[2 * P.d.n_obs:].toarray()
    cols = np.concatenate([P.lay.pose_col[c] + np.arange(6), P.lay.intr_col[c] + np.arange(3)])
    assert Jp.shape[0] == 10 and np.count_nonzero(np.delete(Jp, cols, axis=1)) == 0
    A = Jp[:, cols]
    assert np.array_equal(A[:6, :6], w * np.eye(6)) and not A[6].any() and np.array_equal(A[7:, 6:], w * np.eye(3))
    h, N = 1e-6, np.zeros((10, 9))
    for k, col in enumerate(cols):
        out = []
        for sgn in (1.0, -1.0):
            step = np.zeros(P.n); step[col] = sgn * h
            Q = br.PriorBaProblem(P.d, P.opt, P.loss, P.masks, np_ref.retract(poses, intr, pts, step, P.lay), P.pose_priors, P.intr_priors)
            out.append(np.concatenate([x.ravel() for x in Q.prior_residuals()]))
        N[:, k] = (out[0] - out[1]) / (2 * h)
    # (a central difference of w (f - data) rounds at eps |f| w / h: the focal length is ~1e3 pixels)
    tol_intr = 1e-7 + 4 * np.finfo(float).eps * np.abs(intr[c]).max() * w / h
    assert np.abs(N[7:, 6:] - A[7:, 6:]).max() < tol_intr and np.abs(N[:3, :3] - A[:3, :3]).max() < 1e-7
    assert np.abs(N[:7, 6:]).max() < 1e-7 and np.abs(N[7:, :6]).max() < 1e-7
    # the quaternion's true derivative at R = I -- w/2 on (qx, qy, qz), the seventh row included, none on qw: not what the factor
    # states (w on rows 3..5, the seventh row cut off with its column)
    assert np.abs(N[4:7, 3:6] - 0.5 * w * np.eye(3)).max() < 1e-7 and np.abs(N[3]).max() < 1e-7


def test_known_answer_one_intrinsics_prior():
    """w = 2, data offset (0.5, 0, 0): the camera's intrinsics block of H gains 4 I3 and its gradient 4 r"""
    P, _ = golden()
    c = 2
    H0, g0 = P.normal_equations()
    P.intr_priors = [(c, P.params[1][c] - np.array([0.5, 0.0, 0.0]), None, 2.0)]
    H1, g1 = P.normal_equations()
    idx = P.lay.intr_col[c] + np.arange(3)
    dH, dg = H1 - H0, g1 - g0
    assert np.allclose(dH[np.ix_(idx, idx)], 4.0 * np.eye(3), rtol=0, atol=1e-9)
    dH[np.ix_(idx, idx)] = 0.0
    assert np.abs(dH).max() < 1e-9
    assert np.allclose(dg[idx], 4.0 * np.array([0.5, 0.0, 0.0]), rtol=0, atol=1e-9) and np.abs(np.delete(dg, idx)).max() < 1e-9   # (dense J^T r: the extra rows change the summation order)
    assert abs(P.cost() - golden()[0].cost() - 0.5 * (2.0 * 0.5) ** 2) < 1e-9


def test_huber_inlier_and_outlier_scale():
    P, _ = golden()
    c = 1
    x = br.pose_vector(P.params[0])[c]
    off = np.array([3.0, 0.0, 4.0, 0.0, 0.0, 0.0, 0.0])   # |r| = 5 w
    for w, delta, want in ((1.0, 10.0, 1.0), (1.0, 5.0, 1.0), (1.0, 2.0, np.sqrt(2.0 / 5.0)), (0.25, 1.0, np.sqrt(1.0 / 1.25)), (7.0, 1.0, np.sqrt(1.0 / 35.0))):
        P.pose_priors = [(c, x - off, delta, w)]
        rp, _ = P.prior_residuals()
        assert np.allclose(rp[0], want * w * off, rtol=1e-15, atol=0)
        _, J = P.jacobian()
        assert np.allclose(J[2 * P.d.n_obs:].toarray()[:6, P.lay.pose_col[c]:P.lay.pose_col[c] + 6], want * w * np.eye(6), rtol=1e-15, atol=0)


def test_the_block_check_notices_a_dropped_prior_and_a_seventh_column():
    P, _ = golden()
    c = P.d.n_cam - 1
    P.pose_priors = [(c, br.pose_vector(P.params[0])[c] + 0.01, None, 7.0)]
    P.intr_priors = [(c, P.params[1][c] * 1.01, None, 7.0)]
    H, g = P.normal_equations()
    assert br.camera_blocks_agree(H, H, P.lay, [c])
    Q, _ = golden()
    H_dropped = Q.normal_equations()[0]   # the prior in g but not in H
    assert not br.camera_blocks_agree(H_dropped, H, P.lay, [c])
    H7 = H.copy()   # seven columns instead of six: the quaternion's last row would land on the first intrinsics column
    H7[P.lay.intr_col[c], P.lay.intr_col[c]] += 49.0
    assert not br.camera_blocks_agree(H7, H, P.lay, [c])


def test_d_c_6_has_no_intrinsics_priors():
    d, opt, delta, _ = bt.golden_data("ba6x40_ba")
    assert opt == OptimizationType.BundleAdjustment
    try:
        br.PriorBaProblem(d, opt, bt.huber(delta), bt.gauge(d), intr_priors=[(0, d.intr[0], None, 1.0)])
    except AssertionError:
        return
    raise AssertionError("accepted")
