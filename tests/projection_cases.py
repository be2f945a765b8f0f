"""Crafted observations at the edges of the BAL projection factor -- TEST INFRASTRUCTURE ONLY (CPU;
tests/test_projection_ref_host.py, tests/test_gpu_projection_edges.py).

Every observation is built from the camera frame backwards: the camera-frame point p_c and the camera are chosen,
p_w = R^T (p_c - t) is computed in long double and rounded, and uv = projection - (wanted residual), so that the edge sits where
it is meant to.  `premises` re-derives p_c, r2, dist and s from the ROUNDED inputs (projection_ref.reference) and asserts what each
case claims -- classification margins included -- so that no disagreement between a device form and the reference can come from
an ambiguous classification.  Every input is finite.

Scenes (one per class, at most 9 edge observations each):
  depth       z = -1e-6 (1 +- 1e-3) (valid with -1/z ~ 1e6 | invalid), the camera centre, behind, z = -1e6, z = -1
  field       xn = yn = 0 (r2 = 0 exactly), xn = 0 only, yn = 0 only, r2 ~ 25
  distortion  k1 = k2 = 0, k2 = 0 only, k1 = 0 only, dist = 5e-4, dist = -1 (the fold of the model), |k1 r2| = 1e3
  camera      stored quaternion norms 2, 1e-3, 1 + 1e-9; q_w < 0; pi about each axis; identity; f = 1, 1e4; |t| ~ |p_w| ~ 1e4
  residual    |r| = 1e-9, delta (1 -+ 1e-6), 10 delta, 1e6 pixels, r along one axis (inside and outside), delta = SCALE

Shapes: `isolated(scene)` gives observation i camera i and landmark i of its own; `braced(scene)` gives each edge observation
flagged `brace` two ordinary cameras on its landmark (baseline 1 rad, z = -1, residuals of 0.5 pixels) and its camera two ordinary
landmarks.  Left out of the braced scenes, because cond(S) <= 1e8 cannot hold with them at lambda = 1 or because their own
conditioning (a p_c that is the difference of two numbers 1e6 .. 1e10 times its size) is what the block bound of schur_ref.py
deliberately does not carry: f = 1e4, |t| ~ 1e4, |k1 r2| = 1e3, the 1e6-pixel residual, and the generic-camera twins of the
threshold depths.  The stored quaternion norms 2, 1e-3 and 1 + 1e-9 are left out too: a step is applied on the braced scenes, and
the retraction (se3_plus) rotates the translation part of the step with the quaternion AS STORED, which is unit up to the rounding
of a product wherever a step may be applied; the projection normalises twice and is what those three cases are about.  All of
them stay in the isolated scenes.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import apex_solver_amd as pkg
import np_ref_loss as nl
import projection_ref as pr
from apex_solver_amd import capi
from apex_solver_amd.loss import Loss
from apex_solver_amd.solver import OptimizationType
from tile_ref import LD

SCALE = 2.0        # the scale (delta) of every loss that has one
LAMBDA = 1.0       # the damping of the braced scenes
GENERIC_Q = tuple(np.array([0.9, 0.1, -0.3, 0.2]) / np.linalg.norm([0.9, 0.1, -0.3, 0.2]))   # unit to rounding, as a retraction leaves it
GENERIC_T = (0.3, -0.2, 0.5)
INTR = (100.0, -0.05, 0.01)
R_DEFAULT = (0.3, -0.4)

# every loss apexgpu_set_loss accepts for bundle adjustment (pg_loss_first_arm_only), the legacy double and none
LOSSES = {
    "huber_delta": ("huber_delta", SCALE), "none": None, "l2": Loss(capi.LOSS_L2), "l1": Loss(capi.LOSS_L1),
    "huber": Loss(capi.LOSS_HUBER, SCALE), "cauchy": Loss(capi.LOSS_CAUCHY, SCALE), "fair": Loss(capi.LOSS_FAIR, SCALE),
    "geman": Loss(capi.LOSS_GEMAN_MCCLURE, SCALE), "welsch": Loss(capi.LOSS_WELSCH, SCALE), "tukey": Loss(capi.LOSS_TUKEY, SCALE),
    "ramsay": Loss(capi.LOSS_RAMSAY, SCALE), "trimmed": Loss(capi.LOSS_TRIMMED_MEAN, SCALE), "lp1.5": Loss(capi.LOSS_LP_NORM, 1.5),
    "lp2": Loss(capi.LOSS_LP_NORM, 2.0), "barron1": Loss(capi.LOSS_BARRON, 1.0, SCALE), "barron0": Loss(capi.LOSS_BARRON, 0.0, SCALE),
    "barron-2": Loss(capi.LOSS_BARRON, -2.0, SCALE), "tdist": Loss(capi.LOSS_T_DISTRIBUTION, 5.0),
}
# mode -> (OptimizationType, camera columns, mask code 4 POSE + 2 LANDMARK + INTRINSIC)
MODES = {
    "selfcal": (OptimizationType.SelfCalibration, 9, 7), "ba": (OptimizationType.BundleAdjustment, 6, 6),
    "only_pose": (OptimizationType.OnlyPose, 6, 4), "only_landmarks": (OptimizationType.OnlyLandmarks, 6, 2),
    "only_intrinsics": (OptimizationType.OnlyIntrinsics, 9, 1), "pose_intrinsics": (OptimizationType.PoseAndIntrinsics, 9, 5),
    "landmarks_intrinsics": (OptimizationType.LandmarksAndIntrinsics, 9, 3),
}


def _o(name, pc, q=GENERIC_Q, t=GENERIC_T, intr=INTR, r=R_DEFAULT, valid=True, brace=True, **claims):
    return SimpleNamespace(name=name, pc=pc, q=q, t=t, intr=intr, r=r, valid=valid, brace=brace, claims=claims)


_ID = (1.0, 0.0, 0.0, 0.0)
_Z0 = (0.0, 0.0, 0.0)
_NEAR = (1e-3, -0.05, 0.01)                        # f of the threshold depths: Jl ~ f 1e6 stays comparable with the braces'
_PD = (0.3, -0.2, -1.1); _R2D = (0.09 + 0.04) / 1.21   # the distortion class's point and its r2
_QN = GENERIC_Q
_PCAM = (0.25, -0.15, -1.3)
_PRES = (-0.2, 0.35, -1.2)
_DIR = np.array([0.6, 0.8])

SCENES = {
    "depth": [
        _o("near_valid", (1e-7, -0.7e-7, -1e-6 * (1 + 1e-3)), _ID, _Z0, _NEAR, depth_within=2e-3),
        _o("near_valid_generic", (1e-7, -0.7e-7, -1e-6 * (1 + 1e-3)), intr=_NEAR, brace=False, depth_within=2e-3),
        _o("near_invalid", (1e-7, -0.7e-7, -1e-6 * (1 - 1e-3)), _ID, _Z0, _NEAR, valid=False, depth_within=2e-3),
        _o("near_invalid_generic", (1e-7, -0.7e-7, -1e-6 * (1 - 1e-3)), intr=_NEAR, valid=False, brace=False, depth_within=2e-3),
        _o("centre", (0.0, 0.0, 0.0), valid=False),
        _o("behind", (0.2, -0.1, 1.0), valid=False),
        _o("far", (1e5, -0.7e5, -1e6), move_camera=True),
        _o("unit", (0.1, -0.07, -1.0)),
    ],
    "field": [
        _o("on_axis", (0.0, 0.0, -2.0), _ID, _Z0, r2_zero=True),
        _o("xn_zero", (0.0, 0.3, -1.5), _ID, (0.0, 0.1, -0.5), xn_zero=True),
        _o("yn_zero", (-0.4, 0.0, -1.5), _ID, (0.1, 0.0, -0.5), yn_zero=True),
        _o("wide", (3.5, 3.6, -1.0), intr=(1.0, -0.05, 0.01), r2_about=25.0),
    ],
    "distortion": [
        _o("k1_k2_zero", _PD, intr=(100.0, 0.0, 0.0)),
        _o("k2_zero", _PD, intr=(100.0, -0.05, 0.0)),
        _o("k1_zero", _PD, intr=(100.0, 0.0, 0.01)),
        _o("dist_small", _PD, intr=(100.0, -(1 - 5e-4) / _R2D, 0.0), dist_about=5e-4),
        _o("dist_negative", _PD, intr=(100.0, -2.0 / _R2D, 0.0), dist_about=-1.0),
        _o("k1r2_1e3", _PD, intr=(100.0, 1e3 / _R2D, 0.0), brace=False, dist_about=1001.0),
    ],
    "camera": [
        _o("qnorm_2", _PCAM, q=tuple(2.0 * np.array(_QN)), brace=False),
        _o("qnorm_1e-3", _PCAM, q=tuple(1e-3 * np.array(_QN)), brace=False),
        _o("qnorm_1+1e-9", _PCAM, q=tuple((1 + 1e-9) * np.array(_QN)), brace=False),
        _o("qw_negative", _PCAM, q=tuple(-np.array(GENERIC_Q))),
        _o("pi_x", _PCAM, q=(0.0, 1.0, 0.0, 0.0)),
        _o("pi_y", _PCAM, q=(0.0, 0.0, 1.0, 0.0)),
        _o("pi_z", _PCAM, q=(0.0, 0.0, 0.0, 1.0)),
        _o("identity", _PCAM, q=_ID),
        _o("f_1", _PCAM, intr=(1.0, -0.05, 0.01)),
        _o("f_1e4", _PCAM, intr=(1e4, -0.05, 0.01), brace=False),
        _o("cancellation", _PCAM, t=(1e4, -2e4, 1.5e4), brace=False, pw_about=2.7e4),
    ],
    "residual": [
        _o("r_1e-9", _PRES, r=tuple(1e-9 * _DIR), r_norm=1e-9),
        _o("r_below", _PRES, r=tuple(SCALE * (1 - 1e-6) * _DIR), r_norm=SCALE * (1 - 1e-6)),
        _o("r_above", _PRES, r=tuple(SCALE * (1 + 1e-6) * _DIR), r_norm=SCALE * (1 + 1e-6)),
        _o("r_10", _PRES, r=tuple(10 * SCALE * _DIR), r_norm=10 * SCALE),
        _o("r_1e6", _PRES, r=tuple(1e6 * _DIR), brace=False, r_norm=1e6),
        _o("r_u_inside", _PRES, r=(0.5, 0.0)),
        _o("r_v_inside", _PRES, r=(0.0, -0.5)),
        _o("r_u_outside", _PRES, r=(3.0, 0.0)),
    ],
}


# ---- construction --------------------------------------------------------------------------------------------------------------
def _place(q, t, pc):
    """p_w = R^T (p_c - t) in long double, rounded"""
    R = pr.rotation_ld(q)
    return np.asarray(R.T @ (np.asarray(pc, dtype=LD) - np.asarray(t, dtype=LD)), dtype=np.float64)


def _uv(q, t, intr, pw, r):
    """uv = projection of the rounded inputs - r (a point that does not project gets a plain pixel)"""
    R = pr.rotation_ld(q)
    pc = R @ pw.astype(LD) + np.asarray(t, dtype=LD)
    if not pc[2] < -1e-7:
        return np.array([0.3, -0.2])
    return np.asarray(pr.raw_projection(R, np.asarray(t, dtype=LD), np.asarray(intr, dtype=LD), pw.astype(LD)) - np.asarray(r, dtype=LD),
                      dtype=np.float64)


def _camera_at(q, pw, pc):
    """the pose (7,) with rotation q that sees p_w at p_c"""
    R = pr.rotation_ld(q)
    t = np.asarray(np.asarray(pc, dtype=LD) - R @ np.asarray(pw, dtype=LD), dtype=np.float64)
    return np.concatenate([t, np.asarray(q, dtype=np.float64)])


def _data(poses, intr, pts, ci, li, uv, name):
    return pkg.synthetic.BAProblemData(poses=np.ascontiguousarray(poses, dtype=np.float64), intr=np.ascontiguousarray(intr, dtype=np.float64),
                                       points=np.ascontiguousarray(pts, dtype=np.float64), cam_idx=np.asarray(ci, dtype=np.uint32),
                                       pt_idx=np.asarray(li, dtype=np.uint32), obs_uv=np.ascontiguousarray(uv, dtype=np.float64), name=name)


_CACHE = {}


def isolated(scene):
    """(data, the scene's observation list): observation i = camera i, landmark i"""
    if ("iso", scene) not in _CACHE:
        obs = SCENES[scene]
        poses = np.array([list(o.t) + list(o.q) for o in obs], dtype=np.float64)
        intr = np.array([o.intr for o in obs], dtype=np.float64)
        pts = np.array([_place(o.q, o.t, o.pc) for o in obs])
        uv = np.array([_uv(o.q, o.t, o.intr, p, o.r) for o, p in zip(obs, pts)])
        idx = np.arange(len(obs))
        _CACHE["iso", scene] = (_data(poses, intr, pts, idx, idx, uv, "projection-" + scene), obs)
    return _CACHE["iso", scene]


def second_point(d):
    """A second crafted point for the same structure: every camera turned and moved, every intrinsic and landmark changed,
    by amounts that keep each observation's classification far from the depth threshold it was not built at."""
    n = d.n_cam
    k = np.arange(n)
    poses = d.poses.copy()
    poses[:, 0:3] += 1e-3 * np.stack([np.cos(k), np.sin(k), 0 * k], -1)
    poses[:, 3:7] += 1e-3 * np.stack([np.sin(k), np.cos(2 * k), np.sin(3 * k), np.cos(k)], -1) * np.linalg.norm(poses[:, 3:7], axis=1)[:, None]
    intr = d.intr * (1 + 1e-3 * np.cos(k))[:, None]
    pts = d.points + 1e-3 * np.stack([np.sin(2 * k), np.cos(3 * k), 0 * k], -1)
    return poses, intr, pts


_A_Q = (np.cos(0.25), 0.0, np.sin(0.25), 0.0)      # +0.5 rad about y
_B_Q = (np.cos(0.25), 0.0, -np.sin(0.25), 0.0)     # -0.5 rad about y


def braced(scene):
    """(data, edge, obs): `edge` the indices of the edge observations in data's observation list, obs their specs.  Per edge
    observation: cameras E, A, B and landmarks L, P1, P2; observations E-L (the edge), A-L, B-L, E-P1, E-P2."""
    if ("braced", scene) not in _CACHE:
        obs = [o for o in SCENES[scene] if o.brace]
        poses, intr, pts, ci, li, uv, edge = [], [], [], [], [], [], []
        for o in obs:
            c0, l0 = len(poses), len(pts)
            t = o.t
            if o.claims.get("move_camera"):      # |p_c| = 1e6: the camera goes far away, not the landmark (the braces' rotational
                t = _camera_at(o.q, (0.1, 0.2, 0.3), o.pc)[0:3]   # columns a x p_w would carry the 1e6 into S otherwise)
            L = _place(o.q, t, o.pc)
            P1, P2 = _place(o.q, t, (0.2, 0.1, -1.0)), _place(o.q, t, (-0.3, 0.2, -1.5))
            poses += [np.array(list(t) + list(o.q)), _camera_at(_A_Q, L, (0.1, -0.1, -1.0)), _camera_at(_B_Q, L, (-0.1, 0.05, -1.0))]
            intr += [o.intr, INTR, INTR]
            far = bool(o.claims.get("move_camera"))     # (its ordinary landmarks would lie 1e6 from the origin too: it sees none)
            pts += [L] if far else [L, P1, P2]
            edge.append(len(ci))
            for c, l, r in ((0, 0, o.r), (1, 0, (0.3, -0.4)), (2, 0, (-0.4, 0.3)), (0, 1, (0.2, 0.3)), (0, 2, (-0.1, -0.45)))[:3 if far else 5]:
                ci.append(c0 + c); li.append(l0 + l)
                p = poses[c0 + c]
                uv.append(_uv(p[3:7], p[0:3], intr[c0 + c], pts[l0 + l], r))
        _CACHE["braced", scene] = (_data(np.array(poses), np.array(intr), np.array(pts), ci, li, np.array(uv), "projection-braced-" + scene),
                                   np.array(edge), obs)
    return _CACHE["braced", scene]


# ---- premises ------------------------------------------------------------------------------------------------------------------
def premises(d, obs, at, ref):
    """Assert what every case claims, on the long double re-derivation `ref` (projection_ref.reference of the rounded inputs);
    at[i] is the observation of spec obs[i]."""
    for a in (d.poses, d.intr, d.points, d.obs_uv):
        assert np.isfinite(a).all()
    for name in pr.QUANTITIES:
        assert np.isfinite(np.asarray(getattr(ref, name), dtype=np.float64)).all() and np.isfinite(getattr(ref, "M_" + name)).all(), name
    for o, i in zip(obs, at):
        z = float(ref.pc[i, 2])
        assert bool(ref.valid[i]) == o.valid, (o.name, z)
        # the classification: |z + 1e-6| beyond 1e3 times the rounding of p_c.z (the magnitude of its terms x 2^-53)
        assert abs(z + 1e-6) >= 1e3 * 2.0 ** -53 * float(ref.M_z[i]), (o.name, z, ref.M_z[i])
        assert np.allclose(np.asarray(ref.pc[i], dtype=np.float64), o.pc, rtol=1e-9, atol=64 * 2.0 ** -53 * float(ref.M_z[i]) + 1e-300), (o.name, ref.pc[i])
        c = o.claims
        if "depth_within" in c:
            assert abs(z / -1e-6 - 1.0) <= c["depth_within"] and abs(z / -1e-6 - 1.0) >= 5e-4, (o.name, z)
        if c.get("r2_zero"):
            assert ref.xn[i] == 0 and ref.yn[i] == 0 and ref.r2[i] == 0
        if c.get("xn_zero"):
            assert ref.xn[i] == 0 and ref.yn[i] != 0
        if c.get("yn_zero"):
            assert ref.yn[i] == 0 and ref.xn[i] != 0
        if "r2_about" in c:
            assert abs(float(ref.r2[i]) - c["r2_about"]) <= 0.5
        if "dist_about" in c:
            assert abs(float(ref.dist[i]) / c["dist_about"] - 1.0) <= 1e-6, (o.name, ref.dist[i])
        if "pw_about" in c:
            assert 0.5 <= np.linalg.norm(d.points[d.pt_idx[i]]) / c["pw_about"] <= 2.0
        if o.valid:
            rn = float(np.sqrt(ref.s[i]))
            want = float(np.hypot(*o.r))
            assert abs(rn / want - 1.0) <= 1e-3, (o.name, rn, want)
    # every s away from every branch of the loss: by 1e-6 relative and by 1e3 times the rounding of s itself
    for thr in nl.thresholds(ref.loss):
        s = np.asarray(ref.s, dtype=np.float64)[ref.valid]
        ms = np.asarray(ref.M_s, dtype=np.float64)[ref.valid]
        assert (np.abs(s - thr) >= np.maximum(1e-6 * thr, 1e3 * 2.0 ** -53 * ms)).all(), (ref.loss, thr, s)
