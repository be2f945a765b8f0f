"""The camera priors of bundle adjustment (csrc/ba_prior_kernels.hip) block by block in np.longdouble, with a
same-order fp64 restatement for the referee -- TEST INFRASTRUCTURE ONLY (tests/test_ba_prior_cases_host.py,
tests/test_gpu_ba_prior_crafted.py).

Per block k (camera c, data, delta, w), with x the camera's prepared vector (t, q / |q| normalised twice; f k1 k2):
    r = w (x - data)    s = sum_a r_a^2 (all rows)    rho' = delta / sqrt(s) where delta > 0 and s > delta^2, else 1
    r~ = sqrt(rho') r   j = sqrt(rho') w
Per camera column i (pose columns 0..5 take rows 0..5 of the pose blocks, intrinsics columns 6..8 the intrinsics blocks; the
seventh pose row has no column), over the camera's run of k_i blocks in the caller's order:
    p_i = sum j^2       q_i = sum j r~_a       cost_c = sum over all rows of r~_a^2
The Huber branch is taken with the fp64 value of s in the kernel's order of summation (as so3_ref / manifold_ref do), so the
reference stands on the device's side of the threshold; everything else is in `dtype`.

The rule (tests/schur_ref.py, tests/pg_asm_ref.py):  err <= max(8 e_np, bound),  bound = sum over the terms of
gamma(k_i + C0 + 2 e_k) |term|, gamma_m = m u / (1 - m u), u = 2^-53 (Higham ch. 3: a sum of k terms in any order is within
gamma_{k-1} sum |term|).  C0 counts the dependent roundings of one term in pose_prior_at / intr_prior_at and k_ba_prior_eval,
each at most u relative to the term:
    r_a = w (x_a - d_a)                                   2   (subtraction, product; x_a and d_a are inputs)
    s: seven products, six additions of non-negative terms 7   on top of 2 x 2 from the r_a it squares: 11
    sqrt(s) 1, delta / . 1, sqrt 1: sc                     3   -> sc carries 14 (no credit taken for the roots halving errors)
    j = sc w                                               1   -> 15
    r~_a = r_a sc                                          1   -> 2 + 14 + 1 = 17
    j * j                                                  1   -> 2 x 15 + 1 = 31        (p)
    j * r~_a                                               1   -> 15 + 17 + 1 = 33       (q)
    r~_a * r~_a                                            1   -> 2 x 17 + 1 = 35        (cost)
C0 = 35, the largest.  The quaternion rows have one more source: x_a itself is computed (load_cam: two passes of four products,
three additions, a root and a division: 4 u relative per pass, QX = 8 for the two), so the device's x_a and this file's differ
by up to QX u |x_a| whatever |x_a - d_a| is.  That is an ABSOLUTE error QX u j |x_a| of r~_a, carried by its own magnitude
beside the term's: q_i takes gamma(QX) j^2 |x_a| (rows 3..5: qw qx qy), the cost gamma(2 QX) |r~_a| j |x_a|.  Through s it
reaches sc of a corrected block: d s / s <= 2 QX u w sum_quat |r_a| |x_a| / s and sc = delta^(1/2) s^(-1/4), so sc moves by at most
e_k u with e_k = QX w sum_quat |r_a| |x_a| / s (twice what the exponent gives); a term holds sc at most twice: 2 e_k.
Nothing here is fitted to a device output."""
from __future__ import annotations

import numpy as np

import ba_prior_ref as br
from tile_ref import LD, U  # noqa: F401

C0 = 35
QX = 8


def gam(m):
    m = np.asarray(m, dtype=np.float64) * U
    return m / (1.0 - m)


def prepared(poses, T):
    """to_vector of the poses as load_cam prepares them, in T"""
    if T is np.float64:
        return br.pose_vector(poses)
    p = np.asarray(poses, dtype=T)
    q = p[:, 3:7]
    for _ in range(2):
        q = q / np.sqrt(np.sum(q * q, axis=1))[:, None]
    return np.concatenate([p[:, :3], q], axis=1)


class Blocks:
    """One set (pose: amb 7, intrinsics: amb 3) block by block, in the caller's order."""

    def __init__(self, xT, x64, priors, amb, T, s_rows=None):
        self.cam, data, self.delta, self.w = br._rows(priors, amb)
        n, cam, w, delta = len(self.cam), self.cam, self.w, self.delta
        rows = amb if s_rows is None else min(s_rows, amb)
        r64 = w[:, None] * (x64[cam] - data)
        s64 = np.zeros(n)
        for a in range(rows):
            s64 = s64 + r64[:, a] * r64[:, a]
        self.s64, self.out = s64, (delta > 0) & (s64 > delta * delta)
        r = np.asarray(w, dtype=T)[:, None] * (np.asarray(xT, dtype=T)[cam] - np.asarray(data, dtype=T))
        s = np.zeros(n, dtype=T)
        for a in range(rows):
            s = s + r[:, a] * r[:, a]
        sc = np.ones(n, dtype=T)
        o = self.out
        sc[o] = np.sqrt(np.asarray(delta[o], dtype=T) / np.sqrt(s[o]))
        self.r, self.sc, self.rt, self.j = r, sc, r * sc[:, None], sc * np.asarray(w, dtype=T)
        self.xa = np.abs(np.asarray(x64, dtype=np.float64)[cam]) if n else np.zeros((0, amb))
        e = np.zeros(n)
        if amb == 7 and n:
            quat = np.sum(np.abs(r64[:, 3:7]) * self.xa[:, 3:7], axis=1)
            e[o] = QX * w[o] * quat[o] / s64[o]
        self.e = e


class PriorRef:
    """p, q (n_cam, 9) with the intrinsics columns last (zero at d_c = 6), cost (n_cam,), their bounds pb, qb, cb (fp64), the
    run length k (n_cam, 9) and the term-magnitude sums pmag, qmag; rp (n_pose, 7), ri (n_intr, 3) the corrected residuals."""

    def __init__(self, poses, intr, pose_priors, intr_priors, dtype=LD, s_rows=None):
        T = self.T = dtype
        n_cam = self.n_cam = len(poses)
        self.P = Blocks(prepared(poses, T), br.pose_vector(poses), pose_priors, 7, T, s_rows)
        self.I = Blocks(np.asarray(intr, dtype=T), np.asarray(intr, dtype=np.float64), intr_priors, 3, T, s_rows)
        self.rp, self.ri = self.P.rt, self.I.rt
        self.p = np.zeros((n_cam, 9), dtype=T); self.q = np.zeros((n_cam, 9), dtype=T); self.cost = np.zeros(n_cam, dtype=T)
        self.pb = np.zeros((n_cam, 9)); self.qb = np.zeros((n_cam, 9)); self.cb = np.zeros(n_cam)
        self.pmag = np.zeros((n_cam, 9)); self.qmag = np.zeros((n_cam, 9)); self.k = np.zeros((n_cam, 9), dtype=np.int64)
        runs = np.zeros((n_cam, 2), dtype=np.int64)
        np.add.at(runs[:, 0], self.P.cam, 1); np.add.at(runs[:, 1], self.I.cam, 1)
        self.runs = runs
        rows = 7 * runs[:, 0] + 3 * runs[:, 1]
        for B, cols, which in ((self.P, range(6), 0), (self.I, range(6, 9), 1)):
            cam = B.cam
            if not len(cam):
                continue
            j64, rt64 = np.abs(np.asarray(B.j, dtype=np.float64)), np.abs(np.asarray(B.rt, dtype=np.float64))
            m = runs[cam, which] + C0 + 2.0 * B.e
            amb = B.rt.shape[1]
            quat = np.zeros(amb, dtype=bool)
            if amb == 7:
                quat[3:] = True
            for a, col in enumerate(cols):   # np.add.at adds in index order: a camera's run in the caller's order
                np.add.at(self.p[:, col], cam, B.j * B.j)
                np.add.at(self.q[:, col], cam, B.j * B.rt[:, a])
                np.add.at(self.pmag[:, col], cam, j64 * j64)
                np.add.at(self.qmag[:, col], cam, j64 * rt64[:, a])
                np.add.at(self.pb[:, col], cam, gam(m) * j64 * j64)
                np.add.at(self.qb[:, col], cam, gam(m) * j64 * rt64[:, a] + (gam(QX) * j64 * j64 * B.xa[:, a] if quat[a] else 0.0))
                np.add.at(self.k[:, col], cam, 1)
            mc = rows[cam] + C0 + 2.0 * B.e
            for a in range(amb):
                np.add.at(self.cost, cam, B.rt[:, a] * B.rt[:, a])
                np.add.at(self.cb, cam, gam(mc) * rt64[:, a] ** 2 + (gam(2 * QX) * rt64[:, a] * j64 * B.xa[:, a] if quat[a] else 0.0))

    def total_cost(self):
        """sum r~^2 over every row and the bound of its sum: the per-camera bounds plus one sum over the cameras"""
        c64 = np.asarray(self.cost, dtype=np.float64)
        return self.cost.sum(), float(self.cb.sum() + gam(self.n_cam) * c64.sum())


def pair(poses, intr, pose_priors, intr_priors):
    """(long double reference, fp64 restatement in the same order)"""
    return PriorRef(poses, intr, pose_priors, intr_priors, LD), PriorRef(poses, intr, pose_priors, intr_priors, np.float64)


def dist(a, b):
    return np.abs(np.asarray(a, dtype=LD) - np.asarray(b, dtype=LD)).astype(np.float64)


def ratio(err, bound):
    err = np.asarray(err, dtype=np.float64); bound = np.asarray(bound, dtype=np.float64)
    err, bound = np.broadcast_arrays(err, bound)
    out = np.zeros(err.shape)
    nz = bound > 0
    out[nz] = err[nz] / bound[nz]
    out[~nz & (err > 0)] = np.inf
    return out


def check(dev, ld_val, f64_val, bound, onto=0.0, roundings=1):
    """ratios of the rule: |dev - ld| against max(8 e_np, bound) + roundings u |onto|, `onto` being the value the device added
    the prior's part to (one rounding of that addition, relative to its result)"""
    return ratio(dist(dev, ld_val), np.maximum(8.0 * dist(f64_val, ld_val), bound) + roundings * U * np.abs(np.asarray(onto, dtype=np.float64)))


def worst(r):
    r = np.asarray(r)
    return float(r.max()) if r.size else 0.0
