"""Reference arithmetic of the BAL projection factor, observation by observation -- TEST INFRASTRUCTURE ONLY (CPU;
tests/test_projection_ref_host.py, tests/test_gpu_projection_edges.py).

Written from the mathematical definition in the docstring of tests/np_ref.py, in np.longdouble (tile_ref.LD):

    R      rotation matrix of the twice-normalised stored quaternion          p_c = R p_w + t
    valid  p_c.z < -1e-6 (kMinDepth); an invalid observation has zero residual, zero rows and weight 0
    n      = -(p_c.x, p_c.y) / p_c.z       r2 = |n|^2       dist = 1 + k1 r2 + k2 r2^2       r = f dist n - uv
    d r / d p_c   = f (dist I + 2 (k1 + 2 k2 r2) n n^T) [ -1/z  0  x/z^2 ; 0  -1/z  y/z^2 ]
    d p_c / d delta = [R | -R [p_w]x]  (right perturbation delta = [rho; theta])        d p_c / d p_w = R
    d r / d (f, k1, k2) = n (dist, f r2, f r2^2)
    s = |r|^2,  w = sqrt(rho'(s)) from np_ref_loss.corrector (first arm: r~ = w r, J~ = w J),  column masks last

Every returned entry comes with the pair (M, k) of the rule of tests/schur_ref.py, err <= max(8 e_np, gamma(k) M):
  M  the magnitude of the terms the entry was summed from, carried through the whole evaluation: an input has M = |x|; a sum
     has M_a + M_b; a product has M_a |b| + |a| M_b - |a b| (first order: the relative magnitudes M / |x| add, less the one
     counted twice); 1 / a has M_a / a^2; sqrt has the relative magnitude of its operand; the loss weight w(s) has
     |w| (1 + |d log w / d log s| M_s / s), the logarithmic derivative taken by a central difference of the long double
     corrector.  For an entry without cancellation M is its absolute value; where R p_w + t cancels (|t| ~ 1e4, p_c = O(1)), or
     f dist n - uv cancels (|r| = 1e-9), M says by how much.
  k  the number of terms of the entry's own (final) sum, TERMS below: r = f dist n - uv has 2; w is one; an entry of Jl,
     sum_j (d r / d p_c)_j R_jc, has 3; an entry of Jc has at most 6 (a rotational column is a cross product of two such sums
     with p_w).  The roundings INSIDE a term are C0's business, as in schur_ref.py: the longest chain from the inputs to an
     entry is about 40 roundings (quaternion to R 8, p_c 3, reciprocal 2, n 1, r2 2, r4 1, dist 2, the derivative of dist 2,
     its products with n 3, d r / d p_c 3, times R 3, the cross product 2, s 3, the weight 4, the product with it 1), each at
     most u relative to M, well inside C0 = 114.
gamma is schur_ref.gamma, C0 = 114 unchanged; no constant here is fitted to any output of the code under test.

`reference` is the long double value; `restatement` the fp64 one (np_ref.jacobian_blocks, generalised to the loss family and
the column masks), whose distance e_np from `reference` is the conditioning yardstick, as in schur_ref.vec_check.

A loss is None (no loss), ("huber_delta", delta) (set_structure's legacy double: Huber of scale delta) or anything with .kind,
.p0, .p1 (apex_solver_amd.loss.Loss).  mask_code = 4 POSE + 2 LANDMARK + INTRINSIC; dc = 6 | 9 camera columns.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import np_ref
import np_ref_loss as nl
import schur_ref as sr
from apex_solver_amd import capi
from apex_solver_amd.loss import Loss
from tile_ref import LD

K_MIN_DEPTH = 1e-6
QUANTITIES = ("r_raw", "w", "r", "Jc", "Jl")
TERMS = dict(r_raw=2, w=1, r=2, Jc=6, Jl=3)


# ---- (value, magnitude) arithmetic ----------------------------------------------------------------------------------
class Q:
    __slots__ = ("v", "m")

    def __init__(self, v, m=None):
        self.v = np.asarray(v, dtype=LD)
        self.m = np.abs(self.v) if m is None else np.asarray(m, dtype=LD)

    def __neg__(self):
        return Q(-self.v, self.m)

    def __add__(self, o):
        o = _q(o)
        return Q(self.v + o.v, self.m + o.m)

    def __sub__(self, o):
        return self + (-_q(o))

    def __mul__(self, o):
        o = _q(o)
        a, b = np.abs(self.v), np.abs(o.v)
        return Q(self.v * o.v, self.m * b + a * o.m - a * b)

    __radd__ = __add__
    __rmul__ = __mul__

    def recip(self):
        return Q(1 / self.v, self.m / (self.v * self.v))

    def sqrt(self):
        r = np.sqrt(self.v)
        return Q(r, r * self.m / np.abs(self.v))


def _q(x):
    return x if isinstance(x, Q) else Q(x)


def _rotation(q):
    """q: four Q (w, x, y, z) as stored -> 3 x 3 of Q, the rotation of the twice-normalised quaternion"""
    for _ in range(2):
        inv = (q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]).sqrt().recip()
        q = [c * inv for c in q]
    w, i, j, k = q
    ww, ii, jj, kk = w * w, i * i, j * j, k * k
    return [[ww + ii - jj - kk, (i * j - w * k) * 2, (w * j + i * k) * 2],
            [(w * k + i * j) * 2, ww - ii + jj - kk, (j * k - w * i) * 2],
            [(i * k - w * j) * 2, (w * i + j * k) * 2, ww - ii - jj + kk]]


# ---- the loss ------------------------------------------------------------------------------------------------------------------
def as_loss(loss):
    if loss is None:
        return Loss(capi.LOSS_NONE)
    if isinstance(loss, tuple):
        assert loss[0] == "huber_delta"
        return Loss(capi.LOSS_HUBER, float(loss[1])) if loss[1] > 0 else Loss(capi.LOSS_NONE)
    return loss


def loss_weight(loss, s):
    """sqrt(rho'(s)) in long double at the fp64 squared norm; the corrector takes its first arm"""
    sq, rs, a, arm = nl.corrector(loss, float(s))
    assert arm == 1 and float(a) == 0.0 and rs == sq, (loss, s)
    return LD(sq)


def _weight(loss, sQ):
    """w(s) per observation as a Q"""
    n = len(sQ.v)
    w, m = np.ones(n, dtype=LD), np.ones(n, dtype=LD)
    h = LD(1e-7)
    for i in range(n):
        s = sQ.v[i]
        w[i] = loss_weight(loss, s)
        if w[i] == 0 or s == 0:
            m[i] = abs(w[i])
            continue
        up, dn = loss_weight(loss, s * (1 + h)), loss_weight(loss, s * (1 - h))
        sens = abs(up - dn) / (2 * h * w[i])
        m[i] = abs(w[i]) * (1 + sens * sQ.m[i] / s)
    return Q(w, m)


# ---- the long double reference ------------------------------------------------------------------------------------------------
def reference(poses, intr, pts, cam_idx, pt_idx, obs_uv, loss=None, mask_code=7, dc=9):
    """Per observation: valid, pc, xn, yn, r2, dist, s (the premises' quantities, long double), and for each name in QUANTITIES
    the value `name`, the magnitude `M_name` and the roundings `k_name`: r_raw (n, 2), w (n,), r (n, 2), Jc (n, 2, dc),
    Jl (n, 2, 3)."""
    loss = as_loss(loss)
    ci, li = np.asarray(cam_idx, dtype=np.int64), np.asarray(pt_idx, dtype=np.int64)
    P, I, X, UV = (np.asarray(a, dtype=np.float64) for a in (poses, intr, pts, obs_uv))
    n = len(ci)
    t = [Q(P[ci, a]) for a in range(3)]
    R = _rotation([Q(P[ci, 3 + a]) for a in range(4)])
    pw = [Q(X[li, a]) for a in range(3)]
    f, k1, k2 = (Q(I[ci, a]) for a in range(3))
    pc = [R[a][0] * pw[0] + R[a][1] * pw[1] + R[a][2] * pw[2] + t[a] for a in range(3)]
    valid = pc[2].v < LD(K_MIN_DEPTH) * -1
    z = Q(np.where(valid, pc[2].v, LD(-1)), np.where(valid, pc[2].m, LD(1)))   # (finite stand-in; zeroed below)
    inz = -z.recip()
    xn, yn = pc[0] * inz, pc[1] * inz
    r2 = xn * xn + yn * yn
    r4 = r2 * r2
    dist = k2 * r4 + k1 * r2 + 1
    raw = [f * (xn * dist) - Q(UV[:, 0]), f * (yn * dist) - Q(UV[:, 1])]
    dd = (k2 * r2) * 2 + k1
    dxx, dxy, dyy = (dd * xn * xn) * 2 + dist, (dd * xn * yn) * 2, (dd * yn * yn) * 2 + dist
    Jp = [[f * (dxx * inz), f * (dxy * inz), f * ((dxx * xn + dxy * yn) * inz)],
          [f * (dxy * inz), f * (dyy * inz), f * ((dxy * xn + dyy * yn) * inz)]]
    s = raw[0] * raw[0] + raw[1] * raw[1]
    sv = Q(np.where(valid, s.v, LD(0)), np.where(valid, s.m, LD(0)))
    w = _weight(loss, sv)
    m_pose, m_lm, m_intr = (1 if mask_code & b else 0 for b in (4, 2, 1))
    Jc, Jl, r = [[None] * dc for _ in range(2)], [[None] * 3 for _ in range(2)], [None, None]
    for rr in range(2):
        a = [Jp[rr][0] * R[0][c] + Jp[rr][1] * R[1][c] + Jp[rr][2] * R[2][c] for c in range(3)]
        for c in range(3):
            Jl[rr][c] = a[c] * w * m_lm
            Jc[rr][c] = a[c] * w * m_pose
        Jc[rr][3] = (a[2] * pw[1] - a[1] * pw[2]) * w * m_pose
        Jc[rr][4] = (a[0] * pw[2] - a[2] * pw[0]) * w * m_pose
        Jc[rr][5] = (a[1] * pw[0] - a[0] * pw[1]) * w * m_pose
        if dc == 9:
            nn = xn if rr == 0 else yn
            Jc[rr][6], Jc[rr][7], Jc[rr][8] = (nn * dist) * w * m_intr, (f * nn * r2) * w * m_intr, (f * nn * r4) * w * m_intr
        r[rr] = raw[rr] * w

    out = SimpleNamespace(n=n, dc=dc, valid=valid, pc=np.stack([c.v for c in pc], -1), xn=xn.v, yn=yn.v, r2=r2.v, dist=dist.v,
                          s=sv.v, M_s=sv.m, M_z=pc[2].m, loss=loss, mask_code=mask_code)

    def put(name, qs, shape):
        flat = [x for row in qs for x in row] if isinstance(qs[0], list) else list(qs)
        zero = lambda a: np.where(valid, a, LD(0))
        setattr(out, name, np.stack([zero(x.v) for x in flat], -1).reshape((n,) + shape))
        setattr(out, "M_" + name, np.stack([zero(x.m) for x in flat], -1).reshape((n,) + shape).astype(np.float64))
        setattr(out, "k_" + name, TERMS[name])

    put("r_raw", raw, (2,)); put("w", [w], ()); put("r", r, (2,)); put("Jc", Jc, (2, dc)); put("Jl", Jl, (2, 3))
    return out


def masked(ref, mask_code, dc):
    """The reference (or restatement) of mask 7, dc 9 under another mask and column count: masked columns are exact zeros"""
    import copy
    out = copy.copy(ref)
    m_pose, m_lm, m_intr = (1 if mask_code & b else 0 for b in (4, 2, 1))
    cm = np.array([m_pose] * 6 + [m_intr] * 3)[:dc]
    for pre in ("", "M_"):
        if hasattr(ref, pre + "Jc"):
            setattr(out, pre + "Jc", getattr(ref, pre + "Jc")[:, :, :dc] * cm)
            setattr(out, pre + "Jl", getattr(ref, pre + "Jl") * m_lm)
    out.dc, out.mask_code = dc, mask_code
    return out


# ---- the fp64 restatement -----------------------------------------------------------------------------------------------------
def restatement(poses, intr, pts, cam_idx, pt_idx, obs_uv, loss=None, mask_code=7, dc=9):
    """The same quantities in fp64 through np_ref.jacobian_blocks (another formulation: one normalisation, 1 - 2 (y^2 + z^2),
    matrix products), the weight rounded from the long double corrector at the fp64 squared norm."""
    loss = as_loss(loss)
    ci, li = np.asarray(cam_idx, dtype=np.int64), np.asarray(pt_idx, dtype=np.int64)
    P, I, X, UV = (np.asarray(a, dtype=np.float64) for a in (poses, intr, pts, obs_uv))
    raw, _, Jp, Jl, Ji = np_ref.jacobian_blocks(P, I, X, ci, li, UV, huber_delta=0)
    _, valid, _, _ = np_ref.project(P, I, X, ci, li)
    s = raw[:, 0] * raw[:, 0] + raw[:, 1] * raw[:, 1]
    w = np.array([float(loss_weight(loss, x)) for x in s]) * valid
    m_pose, m_lm, m_intr = (1.0 if mask_code & b else 0.0 for b in (4, 2, 1))
    Jc = np.concatenate([Jp * m_pose, Ji * m_intr], axis=2)[:, :, :dc] * w[:, None, None]
    return SimpleNamespace(n=len(ci), dc=dc, valid=valid, r_raw=raw, w=w, r=raw * w[:, None], Jc=Jc, Jl=Jl * m_lm * w[:, None, None], s=s)


# ---- the Schur system of a scene from the reference's blocks ------------------------------------------------------------------
def schur_pair(d, ld, f64, dc, mask_code, lam):
    """(long double schur_ref.SchurRef from the reference's Jc, Jl, r with their magnitudes -- the blocks themselves are on trial
    here, see SchurRef's `mags` --, fp64 one from the restatement's)"""
    a, b = masked(ld, mask_code, dc), masked(f64, mask_code, dc)
    ci, li = np.asarray(d.cam_idx, dtype=np.int64), np.asarray(d.pt_idx, dtype=np.int64)
    return (sr.SchurRef(d.n_cam, d.n_pt, ci, li, a.Jc, a.Jl, a.r, lam, LD, mags=(a.M_Jc, a.M_Jl, ld.M_r)),
            sr.SchurRef(d.n_cam, d.n_pt, ci, li, b.Jc, b.Jl, b.r, lam, np.float64))


# ---- the rule, per entry ---------------------------------------------------------------------------------------------------------
def entry_ratio(dev, ld, f64, name):
    """err / max(8 e_np, gamma(k) M) for every entry of quantity `name` (schur_ref.vec_check's rule with one entry per row)"""
    ref = getattr(ld, name)
    mag = getattr(ld, "M_" + name).reshape(-1)
    ratio = sr.vec_check(np.asarray(dev).reshape(-1), ref.reshape(-1), np.asarray(getattr(f64, name)).reshape(-1), mag, getattr(ld, "k_" + name))
    return ratio.reshape(ref.shape)


def cost_terms(ld):
    """(long double cost 1/2 sum |r~|^2, the magnitude of its terms, their number n: one term per observation)"""
    c = LD(0.5) * (ld.r * ld.r).sum()
    ar = np.abs(ld.r)
    mag = float((LD(0.5) * (2 * ld.M_r.astype(LD) * ar - ar * ar)).sum())       # M of r^2 is 2 M_r |r| - r^2
    return c, mag, ld.n


def report(label, ratios):
    """One PROJREF line: the worst ratio of every checked quantity and where it sits"""
    parts = []
    for name, r in ratios.items():
        v, at = sr.worst(r)
        parts.append(f"{name} {v:.3g}@{','.join(str(a) for a in at)}")
    print(f"PROJREF {label}: " + "  ".join(parts))


# ---- finite differences of the reference's own residual (long double) ------------------------------------------------------------
def raw_projection(R, t, intr, pw):
    """f dist n of one observation, plainly, in long double: (3, 3), (3,), (3,), (3,) -> (2,)"""
    X, Y, Z = R @ pw + t
    xn, yn = -X / Z, -Y / Z
    r2 = xn * xn + yn * yn
    d = 1 + intr[1] * r2 + intr[2] * r2 * r2
    return np.array([intr[0] * xn * d, intr[0] * yn * d], dtype=LD)


def rotation_ld(q):
    q = np.asarray(q, dtype=LD)
    w, x, y, z = q / np.sqrt((q * q).sum())
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], dtype=LD)


def _exp_axis(axis, h):
    K = np.zeros((3, 3), dtype=LD)
    e = np.zeros(3, dtype=LD); e[axis] = 1
    K[0, 1], K[0, 2], K[1, 0], K[1, 2], K[2, 0], K[2, 1] = -e[2], e[1], e[2], -e[0], -e[1], e[0]
    return np.eye(3, dtype=LD) + np.sin(h) * K + (1 - np.cos(h)) * (K @ K)


def finite_differences(pose, intr, pw, rel=1e-6):
    """Central differences of raw_projection in the 12 columns [rho 3 | theta 3 | f k1 k2 | p_w 3] of one valid observation,
    (2, 12) long double.  The step of each column is `rel` times the length over which the projection changes: |z| for a
    translation or the point, |z| / |p_w| for a rotation (it moves p_c by h |p_w|), the parameter's own size (or 1) for an
    intrinsic, in which the projection is linear."""
    pose, intr, pw = (np.asarray(a, dtype=np.float64).astype(LD) for a in (pose, intr, pw))
    R, t = rotation_ld(pose[3:7]), pose[0:3]
    depth = abs((R @ pw + t)[2])
    out = np.zeros((2, 12), dtype=LD)
    f = lambda R_, t_, i_, p_: raw_projection(R_, t_, i_, p_)
    for a in range(3):
        h = LD(rel) * depth
        e = np.zeros(3, dtype=LD); e[a] = h
        out[:, a] = (f(R, t + R @ e, intr, pw) - f(R, t - R @ e, intr, pw)) / (2 * h)
        out[:, 9 + a] = (f(R, t, intr, pw + e) - f(R, t, intr, pw - e)) / (2 * h)
        hr = LD(rel) * depth / max(np.sqrt((pw * pw).sum()), depth)
        out[:, 3 + a] = (f(R @ _exp_axis(a, hr), t, intr, pw) - f(R @ _exp_axis(a, -hr), t, intr, pw)) / (2 * hr)
        hi = LD(rel) * max(abs(intr[a]), LD(1))
        e = np.zeros(3, dtype=LD); e[a] = hi
        out[:, 6 + a] = (f(R, t, intr + e, pw) - f(R, t, intr - e, pw)) / (2 * hi)
    return out
