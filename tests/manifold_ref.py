"""Cancellation-free long-double reference of the per-factor manifold math (SE3 and SE2 between factors, retractions,
Huber scale), and the edge cases the host and GPU tests share (CPU only; tests/test_manifold_ref_host.py,
tests/test_gpu_manifold_edges.py).

A restatement of the reference solver's formulas in exact-arithmetic spirit: the branches sit where the reference has them
(theta^2 against 1e-10), the Q block keeps its d coefficient as coded, input quaternions are normalised twice, a
retraction uses the stored quaternion as it is.  What differs from the fp64 oracles (oracle/pg_oracle.c, tests/np_ref_se2.py)
is how the coefficients that cancel are evaluated.  With S_n(t) = sum_k (-1)^k t^2k / (2k + n)!:

    sin t / t = S_1      (1 - cos t) / t^2 = S_2      (t - sin t) / t^3 = S_3
    (1 - t^2/2 - cos t) / t^4 = -S_4                  (t - sin t - t^3/6) / t^5 = -S_5
    1/t^2 - (1 + cos t) / (2 t sin t) = (1 - (t/2) cot(t/2)) / t^2 = sum_k |B_2k| t^(2k-2) / (2k)!

each by its series below |t| = SERIES_BELOW and by the closed form above (1 - cos t as 2 sin^2(t/2)).  Trigonometry goes
through libm's long-double routines.  tests/test_manifold_ref_host.py holds every function to 2^-60 of a 60-digit mpmath
evaluation of the literal formulas (measured worst, in units of 2^-60: SE3 residuals 0.62, Jacobians 0.84).

Everything is batched: poses (n, 7) = [t, qw, qx, qy, qz], tangents (n, 6) = [rho, theta]; SE2 poses and tangents (n, 3) =
[x, y, theta].  Inputs are fp64 (taken exactly), outputs long double.
"""
from __future__ import annotations

from fractions import Fraction
from math import factorial

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, "the long double references need an 80-bit (or wider) long double"

SMALL2 = 1e-10          # SMALL_ANGLE_THRESHOLD, compared with theta^2 (apex-manifolds/src/lib.rs:61)
SERIES_BELOW = 0.5      # |t| below which the cancelling coefficients come from their series
_TERMS = 14             # t^28 / 29! at t = 0.5: 2^-130


def _ld(x):
    return np.asarray(x, dtype=np.float64).astype(LD) if not (isinstance(x, np.ndarray) and x.dtype == LD) else x


def _frac_ld(f: Fraction):
    return LD(f.numerator) / LD(f.denominator)


def _series(n, t):
    """S_n(t) = sum_k (-1)^k t^2k / (2k + n)!, Horner in t^2"""
    t2 = t * t
    acc = np.zeros_like(t2)
    for k in reversed(range(_TERMS)):
        acc = _frac_ld(Fraction((-1) ** k, factorial(2 * k + n))) + t2 * acc
    return acc


def _bernoulli(m):
    B = [Fraction(0)] * (m + 1)
    B[0] = Fraction(1)
    for n in range(1, m + 1):
        B[n] = -sum(Fraction(factorial(n + 1), factorial(k) * factorial(n + 1 - k)) * B[k] for k in range(n)) / (n + 1)
    return B


_B = _bernoulli(2 * _TERMS + 2)
_COT = [abs(_B[2 * k]) / factorial(2 * k) for k in range(1, _TERMS + 2)]   # (t / 2pi)^2 per term: 2^-100 after 14 at 0.5


def _join(t, series, closed):
    small = np.abs(t) < SERIES_BELOW
    ts = np.where(small, LD(1), t)       # keep the unused branch finite
    return np.where(small, series(np.where(small, t, LD(0))), closed(ts))


def sinc(t):
    return _join(t, lambda x: _series(1, x), lambda x: np.sin(x) / x)


def one_minus_cos_over_t2(t):
    return _join(t, lambda x: _series(2, x), lambda x: 2 * np.sin(x / 2) ** 2 / (x * x))


def t_minus_sin_over_t3(t):
    return _join(t, lambda x: _series(3, x), lambda x: (x - np.sin(x)) / (x * x * x))


def q_c(t):
    """(1 - t^2/2 - cos t) / t^4"""
    return _join(t, lambda x: -_series(4, x), lambda x: (2 * np.sin(x / 2) ** 2 - x * x / 2) / (x * x) ** 2)


def q_dnum_over_t5(t):
    """(t - sin t - t^3/6) / t^5"""
    return _join(t, lambda x: -_series(5, x), lambda x: (x - np.sin(x) - x * x * x / 6) / (x * x * x * x * x))


def jlinv_coef(t):
    """1/t^2 - (1 + cos t) / (2 t sin t), through cot(t/2)"""
    def ser(x):
        x2 = x * x
        acc = np.zeros_like(x2)
        for c in reversed(_COT):
            acc = _frac_ld(c) + x2 * acc
        return acc
    return _join(t, ser, lambda x: (1 - (x / 2) * np.cos(x / 2) / np.sin(x / 2)) / (x * x))


# ---- small linear algebra, batched -------------------------------------------------------------------------------------
# Every inner product is compensated (Ogita, Rump, Oishi: Dot2 with Dekker's product): its result is the long-double rounding
# of a sum accumulated in twice the precision, so what is left of the reference's error is the rounding of stored values.
_SPLIT = LD(2 ** 32 + 1)


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    p = a * b
    ca, cb = _SPLIT * a, _SPLIT * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _dot(a, b):
    """sum over the last axis of a * b"""
    a, b = np.broadcast_arrays(a, b)
    p, s = _two_prod(a[..., 0], b[..., 0])
    for i in range(1, a.shape[-1]):
        h, r = _two_prod(a[..., i], b[..., i])
        p, q = _two_sum(p, h)
        s = s + (q + r)
    return p + s


def _terms(*pairs):
    """sum of products x_i y_i given as (x_0, y_0), (x_1, y_1), ..."""
    xs = np.broadcast_arrays(*[np.asarray(x, dtype=LD) for x, _ in pairs], *[np.asarray(y, dtype=LD) for _, y in pairs])
    k = len(pairs)
    return _dot(np.stack(xs[:k], -1), np.stack(xs[k:], -1))


def _mm(A, B):
    return _dot(A[..., :, None, :], np.swapaxes(B, -1, -2)[..., None, :, :])


def _hat(v):
    z = np.zeros_like(v[..., 0])
    return np.stack([np.stack([z, -v[..., 2], v[..., 1]], -1), np.stack([v[..., 2], z, -v[..., 0]], -1),
                     np.stack([-v[..., 1], v[..., 0], z], -1)], -2)


def _cross(a, b):
    return np.stack([_terms((a[..., 1], b[..., 2]), (-a[..., 2], b[..., 1])), _terms((a[..., 2], b[..., 0]), (-a[..., 0], b[..., 2])),
                     _terms((a[..., 0], b[..., 1]), (-a[..., 1], b[..., 0]))], -1)


def _mv(M, v):
    return _dot(M, v[..., None, :])


def _eye(n, k):
    return np.broadcast_to(np.eye(k, dtype=LD), (n, k, k)).copy()


# ---- quaternions [w, x, y, z] and SE3 ----------------------------------------------------------------------------------
def _qmul(a, b):
    a0, a1, a2, a3 = (a[..., i] for i in range(4))
    b0, b1, b2, b3 = (b[..., i] for i in range(4))
    return np.stack([_terms((a0, b0), (-a1, b1), (-a2, b2), (-a3, b3)), _terms((a0, b1), (b0, a1), (a2, b3), (-a3, b2)),
                     _terms((a0, b2), (b0, a2), (a3, b1), (-a1, b3)), _terms((a0, b3), (b0, a3), (a1, b2), (-a2, b1))], -1)


def _qconj(q):
    return np.concatenate([q[..., :1], -q[..., 1:]], -1)


def _qrot(q, v):
    """q v q* as the reference multiplies it (t = 2 qv x v; t w + qv x t + v); q is used as it is"""
    t = 2 * _cross(q[..., 1:], v)
    w, x, y, z = (q[..., i] for i in range(4))
    one = np.ones_like(w)
    return np.stack([_terms((t[..., 0], w), (y, t[..., 2]), (-z, t[..., 1]), (v[..., 0], one)),
                     _terms((t[..., 1], w), (z, t[..., 0]), (-x, t[..., 2]), (v[..., 1], one)),
                     _terms((t[..., 2], w), (x, t[..., 1]), (-y, t[..., 0]), (v[..., 2], one))], -1)


def _q_to_R(q):
    w, x, y, z = (q[..., i] for i in range(4))
    x2, y2, z2 = 2 * x, 2 * y, 2 * z
    return np.stack([np.stack([_terms((w, w), (x, x), (-y, y), (-z, z)), _terms((x2, y), (-w, z2)), _terms((w, y2), (x2, z))], -1),
                     np.stack([_terms((w, z2), (x2, y)), _terms((w, w), (-x, x), (y, y), (-z, z)), _terms((y2, z), (-w, x2))], -1),
                     np.stack([_terms((x2, z), (-w, y2)), _terms((w, x2), (y2, z)), _terms((w, w), (-x, x), (-y, y), (z, z))], -1)], -2)


def se3_from_vec(v):
    """SE3::from(DVector): the quaternion normalised twice"""
    v = _ld(np.atleast_2d(v))
    q = v[:, 3:]
    for _ in range(2):
        q = q / np.sqrt(_dot(q, q))[:, None]
    return v[:, :3], q


def _inv(t, q):
    qi = _qconj(q)
    return -_qrot(qi, t), qi


def _mul(ta, qa, tb, qb):
    return _qrot(qa, tb) + ta, _qmul(qa, qb)


def so3_log(q):
    s2 = _dot(q[:, 1:], q[:, 1:])
    big = s2 > SMALL2
    s = np.sqrt(np.where(big, s2, LD(1)))
    c = q[:, 0]
    two = 2 * np.where(c < 0, np.arctan2(-s, -c), np.arctan2(s, c))
    return q[:, 1:] * np.where(big, two / s, LD(2))[:, None]


def so3_left_jacobian_inv(th):
    a = (th * th).sum(-1)
    big = a > SMALL2
    c2 = np.where(big, jlinv_coef(np.sqrt(np.where(big, a, LD(1)))), LD(0))
    K = _hat(th)
    return _eye(len(th), 3) - K / 2 + c2[:, None, None] * _mm(K, K)


def se3_q_block(rho, th):
    """Q(rho, theta) as the reference codes it (se3.rs:520-558), its d coefficient included"""
    Rk, Tk = _hat(rho), _hat(th)
    t2 = (th * th).sum(-1)
    big = t2 > SMALL2
    t = np.sqrt(np.where(big, t2, LD(1)))
    b = np.where(big, t_minus_sin_over_t3(t), LD(1) / 6 + t2 / 120)
    c = np.where(big, q_c(t), -LD(1) / 24 + t2 / 720)
    d = np.where(big, (c - 3) * q_dnum_over_t5(t), -LD(1) / 60)
    tr, rt = _mm(Tk, Rk), _mm(Rk, Tk)
    trt, rtt = _mm(tr, Tk), _mm(rt, Tk)
    trtt = _mm(trt, Tk)
    e = lambda x: x[:, None, None]
    return Rk / 2 + (tr + rt + trt) * e(b) - (rtt - np.swapaxes(rtt, -1, -2) - 3 * trt) * e(c) - trtt * e(d)


def _adjoint_inv(t, q):
    """Adj((t, q)^-1) = [R^T, -R^T [t]x; 0, R^T]: what the reference forms as Adj of the inverted pose, [-R^T t]x R^T, without
    the rotated translation in between"""
    Rt = np.swapaxes(_q_to_R(q), -1, -2)
    A = np.zeros((len(t), 6, 6), dtype=LD)
    A[:, :3, :3] = Rt; A[:, 3:, 3:] = Rt; A[:, :3, 3:] = -_mm(Rt, _hat(t))
    return A


def se3_between(k0, k1, meas):
    """r (n, 6), J (n, 6, 12) = [dr/dk0 | dr/dk1] of r = Log((k1^-1 k0) meas) (between_factor.rs:268-322), uncorrected"""
    (t0, q0), (t1, q1), (tm, qm) = se3_from_vec(k0), se3_from_vec(k1), se3_from_vec(meas)
    tA, qA = _mul(*_inv(t1, q1), t0, q0)
    tD, qD = _mul(tA, qA, tm, qm)
    th = so3_log(qD)
    D = so3_left_jacobian_inv(th)
    rho = _mv(D, tD)
    r = np.concatenate([rho, th], -1)
    Q = se3_q_block(-rho, -th)
    Jlog = np.zeros((len(r), 6, 6), dtype=LD)
    Jlog[:, :3, :3] = D; Jlog[:, 3:, 3:] = D; Jlog[:, :3, 3:] = -_mm(_mm(D, Q), D)
    Am = _adjoint_inv(tm, qm)
    J0 = _mm(Jlog, Am)
    # Adj(meas^-1) (-Adj(A^-1)) = -Adj((A meas)^-1): the same matrix in exact arithmetic, without the products of the two
    # translations that cancel in it
    J1 = _mm(Jlog, -_adjoint_inv(tD, qD))
    return r, np.concatenate([J0, J1], -1)


def se3_plus(pose, delta):
    """pose (+) delta = pose * Exp(delta) on the stored (un-normalised) quaternion, stored un-normalised"""
    p, d = _ld(np.atleast_2d(pose)), _ld(np.atleast_2d(delta))
    rho, th = d[:, :3], d[:, 3:]
    a = (th * th).sum(-1)
    big = a > SMALL2
    t = np.sqrt(np.where(big, a, LD(1)))
    n = t / 2
    qe_big = np.concatenate([np.cos(n)[:, None], (th / 2) * sinc(n)[:, None]], -1)
    qs = np.concatenate([np.ones((len(th), 1), dtype=LD), th / 2], -1)
    qe_small = qs / np.sqrt((qs * qs).sum(-1))[:, None]
    qe = np.where(big[:, None], qe_big, qe_small)
    k1 = _cross(th, rho)
    k2 = _cross(th, k1)
    c1 = np.where(big, one_minus_cos_over_t2(t), LD(1) / 2)
    c2 = np.where(big, t_minus_sin_over_t3(t), LD(0))
    te = rho + c1[:, None] * k1 + c2[:, None] * k2
    return np.concatenate([_qrot(p[:, 3:], te) + p[:, :3], _qmul(p[:, 3:], qe)], -1)


def huber_scale(delta, s):
    """sqrt(rho') of HuberLoss at the squared norm s; delta None or <= 0: no loss"""
    s = np.asarray(s, dtype=LD)
    if delta is None or delta <= 0:
        return np.ones_like(s)
    dl = LD(delta)
    over = s > dl * dl
    return np.where(over, np.sqrt(dl / np.sqrt(np.where(over, s, LD(1)))), LD(1))


# ---- SE2 (signatures of tests/np_ref_se2.py) ---------------------------------------------------------------------------
def _se2_mat(v):
    v = _ld(np.atleast_2d(v))
    c, s = np.cos(v[:, 2]), np.sin(v[:, 2])
    T = np.zeros((len(v), 3, 3), dtype=LD)
    T[:, 0, 0] = c; T[:, 0, 1] = -s; T[:, 0, 2] = v[:, 0]
    T[:, 1, 0] = s; T[:, 1, 1] = c; T[:, 1, 2] = v[:, 1]
    T[:, 2, 2] = 1
    return T


def _se2_inv(T):
    Ti = np.zeros_like(T)
    Rt = np.swapaxes(T[:, :2, :2], -1, -2)
    Ti[:, :2, :2] = Rt
    Ti[:, :2, 2] = -_mv(Rt, T[:, :2, 2])
    Ti[:, 2, 2] = 1
    return Ti


def _se2_adjoint(T):
    A = np.zeros_like(T)
    A[:, :2, :2] = T[:, :2, :2]
    A[:, 0, 2] = T[:, 1, 2]; A[:, 1, 2] = -T[:, 0, 2]; A[:, 2, 2] = 1
    return A


def _se2_ab(th):
    """sin t / t and (1 - cos t) / t with the reference's Taylor branch below the threshold"""
    t2 = th * th
    small = t2 < SMALL2
    a = np.where(small, 1 - t2 / 6, sinc(th))
    b = np.where(small, th / 2 - th * t2 / 24, th * one_minus_cos_over_t2(th))
    return a, b


def se2_between(k0, k1, m):
    """r (n, 3), J (n, 3, 6) = [dr/dk0 | dr/dk1] of r = Log((k1^-1 k0) m), uncorrected"""
    K0, K1, M = _se2_mat(k0), _se2_mat(k1), _se2_mat(m)
    A = _se2_inv(K1) @ K0
    D = A @ M
    th = np.arctan2(D[:, 1, 0], D[:, 0, 0])
    a, b = _se2_ab(th)
    den = a * a + b * b
    x, y = D[:, 0, 2], D[:, 1, 2]
    r = np.stack([(a * x + b * y) / den, (-b * x + a * y) / den, th], -1)
    # Jr^-1 (se2.rs:577-613): J00 = (t/2) cot(t/2), J02 = y/2 + x k, J12 = -x/2 + y k, k = (1 - J00) / t = t jlinv_coef(t)
    rx, ry = r[:, 0], r[:, 1]
    t2 = th * th
    big = t2 > SMALL2
    cf = jlinv_coef(np.where(big, np.abs(th), LD(1)))
    d = np.where(big, 1 - t2 * cf, 1 - t2 / 12)
    k = np.where(big, th * cf, th / 12)
    Jl = np.zeros((len(th), 3, 3), dtype=LD)
    Jl[:, 0, 0] = d; Jl[:, 1, 1] = d; Jl[:, 2, 2] = 1
    Jl[:, 0, 1] = -th / 2; Jl[:, 1, 0] = th / 2
    Jl[:, 0, 2] = ry / 2 + rx * k; Jl[:, 1, 2] = -rx / 2 + ry * k
    Am = _se2_adjoint(_se2_inv(M))
    J0 = Jl @ Am
    J1 = Jl @ (Am @ -_se2_adjoint(_se2_inv(A)))
    return r, np.concatenate([J0, J1], -1)


def se2_plus(v, d):
    """x (+) d = x * Exp(d) in vector form; x (+) 0 = x"""
    vv, dd = _ld(np.atleast_2d(v)), _ld(np.atleast_2d(d))
    th = dd[:, 2]
    a, b = _se2_ab(th)
    E = _se2_mat(np.zeros((len(th), 3)))
    E[:, 0, 0] = np.cos(th); E[:, 0, 1] = -np.sin(th); E[:, 1, 0] = np.sin(th); E[:, 1, 1] = np.cos(th)
    E[:, 0, 2] = a * dd[:, 0] - b * dd[:, 1]; E[:, 1, 2] = b * dd[:, 0] + a * dd[:, 1]
    T = _se2_mat(vv) @ E
    out = np.stack([T[:, 0, 2], T[:, 1, 2], np.arctan2(T[:, 1, 0], T[:, 0, 0])], -1)
    return np.where(np.all(dd == 0, axis=-1)[:, None], vv, out)


# ---- errors and the referee ----------------------------------------------------------------------------------------------
def err(x, ref):
    """per case (leading axis): max |x - ref| over max(1, max |ref|)"""
    ref = np.asarray(ref, dtype=LD)
    n = ref.shape[0]
    num = np.abs(np.asarray(x).astype(LD) - ref).reshape(n, -1).max(-1)
    den = np.maximum(1, np.abs(ref).reshape(n, -1).max(-1))
    return (num / den).astype(np.float64)


FLOOR_R, FLOOR_J, FLOOR_H = 1e-13, 1e-12, 1e-12     # tests/test_pg_device_math_host.py
FLOOR_POSE = 1e-13 + 1e-15                          # tests/test_gpu_fixed_dofs.py: rtol 1e-13 plus atol 1e-15
CAP_J, CAP_R = 1e-8, 1e-10                          # what the fp64 oracle may itself be off by on a case that is kept


def referee(e_dev, e_oracle, floor):
    """tile_ref.referee per case: (all hold, index of the worst excess)"""
    e_dev, e_oracle = np.atleast_1d(e_dev), np.atleast_1d(e_oracle)
    bound = np.maximum(8.0 * e_oracle, floor)
    return bool((e_dev <= bound).all()), int(np.argmax(e_dev / bound))


BANDS = ((0.0, 1e-5), (1e-5, 1e-3), (1e-3, 0.5), (0.5, 3.0), (3.0, np.inf))
BAND_NAMES = ("<1e-5", "1e-5..1e-3", "1e-3..0.5", "0.5..3", ">3")


def band_of(angle):
    angle = np.abs(np.asarray(angle, dtype=np.float64))
    return np.array([next(i for i, (lo, hi) in enumerate(BANDS) if lo <= a < hi) for a in angle.ravel()]).reshape(angle.shape)


def report(tag, angle, **cols):
    """one MANIFOLD line: per band of `angle`, the worst of every column"""
    b = band_of(angle)
    parts = []
    for i, name in enumerate(BAND_NAMES):
        if (b == i).any():
            parts.append(name + " n=%d " % int((b == i).sum()) + " ".join(f"{k}={np.asarray(v)[b == i].max():.1e}" for k, v in cols.items()))
    print(f"MANIFOLD {tag}: " + " | ".join(parts))


# ---- the cases ---------------------------------------------------------------------------------------------------------
ANGLES = (0.0, 3e-6, 0.99e-5, 1.01e-5, 2e-5, 1e-4, 1e-3, 1e-2, 0.1, 1.0, 3.0, np.pi - 1e-2, np.pi - 1e-4, np.pi - 1e-6)
HUBER_DELTA = 1.5       # delta^2 = 2.25 is exact and has neighbours 2^-51 away


def _unit(rng, n, k):
    v = rng.standard_normal((n, k))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _huber_translations():
    """|t|^2 one ulp below, at, and one ulp above delta^2 = 2.25 in fp64 (and far inside either branch in exact arithmetic)"""
    x_lo = 1.5 - 2.0 ** -52          # x^2 = 2.25 - 1.5 ulp + 2^-104 -> rounds to 2.25 - 1 ulp
    y_hi = np.sqrt(2.0 ** -51)       # 2.25 + fl(y^2) -> 2.25 + 1 ulp
    out = np.array([[x_lo, 0.0], [1.5, 0.0], [1.5, y_hi]])
    s = out[:, 0] * out[:, 0] + out[:, 1] * out[:, 1]
    assert s[0] == np.nextafter(2.25, 0.0) and s[1] == 2.25 and s[2] == np.nextafter(2.25, 3.0)
    return out


def se3_cases(seed=2024):
    """dict(k0, k1, meas (n, 7) fp64; angle (n,) the residual rotation angle aimed at; label list).  Edge e joins its own
    vertices 2e (k0, `from`) and 2e + 1 (k1, `to`).  Per angle of ANGLES six random axes, each in three forms: as it is,
    with the measurement's quaternion negated, with k0's quaternion negated (the composed scalar part is then negative:
    the mirror of so3_log); then un-normalised quaternions and the Huber threshold."""
    rng = np.random.default_rng(seed)
    k0s, k1s, ms, ang, lab = [], [], [], [], []

    def add(k0, k1, m, a, label):
        k0s.append(np.asarray(k0, dtype=np.float64)); k1s.append(np.asarray(k1, dtype=np.float64)); ms.append(np.asarray(m, dtype=np.float64))
        ang.append(a); lab.append(label)

    def edge(angle, axis):
        """k0, k1 random, meas = A^-1 D with D = (t_D, rotation by `angle` about `axis`), A = k1^-1 k0: all in long double"""
        k0 = np.concatenate([rng.uniform(-3, 3, 3), _unit(rng, 1, 4)[0]])
        k1 = np.concatenate([rng.uniform(-3, 3, 3), _unit(rng, 1, 4)[0]])
        tD = rng.uniform(-3, 3, 3)
        if angle == 0.0:
            k0[3:] = k1[3:]
            return k0, k1, np.concatenate([tD, [1.0, 0, 0, 0]])
        (t0, q0), (t1, q1) = se3_from_vec(k0), se3_from_vec(k1)
        tA, qA = _mul(*_inv(t1, q1), t0, q0)
        h = LD(angle) / 2
        qD = np.concatenate([[np.cos(h)], np.sin(h) * _ld(axis)])[None]
        qm = _qmul(_qconj(qA), qD)
        return k0, k1, np.concatenate([tD, qm[0].astype(np.float64)])

    for a in ANGLES:
        for i, axis in enumerate(_unit(rng, 6, 3)):
            k0, k1, m = edge(a, axis)
            add(k0, k1, m, a, f"angle {a:.17g} axis {i}")
            mn = m.copy(); mn[3:] = -mn[3:]
            add(k0, k1, mn, a, f"angle {a:.17g} axis {i} meas q negated")
            kn = k0.copy(); kn[3:] = -kn[3:]
            add(kn, k1, m, a, f"angle {a:.17g} axis {i} k0 q negated")
    for scale in (1 + 1e-9, 1 - 1e-9, 2.0):
        for which in range(3):
            a = (0.3, 1e-4, 2.0)[which]
            trip = list(edge(a, _unit(rng, 1, 3)[0]))
            trip[which] = trip[which].copy(); trip[which][3:] *= scale
            add(*trip, a, f"quaternion norm {scale!r} in {('k0', 'k1', 'meas')[which]}")
    ident = np.array([0.0, 0, 0, 1, 0, 0, 0])
    for (x, y), side in zip(_huber_translations(), ("below", "at", "above")):
        add(np.array([x, y, 0, 1.0, 0, 0, 0]), ident, ident, 0.0, f"huber |r|^2 one ulp {side} delta^2")
    return dict(k0=np.array(k0s), k1=np.array(k1s), meas=np.array(ms), angle=np.array(ang), label=lab)


def se2_cases(seed=2025):
    """The SE2 counterpart: residual theta at +-ANGLES, four translations each, theta across the +-pi wrap, the Huber
    threshold.  k1 sits near +-pi on some edges so that a step of the retraction test carries theta across."""
    rng = np.random.default_rng(seed)
    k0s, k1s, ms, ang, lab = [], [], [], [], []

    def add(k1, m, tau, label, target=None):
        """k0 = k1 * Exp(tau) * m^-1, so that (k1^-1 k0) m = Exp(tau), in long double"""
        K0 = _se2_mat(k1) @ _se2_mat(se2_plus(np.zeros(3), tau)) @ _se2_inv(_se2_mat(m))
        k0 = np.array([K0[0, 0, 2], K0[0, 1, 2], np.arctan2(K0[0, 1, 0], K0[0, 0, 0])], dtype=np.float64)
        k0s.append(k0); k1s.append(np.asarray(k1, dtype=np.float64)); ms.append(np.asarray(m, dtype=np.float64))
        ang.append(tau[2] if target is None else target); lab.append(label)

    for a in ANGLES:
        for sign in (1.0, -1.0):
            for i in range(4):
                near_pi = i == 3
                th1 = (np.pi - 0.01) * (1 if rng.random() < 0.5 else -1) if near_pi else rng.uniform(-3, 3)
                k1 = np.array([*rng.uniform(-3, 3, 2), th1])
                m = np.array([*rng.uniform(-3, 3, 2), rng.uniform(-3, 3)])
                tau = np.array([*rng.uniform(-3, 3, 2), sign * a])
                add(k1, m, tau, f"theta {sign * a:.17g} #{i}")
    for over in (0.01, 1e-6):            # the sum of angles passes +-pi: the residual comes back from the other side
        for sign in (1.0, -1.0):
            k1 = np.array([*rng.uniform(-3, 3, 2), 0.5]); m = np.array([*rng.uniform(-3, 3, 2), -0.25])
            tau = np.array([*rng.uniform(-3, 3, 2), sign * (np.pi + over)])
            add(k1, m, tau, f"theta wraps at {sign:+.0f}pi by {over:g}", target=-sign * (np.pi - over))
    z = np.zeros(3)
    for (x, y), side in zip(_huber_translations(), ("below", "at", "above")):
        k0s.append(np.array([x, y, 0.0])); k1s.append(z); ms.append(z); ang.append(0.0); lab.append(f"huber |r|^2 one ulp {side} delta^2")
    return dict(k0=np.array(k0s), k1=np.array(k1s), meas=np.array(ms), angle=np.array(ang), label=lab)


def graph_of(cases):
    """PoseGraphData of the disjoint pairs: vertex 2e = k0 (`from`), 2e + 1 = k1 (`to`)"""
    from apex_solver_amd.synthetic import PoseGraphData

    n = len(cases["angle"])
    poses = np.empty((2 * n, cases["k0"].shape[1]))
    poses[0::2] = cases["k0"]; poses[1::2] = cases["k1"]
    e = np.arange(n, dtype=np.uint32)
    return PoseGraphData(ids=np.arange(2 * n, dtype=np.int64), poses=poses, e_from=2 * e, e_to=2 * e + 1, meas=cases["meas"].copy())


FROM_SCALE = 2.0 ** -10   # column scaling of the fixed `from` vertices in the retraction graphs (see retraction_problem)


def retraction_problem(cases):
    """(problem, scaling) of the retraction tests: the disjoint pairs with every `from` vertex fully fixed.  A fixed DOF
    stays in the linear system (it is zeroed when the step is applied), so the damped solve would split an edge's residual
    between its two vertices; the Jacobi column scaling FROM_SCALE on the `from` columns (a power of two: scaling and
    unscaling are exact) leaves the step to the free vertex, whose rotation part is then of the size of the residual's."""
    from apex_solver_amd.pose_graph import PoseGraphProblem

    d = graph_of(cases)
    prob = PoseGraphProblem(d)
    prob.fix[0::2, :] = 1
    scal = np.ones(prob.total_dof)
    for v in range(0, d.n_v, 2):
        scal[prob.pose_col[v]:prob.pose_col[v] + prob.dof] = FROM_SCALE
    return prob, scal


RETRACT_LAMBDA = 1e-9


BA_ANGLES = (3e-6, 8e-6, 1e-4, 5e-4, 1e-2, 0.1, 0.4, 5e-6, 2e-4, 3e-2, 0.8)


def ba_band_problem():
    """12 cameras, 400 points at the generator's true parameters with the observations projected from them (no pixel noise:
    a noisy problem's first step turns every camera by 1e-3 at least), the rotation of camera c >= 1 turned by
    BA_ANGLES[c - 1] about a random axis: the first step turns each camera back by about that angle, so its rotation parts
    span the lower bands of the retraction tests (camera 0 is the gauge)."""
    import apex_solver_amd as pkg

    d = pkg.synthetic.make_problem(12, 400, 3, 8, config_id=77, outlier_frac=0.0)
    rng = np.random.default_rng(77)
    poses = d.truth_poses.copy()
    for cam, a in enumerate(BA_ANGLES, start=1):
        ax = _unit(rng, 1, 3)[0]
        qe = np.concatenate([[np.cos(a / 2)], np.sin(a / 2) * ax])
        poses[cam, 3:] = _qmul(_ld(poses[cam, 3:]), _ld(qe)).astype(np.float64)
    d.obs_uv = pkg.synthetic.project_bal(d.truth_poses[d.cam_idx], d.truth_intr[d.cam_idx], d.truth_points[d.pt_idx])
    d.poses, d.intr, d.points = poses, d.truth_intr.copy(), d.truth_points.copy()
    return d


BA_LAMBDA = 1e-3
