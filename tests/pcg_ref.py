"""The reference's conjugate-gradient loops restated plainly (CPU only), and the crafted systems the PCG tests run
(tests/test_pcg_ref_host.py, tests/test_gpu_pcg.py, tests/test_gpu_pcg_solver.py).

solve_with_pcg (explicit_schur.rs:639-756, as oracle/ba_oracle.c states it in ora_solve_pcg):
    pre_i = 1 / d_i where |d_i| > 1e-12, else 1;  x = 0, r = b, z = pre r, p = z, rz_old = r.z
    abs_tol = tol * max(|b|, 1)
    each iteration:  pAp = p.Ap;  |pAp| < 1e-30: break, NOT counted;  alpha = rz_old / pAp;  x += alpha p;  r -= alpha Ap
                     |r| < abs_tol: count, break;  z = pre r;  rz_new = r.z;  |rz_old| < 1e-30: count, break
                     beta = rz_new / rz_old;  p = z + beta p;  rz_old = rz_new
The matrix-free loop (implicit_schur.rs:577-679, ora_solve_implicit_pcg) is the same with a block-diagonal preconditioner
(the inverses of the diagonal blocks of S) and the first threshold at 1e-20.

Everything runs in the dtype asked for: np.longdouble is the reference, np.float64 the competitor of the referee rule
(tile_ref.referee).  The operator is a callable, so tile dictionaries of any size never become a dense matrix.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

import tile_ref as tr

NB = tr.NB
LD = tr.LD
CUT = 1e-12          # the preconditioner's cut-off on |d|
TINY = 1e-30         # the absolute thresholds on p.Ap and rz_old


@dataclass
class Trajectory:
    x: np.ndarray
    iters: int
    exit: str                                   # "cap", "pap", "residual", "rz_old"
    abs_tol: float
    rn: list = field(default_factory=list)      # |r_k| after iteration k's update (k = 1 ..)
    pap: list = field(default_factory=list)     # p.Ap of every iteration entered
    rz_old: list = field(default_factory=list)  # rz_old of every iteration entered
    xs: list = field(default_factory=list)      # x_k (on request)


def pcg_loop(matvec, precond, b, max_iter, tol, dtype=LD, keep_x=False, pap_tiny=TINY):
    """The loop above with the operator and the preconditioner as callables on vectors of `dtype`."""
    b = np.asarray(b, dtype=dtype)
    x = np.zeros_like(b)
    r = b.copy()
    z = precond(r)
    p = z.copy()
    rz_old = np.dot(r, z)
    abs_tol = dtype(tol) * max(np.sqrt(np.dot(r, r)), dtype(1))
    t = Trajectory(x=x, iters=0, exit="cap", abs_tol=float(abs_tol))
    it = 0
    while it < max_iter:
        ap = matvec(p)
        pap = np.dot(p, ap)
        t.pap.append(float(pap)); t.rz_old.append(float(rz_old))
        if abs(pap) < pap_tiny:
            t.exit = "pap"
            break
        alpha = rz_old / pap
        x = x + alpha * p
        r = r - alpha * ap
        rn = np.sqrt(np.dot(r, r))
        t.rn.append(float(rn))
        if keep_x:
            t.xs.append(x.copy())
        if rn < abs_tol:
            it += 1
            t.exit = "residual"
            break
        z = precond(r)
        rz_new = np.dot(r, z)
        if abs(rz_old) < TINY:
            it += 1
            t.exit = "rz_old"
            break
        beta = rz_new / rz_old
        p = z + beta * p
        rz_old = rz_new
        it += 1
    t.x, t.iters = x, it
    return t


def matvec_tiles(T, x, nt, dtype):
    """y = A x from the lower tiles of a symmetric A, in `dtype`."""
    if dtype is LD:
        return tr.matvec_ld(T, x, nt)
    y = np.zeros(nt * NB, dtype=dtype)
    for (I, J), t in T.items():
        y[I * NB:(I + 1) * NB] += t @ x[J * NB:(J + 1) * NB]
        if I != J:
            y[J * NB:(J + 1) * NB] += t.T @ x[I * NB:(I + 1) * NB]
    return y


def jacobi_weights(d, dtype=LD):
    d = np.asarray(d, dtype=dtype)
    w = np.ones_like(d)
    m = np.abs(d) > CUT
    w[m] = dtype(1) / d[m]
    return w


def tile_diag(T, nt):
    return np.concatenate([np.diag(T[(I, I)]) for I in range(nt)])


def pcg_tiles(T, nt, b, max_iter, tol, dtype=LD, keep_x=False):
    """Jacobi-PCG on a tile dictionary."""
    w = jacobi_weights(tile_diag(T, nt), dtype)
    return pcg_loop(lambda v: matvec_tiles(T, v, nt, dtype), lambda v: w * v, b, max_iter, tol, dtype, keep_x)


def pcg_dense(S, b, max_iter, tol, dtype=LD, keep_x=False):
    """Jacobi-PCG on a dense symmetric matrix."""
    Sd = np.asarray(S, dtype=dtype)
    w = jacobi_weights(np.diag(Sd), dtype)
    return pcg_loop(lambda v: Sd @ v, lambda v: w * v, b, max_iter, tol, dtype, keep_x)


def inverse_gj(a):
    """Gauss-Jordan with partial pivoting in a's dtype (the small diagonal blocks of the block preconditioner)."""
    a = np.array(a)
    n = a.shape[0]
    m = np.concatenate([a, np.eye(n, dtype=a.dtype)], axis=1)
    for c in range(n):
        piv = c + int(np.argmax(np.abs(m[c:, c])))
        if m[piv, c] == 0:
            raise np.linalg.LinAlgError("singular block")
        m[[c, piv]] = m[[piv, c]]
        m[c] = m[c] / m[c, c]
        for rr in range(n):
            if rr != c:
                m[rr] = m[rr] - m[rr, c] * m[c]
    return m[:, n:]


def pcg_dense_blocks(S, b, blocks, max_iter, tol, dtype=LD, keep_x=False):
    """The matrix-free loop's arithmetic on a dense S: block-diagonal preconditioner from S's own diagonal blocks, given as
    (start, size) pairs that tile the rows (6 per camera pose, 3 per camera's intrinsics), first threshold 1e-20
    (implicit_schur.rs:610-613)."""
    Sd = np.asarray(S, dtype=dtype)
    assert sorted(i for s0, n in blocks for i in range(s0, s0 + n)) == list(range(Sd.shape[0]))
    inv = [(s0, n, inverse_gj(Sd[s0:s0 + n, s0:s0 + n])) for s0, n in blocks]

    def precond(v):
        out = np.empty_like(v)
        for s, n, m in inv:
            out[s:s + n] = m @ v[s:s + n]
        return out
    return pcg_loop(lambda v: Sd @ v, precond, b, max_iter, tol, dtype, keep_x, pap_tiny=1e-20)


# ---------------------------------------------------------------------------------------------------------------------
# the crafted systems


@dataclass
class Case:
    label: str
    pat: np.ndarray
    A: dict                      # tiles, full n_pad (rows / columns from n_valid on are zero: the device sets their diagonal to 1)
    b: np.ndarray                # n_pad (zero from n_valid on)
    tol: float = 1e-13
    n_valid: int | None = None
    fill_mode: int = 0
    kappa_bound: float | None = None   # for n > 576: a bound on kappa_J by construction
    expect_iters: int | None = None    # the count the construction promises (finite termination, the threshold exits)
    expect_exit: str | None = None

    @property
    def nt(self):
        return self.pat.shape[0]

    @property
    def n_pad(self):
        return self.nt * NB

    @property
    def n(self):
        return self.n_pad if self.n_valid is None else self.n_valid

    @property
    def small(self):
        return self.n_pad <= 576

    def dense(self):
        return tr.dense_of(self.A, self.nt)[:self.n, :self.n]

    def run(self, max_iter, dtype=LD, keep_x=False, tol=None):
        """The restatement on the n_valid x n_valid system (dense where a part of the last tile is padding)."""
        tol = self.tol if tol is None else tol
        if self.n_valid is None:
            return pcg_tiles(self.A, self.nt, self.b, max_iter, tol, dtype, keep_x)
        return pcg_dense(self.dense(), self.b[:self.n], max_iter, tol, dtype, keep_x)

    def kappa_j(self):
        """Condition number of the matrix as the reference preconditions it (numpy), or the bound of the construction."""
        if not self.small:
            assert self.kappa_bound is not None
            return self.kappa_bound
        S = self.dense()
        w = np.sqrt(jacobi_weights(np.diag(S), np.float64))
        return float(np.linalg.cond(S * w[:, None] * w[None, :]))

    def floor(self):
        return 8 * self.n * tr.U * max(1.0, self.kappa_j())


def tol_between(case, k):
    """The tolerance that puts abs_tol at the geometric mean of the long double reference's |r_{k-1}| and |r_k|: the
    reference stops after exactly k iterations with the same margin on either side."""
    t = case.run(k, LD, tol=0.0)
    assert t.iters == k and t.exit == "cap", (case.label, t.iters, t.exit)
    bn = float(np.sqrt(np.dot(np.asarray(case.b, dtype=LD), np.asarray(case.b, dtype=LD))))
    return float(np.sqrt(t.rn[k - 2] * t.rn[k - 1])) / max(bn, 1.0)


K_CONV = 10          # the dominant cases converge by a factor of about 0.045 per iteration: ten iterations to 1e-13
DOMINANT_KAPPA = 9.0   # Gershgorin: the diagonal dominates its row by 1.25, so the Jacobi-scaled spectrum lies in [0.2, 1.8]


def dominant(label, pat, seed, fill_mode=0):
    rng = np.random.default_rng(seed)
    A = tr.dominant_case(pat, rng)
    n = pat.shape[0] * NB
    c = Case(label, pat, A, rng.standard_normal(n), fill_mode=fill_mode, kappa_bound=DOMINANT_KAPPA)
    c.tol = tol_between(c, K_CONV)
    c.expect_iters = K_CONV
    c.expect_exit = "residual"
    return c


ITERATE = {"band6": (lambda: tr.band(6), 11, 0), "arrow5": (lambda: tr.arrow(5), 12, 0), "dense3": (lambda: tr.dense(3), 13, 0),
           "nd2_nanfill": (lambda: tr.nested_dissection(2), 14, 1)}       # every iterate, the bits behind the speculation
# Shapes: one tile; two tiles (two 256-blocks, the second partial); more tile rows and more 256-blocks than one trip of the strided
# reductions takes.  (One tile of the dominant construction converges by 0.075 per iteration: no tolerance leaves a factor of 4
# on both sides of a stopping residual, so the single tile gets the finite-termination construction and its count r + 1 = 4.)
SHAPES = ("lowrank_r3_nt1", "nt2", "band460")


def low_rank(r, seed=31, nt=3):
    rng = np.random.default_rng(seed + r)
    A, _, _ = tr.low_rank_case(nt, r, rng)
    return Case(f"lowrank_r{r}" + ("" if nt == 3 else f"_nt{nt}"), tr.dense(nt), A, rng.standard_normal(nt * NB), tol=1e-12, expect_iters=r + 1, expect_exit="residual")


def diagonal_case(nt=3, seed=41):
    """A diagonal matrix on which every operation of the first iteration is exact: d_i = 2^e, e in [-4, 4], b_i integers in
    [-64, 64].  pre = 1/d, p = b/d, d p = b and the terms b^2/d of r.z and p.Ap (multiples of 2^-4 below 2^16) are exact, and so
    are their sums in any order: alpha = 1, x = b/d and r = 0 exactly -- in fp64 as in long double."""
    rng = np.random.default_rng(seed)
    n = nt * NB
    d = np.ldexp(1.0, rng.integers(-4, 5, size=n))
    A = {(I, I): np.diag(d[I * NB:(I + 1) * NB]) for I in range(nt)}
    b = rng.integers(-64, 65, size=n).astype(np.float64)
    return Case("diagonal", tr.block_diagonal(nt), A, b, tol=1e-12, expect_iters=1, expect_exit="residual")


def threshold_base():
    """The dominant system the absolute thresholds are reached on (small, so the oracle runs it too)."""
    return dominant("dense3_thresholds", tr.dense(3), 51)


def scaled_rhs(base, exp2, tol, label, expect_iters, expect_exit):
    return Case(f"{base.label}_{label}", base.pat, base.A, np.ldexp(base.b, exp2), tol=tol, kappa_bound=base.kappa_bound,
                expect_iters=expect_iters, expect_exit=expect_exit)


def threshold_cases():
    base = threshold_base()
    zero = scaled_rhs(base, 0, 1e-13, "zero_rhs", 0, "pap")
    zero.b = np.zeros_like(base.b)
    return [zero,
            scaled_rhs(base, -60, 1e-13, "pap_exit", 0, "pap"),
            scaled_rhs(base, -46, 1e-6, "tiny_rhs_residual_exit", 1, "residual")]


def rz_old_case(nt=3, seed=61):
    """The rz_old exit: A = S (I + u u^T) S with u in {+-1/2}^n and b = c S u, so that p0 = pre b is the top eigenvector of
    the Jacobi-scaled operator: p.Ap / rz_old = (1 + n/4) / 1.25 (87.2 at n = 432).  c puts rz_old at 2^-103 = 9.86e-32 (10.1 x
    below 1e-30), which leaves p.Ap at 8.6e-30 (8.6 x above): both at least 8 x from the threshold, on the intended sides.
    tol = 0 keeps the residual test out of it."""
    rng = np.random.default_rng(seed)
    A, Um, e = tr.low_rank_case(nt, 1, rng, u=0.5)
    su = np.ldexp(Um[:, 0], e)                       # S u, exact
    # rz_old = b.(pre b) = c^2 sum_i (s_i u_i)^2 / (1.25 s_i^2) = c^2 n / 5; n / 5 = 86.4, c^2 = 2^-103 / 86.4 (c rounded once)
    n = nt * NB
    c = float(np.sqrt(np.ldexp(1.0, -103) / (n / 5.0)))
    return Case("rz_old_exit", tr.dense(nt), A, c * su, tol=0.0, expect_iters=1, expect_exit="rz_old")


def cutoff_case(nt=3, r=3, seed=71):
    """The preconditioner cut-off: a third of the rows carries S = 2^-25, so their diagonal (1 + r/64) 2^-50 = 9.3e-16 lies below the 1e-12 cut-off and
    the reference preconditions them with 1, not 1/d."""
    rng = np.random.default_rng(seed)
    n = nt * NB
    e = rng.integers(-6, 7, size=n)
    e[rng.permutation(n)[:n // 3]] = -25
    A, _, _ = tr.low_rank_case(nt, r, rng, row_exp=e)
    return Case("cutoff_rows", tr.dense(nt), A, rng.standard_normal(n), tol=1e-13)


def padded_case(nt=3, n_valid=400, seed=81):
    """A partial last tile.  Rows and columns from n_valid on are zero in the tiles handed over (a solver's assembly never
    writes them); the device sets their diagonal to 1, their right-hand side is 0."""
    rng = np.random.default_rng(seed)
    pat = tr.dense(nt)
    A = tr.dominant_case(pat, rng)
    n = nt * NB
    keep = (np.arange(n) < n_valid).astype(np.float64)
    A = {(I, J): t * keep[I * NB:(I + 1) * NB, None] * keep[None, J * NB:(J + 1) * NB] for (I, J), t in A.items()}
    b = rng.standard_normal(n) * keep
    c = Case("padded_400_of_432", pat, A, b, n_valid=n_valid, kappa_bound=DOMINANT_KAPPA)
    c.tol = tol_between(c, K_CONV)
    c.expect_iters, c.expect_exit = K_CONV, "residual"
    return c


THRESHOLDS = ("zero_rhs", "pap_exit", "tiny_rhs_residual_exit")
LABELS = (tuple(ITERATE) + SHAPES + ("lowrank_r1", "lowrank_r3", "lowrank_r7", "diagonal") + tuple(f"dense3_thresholds_{k}" for k in THRESHOLDS)
          + ("rz_old_exit", "cutoff_rows", "padded_400_of_432"))
SMALL_LABELS = tuple(k for k in LABELS if k not in ("band6", "arrow5", "nd2_nanfill", "band460"))   # n <= 576


@functools.lru_cache(maxsize=None)
def case(label):
    """The crafted system of that name (built once per process)."""
    if label in ITERATE:
        pat, seed, fill = ITERATE[label]
        c = dominant(label, pat(), seed, fill)
    elif label == "lowrank_r3_nt1":
        c = low_rank(3, seed=20, nt=1)
    elif label == "nt2":
        c = dominant("nt2", tr.dense(2), 22)
    elif label == "band460":
        c = dominant("band460", tr.band(460), 23)
    elif label.startswith("lowrank_r"):
        c = low_rank(int(label[9:]))
    elif label.startswith("dense3_thresholds_"):
        c = threshold_cases()[THRESHOLDS.index(label[len("dense3_thresholds_"):])]
    else:
        c = {"diagonal": diagonal_case, "rz_old_exit": rz_old_case, "cutoff_rows": cutoff_case, "padded_400_of_432": padded_case}[label]()
    assert c.label == label, (c.label, label)
    return c
