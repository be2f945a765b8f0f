"""Reference arithmetic for the tile Cholesky tests (CPU only; tests/test_tile_ref_host.py, tests/test_gpu_tile_cholesky.py).

A matrix on a tile pattern is a dict {(I, J): 144 x 144 array} over I >= J; a diagonal tile of A holds the full symmetric
block, a diagonal tile of L its lower triangle.  Everything is computed tile by tile, so patterns of many tile columns never
need a dense n x n product in long double.

Exact factors by construction.  L0 is drawn on a pattern without fill with every entry a multiple of 2^-q (an int64 matrix
M times 2^-q).  A 2^(2q) = M M^T is then an integer product, exact in int64; as long as every entry of it stays below 2^53
(checked) A is exact in fp64 and its Cholesky factor (positive diagonal) is exactly L0.  Multiplying the rows by powers of
two, D = diag(2^e), keeps all of this exact: D A D has the factor D L0.

Bounds (u = 2^-53, gamma_m = m u / (1 - m u)), elementwise on every tile of the filled pattern:
  factor   |A - L^ L^T| <= 2 gamma_m |L^| |L^T|       m = the inner-product length of the tile (144 x shared tile columns)
           + 4 gamma_144 |W| |X^T| |L^_JJ^T| for the tiles (and 16 x 16 blocks) that the device solves by a product with the
           computed inverse X (factor_ratio)
  solve    |b - A x^| <= 2 gamma_{3n+1} |L^| |L^T| |x^|
  Linv     |L^_JJ X^ - I| <= 2 gamma_144 |L^_JJ| |X^|
           (k_potrf_inv_mf builds X row block by row block from X_rj = -X_rr sum_{k=j}^{r-1} L_rk X_kj, and inside a 16 x 16
           block row j+1 of X from row j: both are forward substitution for L X = I, whose computed columns satisfy
           (L + dL_j) x_j = e_j with |dL_j| <= gamma_n |L| (Higham, Thm 8.5), i.e. the RIGHT residual |L X^ - I| <= gamma_n |L||X^|.)
  matvec   |y - A x| <= gamma_n |A| |x|
The residuals are formed in long double (or from the exact L0, where the error E = L^ - L0 makes A - L^ L^T = E L0^T + L^ E^T
computable in fp64 to far below the bound).  The factor 2 on each bound covers the pairwise / fma order of the device's sums.
"""
from __future__ import annotations

import numpy as np

NB = 144
U = 2.0 ** -53
LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, "the long double references need an 80-bit (or wider) long double"


def gamma(m):
    return m * U / (1.0 - m * U)


# ---------------------------------------------------------------------------------------------------------------------
# patterns


def pattern_from_edges(nt, edges):
    """Lower-triangular 0/1 tile structure with the diagonal and the given (I, J) / (J, I) pairs."""
    p = np.eye(nt, dtype=np.uint8)
    for a, b in edges:
        p[max(a, b), min(a, b)] = 1
    return p


def band(nt, bw=1):
    return pattern_from_edges(nt, [(i, j) for i in range(nt) for j in range(max(0, i - bw), i)])


def dense(nt):
    return pattern_from_edges(nt, [(i, j) for i in range(nt) for j in range(i)])


def arrow(n_leaves):
    """n_leaves independent tiles and one border tile (last) coupled to all of them."""
    return pattern_from_edges(n_leaves + 1, [(n_leaves, j) for j in range(n_leaves)])


def block_diagonal(nt):
    return np.eye(nt, dtype=np.uint8)


def grid(r, c):
    """4-neighbour grid graph of r x c tiles in row-major order (fills in)."""
    e = []
    for i in range(r):
        for j in range(c):
            k = i * c + j
            if j + 1 < c:
                e.append((k, k + 1))
            if i + 1 < r:
                e.append((k, k + c))
    return pattern_from_edges(r * c, e)


def star_of_chains(n_chains, length):
    """Chains of `length` tiles whose last tiles all couple to one hub (last), eliminated chain by chain (fills in)."""
    nt = n_chains * length + 1
    e = []
    for c in range(n_chains):
        for k in range(length - 1):
            e.append((c * length + k, c * length + k + 1))
        e.append((c * length, nt - 1))   # the chain's FIRST tile couples to the hub: fill along the whole chain
    return pattern_from_edges(nt, e)


def nested_dissection(levels=2):
    """Two halves with a separator, recursively; every leaf couples to both separators above it (fills in between)."""
    def build(lo, depth):
        if depth == 0:
            return [lo], [], lo + 1
        a, ea, nxt = build(lo, depth - 1)
        b, eb, nxt = build(nxt, depth - 1)
        sep = nxt
        e = ea + eb + [(a[0], sep), (b[-1], sep)]
        return a + b + [sep], e, sep + 1
    cols, e, nt = build(0, levels)
    return pattern_from_edges(nt, e)


def symbolic_cols(present):
    """Tile-level symbolic fill: cols[K] = sorted rows I > K of column K of L."""
    nt = present.shape[0]
    rows = [set(np.nonzero(present[K + 1:, K])[0] + K + 1) for K in range(nt)]
    for K in range(nt):
        if rows[K]:
            p = min(rows[K])
            rows[p] |= rows[K] - {p}
    return [sorted(r) for r in rows]


def filled_pattern(present):
    cols = symbolic_cols(present)
    return [(K, K) for K in range(present.shape[0])] + [(I, K) for K in range(present.shape[0]) for I in cols[K]]


def has_fill(present):
    return any(not present[I, J] for I, J in filled_pattern(present))


# ---------------------------------------------------------------------------------------------------------------------
# matrices


def exact_factor(present, rng, q=14, diag_exp=(0, 0), off_ratio=4.0, pivots=None):
    """(M, q): int64 tiles of L0 = M 2^-q on `present` (must not fill in).  Diagonal entries about 2^e, e drawn from diag_exp
    (inclusive); off-diagonal entries random integers with |row sum| about off_ratio of the diagonal of the first
    exponent; pivots = {row: exponent} overrides single diagonal entries (global row numbers)."""
    assert not has_fill(present)
    nt = present.shape[0]
    nnz_row = [NB * (1 + int(present[I, :I].sum())) for I in range(nt)]
    M = {}
    for I in range(nt):
        amp = max(1, int(off_ratio * 2.0 ** (q + diag_exp[0]) * 2 / nnz_row[I]))
        for J in range(I + 1):
            if not present[I, J]:
                continue
            t = rng.integers(-amp, amp + 1, size=(NB, NB), dtype=np.int64)
            if I == J:
                t = np.tril(t, -1)
                e = rng.integers(diag_exp[0], diag_exp[1] + 1, size=NB)
                for r in range(NB):
                    g = I * NB + r
                    if pivots and g in pivots:
                        e[r] = pivots[g]
                assert e.min() >= -q
                # 2^e (1 + k/8), k in {1, 3, 5} where there are bits for it: the pivots are then not powers of four, and
                # 1/sqrt of them is not exact (a missing Newton step after the approximate rsq shows)
                k = rng.choice([1, 3, 5], size=NB)
                frac = np.where(e + q >= 3, np.left_shift(k, np.maximum(e + q - 3, 0)), 0)
                t[np.arange(NB), np.arange(NB)] = (2 ** (e + q)).astype(np.int64) + frac
            M[(I, J)] = t
    return M, q


def product_int(M, present):
    """A 2^(2q) = M M^T, tile by tile in int64 (exact: asserted below 2^53 per entry)."""
    nt = present.shape[0]
    A = {}
    for I in range(nt):
        for J in range(I + 1):
            if not present[I, J]:
                continue
            acc = np.zeros((NB, NB), dtype=np.int64)
            for K in range(J + 1):
                if present[I, K] and present[J, K]:
                    acc += M[(I, K)] @ M[(J, K)].T
            assert np.abs(acc).max() < 2 ** 53, "the exact construction left fp64's integer range"
            A[(I, J)] = acc
    return A


def to_float(Mi, q):
    """tiles of M 2^-q (exact)."""
    return {k: v.astype(np.float64) * 2.0 ** -q for k, v in Mi.items()}


def scale_rows(T, row_exp, cols=True):
    """D T (cols False) or D T D (cols True), D = diag(2^row_exp): exact for power-of-two scales."""
    out = {}
    for (I, J), t in T.items():
        ri = np.ldexp(1.0, row_exp[I * NB:(I + 1) * NB])[:, None]
        s = t * ri
        if cols:
            s = s * np.ldexp(1.0, row_exp[J * NB:(J + 1) * NB])[None, :]
        out[(I, J)] = s
    return out


def exact_case(present, rng, **kw):
    """(A, L0) in fp64, both exact: A = L0 L0^T."""
    M, q = exact_factor(present, rng, **kw)
    Ai = product_int(M, present)
    A = {k: v.astype(np.float64) * 2.0 ** (-2 * q) for k, v in Ai.items()}
    L0 = to_float(M, q)
    return A, L0


def dominant_case(present, rng, q=14, amp=64):
    """SPD by diagonal dominance with dyadic entries (for patterns that fill in: no exact factor)."""
    nt = present.shape[0]
    A = {}
    rowsum = np.zeros(nt * NB)
    for I in range(nt):
        for J in range(I):
            if present[I, J]:
                t = rng.integers(-amp, amp + 1, size=(NB, NB)).astype(np.float64) * 2.0 ** -q
                A[(I, J)] = t
                rowsum[I * NB:(I + 1) * NB] += np.abs(t).sum(1)
                rowsum[J * NB:(J + 1) * NB] += np.abs(t).sum(0)
    for I in range(nt):
        t = rng.integers(-amp, amp + 1, size=(NB, NB)).astype(np.float64) * 2.0 ** -q
        t = np.tril(t, -1)
        t = t + t.T
        d = rowsum[I * NB:(I + 1) * NB] + np.abs(t).sum(1)
        t[np.arange(NB), np.arange(NB)] = np.ceil(d * 2.0 ** q * 1.25 + 1) * 2.0 ** -q
        A[(I, I)] = t
    return A


def low_rank_case(nt, r, rng, u=0.125, exp_range=(-6, 6), row_exp=None):
    """(A, U, e): A = S (I + U U^T) S on dense(nt), U in {+-u}^(n x r), S = diag(2^e) with e drawn from exp_range (inclusive)
    or given as row_exp.  Every row of U has the norm u sqrt(r), so I + U U^T has the constant diagonal 1 + r u^2 and the
    Jacobi-scaled matrix is (I + U U^T) / (1 + r u^2): r + 1 distinct eigenvalues, so CG with the Jacobi preconditioner ends
    after r + 1 iterations in exact arithmetic.  u a power of two: every entry is dyadic and exact in fp64."""
    n = nt * NB
    Um = rng.choice([-1.0, 1.0], size=(n, r)) * u
    e = rng.integers(exp_range[0], exp_range[1] + 1, size=n) if row_exp is None else np.asarray(row_exp, dtype=np.int64)
    assert e.shape == (n,)
    A = {}
    for I in range(nt):
        for J in range(I + 1):
            t = Um[I * NB:(I + 1) * NB] @ Um[J * NB:(J + 1) * NB].T   # (sums of r terms +-u^2: exact)
            if I == J:
                t = t + np.eye(NB)
            A[(I, J)] = t
    return scale_rows(A, e), Um, e


def touched_array(A, dev):
    """The tiles of A in the plan's slot order (the first n_touched slots)."""
    out = np.zeros((dev.n_touched, NB, NB))
    for (I, J), t in A.items():
        s = dev.slot[I, J]
        assert 0 <= s < dev.n_touched, (I, J, s)
        out[s] = t
    return out


def from_slots(arr, dev, keys):
    return {k: arr[dev.slot[k]] for k in keys}


def dense_of(T, nt, sym=True):
    n = nt * NB
    D = np.zeros((n, n), dtype=next(iter(T.values())).dtype)
    for (I, J), t in T.items():
        D[I * NB:(I + 1) * NB, J * NB:(J + 1) * NB] = t
        if sym and I != J:
            D[J * NB:(J + 1) * NB, I * NB:(I + 1) * NB] = t.T
    return D


# ---------------------------------------------------------------------------------------------------------------------
# long double kernels (any size)


def chol_ld(a):
    """Cholesky of a symmetric block in long double (right-looking, row by row)."""
    a = np.array(a, dtype=LD)
    n = a.shape[0]
    L = np.zeros_like(a)
    for j in range(n):
        d = a[j, j] - np.dot(L[j, :j], L[j, :j])
        if not d > 0:
            raise np.linalg.LinAlgError(f"pivot {j} not positive")
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (a[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def tri_inv_ld(L):
    """Inverse of a lower-triangular block in long double (2 x 2 block recursion)."""
    L = np.asarray(L, dtype=LD)
    n = L.shape[0]
    if n <= 16:
        X = np.zeros_like(L)
        for j in range(n):
            X[j, :j + 1] = -(L[j, :j] @ X[:j, :j + 1])
            X[j, j] += 1
            X[j, :j + 1] /= L[j, j]
        return X
    h = n // 2
    Ai = tri_inv_ld(L[:h, :h])
    Ci = tri_inv_ld(L[h:, h:])
    X = np.zeros_like(L)
    X[:h, :h] = Ai
    X[h:, h:] = Ci
    X[h:, :h] = -(Ci @ (L[h:, :h] @ Ai))
    return X


def tile_cholesky(A, present, ld=True):
    """Right-looking tile Cholesky on the filled pattern: in long double (reference) or with numpy / scipy fp64 (the
    referee's e_np).  Returns (L, Linv) tile dicts."""
    from scipy.linalg import solve_triangular

    cols = symbolic_cols(present)
    nt = present.shape[0]
    dt = LD if ld else np.float64
    W = {k: np.array(v, dtype=dt) for k, v in A.items()}
    for I, J in filled_pattern(present):
        W.setdefault((I, J), np.zeros((NB, NB), dtype=dt))
    L, Li = {}, {}
    for K in range(nt):
        L[(K, K)] = chol_ld(W[(K, K)]) if ld else np.linalg.cholesky(W[(K, K)])
        Li[K] = tri_inv_ld(L[(K, K)]) if ld else solve_triangular(L[(K, K)], np.eye(NB), lower=True)
        for I in cols[K]:
            L[(I, K)] = W[(I, K)] @ Li[K].T if ld else solve_triangular(L[(K, K)], W[(I, K)].T, lower=True).T
        for a, I in enumerate(cols[K]):
            for J in cols[K][:a + 1]:
                W[(I, J)] = W[(I, J)] - L[(I, K)] @ L[(J, K)].T
    return L, Li


def selected_inverse(L, Li, present, dtype=LD, cols_wanted=None):
    """Z = (L L^T)^-1 on the filled pattern by the block Takahashi recurrence (root first) in `dtype`.  cols_wanted: only
    these tile columns (and what they need: their ancestors)."""
    cols = symbolic_cols(present)
    nt = present.shape[0]
    need = set(range(nt)) if cols_wanted is None else set()
    for j in (cols_wanted or []):
        k = j
        while True:
            need.add(k)
            if not cols[k]:
                break
            k = cols[k][0]
    Z = {}
    Lt = {k: np.asarray(v, dtype=dtype) for k, v in L.items()}
    for j in reversed(range(nt)):
        if j not in need:
            continue
        X = np.asarray(Li[j], dtype=dtype)
        Y = {r: Lt[(r, j)] @ X for r in cols[j]}

        def zt(r, s):
            return Z[(r, s)] if r >= s else Z[(s, r)].T
        for r in cols[j]:
            acc = np.zeros((NB, NB), dtype=dtype)
            for s in cols[j]:
                acc -= zt(r, s) @ Y[s]
            Z[(r, j)] = acc
        acc = X.T @ X
        for r in cols[j]:
            acc -= Y[r].T @ Z[(r, j)]
        Z[(j, j)] = acc
    return Z


# ---------------------------------------------------------------------------------------------------------------------
# bounds: each returns the worst ratio measured / bound (<= 1: holds)


def _ratio(res, bnd):
    res = np.abs(np.asarray(res, dtype=np.float64))
    bnd = np.asarray(bnd, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bnd > 0, res / bnd, np.where(res > 0, np.inf, 0.0))
    return float(np.nan_to_num(r, nan=np.inf).max())


def factor_ratio(A, Lh, present, L0=None, keys=None, X=None):
    """max over the filled pattern (or `keys`) of |A - L^ L^T| / bound, lower triangle of diagonal tiles, with
    bound = 2 gamma_m |L^||L^T| (Higham Thm 10.3: the substitution form).  L0 (exact factor): the residual as
    E L0^T + L^ E^T in fp64; else in long double.

    X (the device's diagonal inverses, tile column -> 144 x 144): the device's panel solves are products with the inverse,
    L_IJ = fl(W_IJ X_JJ^T) with W_IJ the updated tile (and inside a diagonal tile, its 16 x 16 blocks below the diagonal
    likewise with the 16 x 16 diagonal blocks of X).  A product with a computed inverse is not a substitution: with
    |L X - I| <= gamma |L||X| (linv_ratio) and |fl(W X^T) - W X^T| <= gamma_144 |W||X^T|,
        W - L^ L_JJ^T = W (I - X^T L_JJ^T) - dW L_JJ^T   =>   |W - L^ L_JJ^T| <= 4 gamma_144 |W| |X^T| |L_JJ^T|,
    which the bound then adds, with |W| <= |A_IJ| + sum_K |L^_IK||L^_JK^T|.  Without X only the substitution bound is used."""
    cols = symbolic_cols(present)
    nt = present.shape[0]
    rows_of = [set() for _ in range(nt)]   # rows_of[I] = tile columns K with a tile (I, K)
    for K in range(nt):
        rows_of[K].add(K)
        for I in cols[K]:
            rows_of[I].add(K)
    worst = 0.0
    low = np.tril(np.ones((NB, NB), dtype=bool))
    for I, J in (keys or filled_pattern(present)):
        shared = sorted(rows_of[I] & rows_of[J])
        shared = [K for K in shared if K <= J]
        bnd = np.zeros((NB, NB))
        if L0 is not None:
            res = np.zeros((NB, NB))
            for K in shared:
                Ei, Ej = Lh[(I, K)] - L0[(I, K)], Lh[(J, K)] - L0[(J, K)]
                res += Ei @ L0[(J, K)].T + Lh[(I, K)] @ Ej.T
                bnd += np.abs(Lh[(I, K)]) @ np.abs(Lh[(J, K)]).T
        else:
            res = np.array(A.get((I, J), np.zeros((NB, NB))), dtype=LD)
            for K in shared:
                res -= np.asarray(Lh[(I, K)], dtype=LD) @ np.asarray(Lh[(J, K)], dtype=LD).T
                bnd += np.abs(Lh[(I, K)]) @ np.abs(Lh[(J, K)]).T
        bnd *= 2 * gamma(NB * len(shared)) * (1 + 1e-12)
        if X is not None:
            W = np.abs(A.get((I, J), np.zeros((NB, NB)))) + sum(np.abs(Lh[(I, K)]) @ np.abs(Lh[(J, K)]).T for K in shared)
            if I != J:
                extra = W @ (np.abs(X[J]).T @ np.abs(Lh[(J, J)]).T)
            else:   # the 16 x 16 blocks below the diagonal, each from its block row of W and the diagonal blocks of X, L
                extra = np.zeros((NB, NB))
                for c in range(0, NB, 16):
                    B = np.abs(X[J][c:c + 16, c:c + 16]).T @ np.abs(Lh[(J, J)][c:c + 16, c:c + 16]).T
                    extra[c + 16:, c:c + 16] = W[c + 16:, c:c + 16] @ B
            bnd += 4 * gamma(NB) * extra * (1 + 1e-12)
        if I == J:
            res, bnd = np.where(low, res, 0), np.where(low, bnd, 0)
        worst = max(worst, _ratio(res, bnd))
    return worst


def linv_ratio(Ljj, X):
    """|L^_JJ X^ - I| / (2 gamma_144 |L^_JJ||X^|) (the right residual: see the module docstring)."""
    R = np.asarray(Ljj, dtype=LD) @ np.asarray(X, dtype=LD) - np.eye(NB, dtype=LD)
    return _ratio(R, 2 * gamma(NB) * (np.abs(Ljj) @ np.abs(X)) * (1 + 1e-12))


def matvec_ld(T, x, nt):
    """y = A x in long double from the lower tiles of a symmetric A."""
    xl = np.asarray(x, dtype=LD)
    y = np.zeros(nt * NB, dtype=LD)
    for (I, J), t in T.items():
        tl = np.asarray(t, dtype=LD)
        y[I * NB:(I + 1) * NB] += tl @ xl[J * NB:(J + 1) * NB]
        if I != J:
            y[J * NB:(J + 1) * NB] += tl.T @ xl[I * NB:(I + 1) * NB]
    return y


def abs_matvec(T, x, nt, sym=True, trans=False):
    """|T| |x| (fp64; the bounds' own rounding is far below their slack)."""
    y = np.zeros(nt * NB)
    ax = np.abs(x)
    for (I, J), t in T.items():
        a = np.abs(t)
        if trans:
            y[J * NB:(J + 1) * NB] += a.T @ ax[I * NB:(I + 1) * NB]
        else:
            y[I * NB:(I + 1) * NB] += a @ ax[J * NB:(J + 1) * NB]
            if sym and I != J:
                y[J * NB:(J + 1) * NB] += a.T @ ax[I * NB:(I + 1) * NB]
    return y


def solve_ratio(A, Lh, x, b, nt):
    """|b - A x^| / (2 gamma_{3n+1} |L^||L^T||x^|), elementwise."""
    r = np.asarray(b, dtype=LD) - matvec_ld(A, x, nt)
    w = abs_matvec(Lh, abs_matvec(Lh, x, nt, sym=False, trans=True), nt, sym=False)
    return _ratio(r, 2 * gamma(3 * nt * NB + 1) * w * (1 + 1e-12))


def matvec_ratio(A, x, y, nt):
    r = np.asarray(y, dtype=LD) - matvec_ld(A, x, nt)
    return _ratio(r, gamma(nt * NB) * abs_matvec(A, x, nt) * (1 + 1e-12))


def refined_solve(A, L, Li, b, present):
    """x of A x = b: a long double tile solve with L (exact or long double), one refinement step (residual in long double)."""
    nt = present.shape[0]
    cols = symbolic_cols(present)

    def sweep(rhs):
        y = np.array(rhs, dtype=LD)
        for K in range(nt):
            y[K * NB:(K + 1) * NB] = np.asarray(Li[K], dtype=LD) @ y[K * NB:(K + 1) * NB]
            for I in cols[K]:
                y[I * NB:(I + 1) * NB] -= np.asarray(L[(I, K)], dtype=LD) @ y[K * NB:(K + 1) * NB]
        for K in reversed(range(nt)):
            for I in cols[K]:
                y[K * NB:(K + 1) * NB] -= np.asarray(L[(I, K)], dtype=LD).T @ y[I * NB:(I + 1) * NB]
            y[K * NB:(K + 1) * NB] = np.asarray(Li[K], dtype=LD).T @ y[K * NB:(K + 1) * NB]
        return y
    x = sweep(b)
    return x + sweep(np.asarray(b, dtype=LD) - matvec_ld(A, x, nt))


def np_solve(Lnp, Linp, b, present):
    """The fp64 tile solve with numpy's factor (the referee's e_np for x)."""
    nt = present.shape[0]
    cols = symbolic_cols(present)
    y = np.array(b, dtype=np.float64)
    for K in range(nt):
        y[K * NB:(K + 1) * NB] = Linp[K] @ y[K * NB:(K + 1) * NB]
        for I in cols[K]:
            y[I * NB:(I + 1) * NB] -= Lnp[(I, K)] @ y[K * NB:(K + 1) * NB]
    for K in reversed(range(nt)):
        for I in cols[K]:
            y[K * NB:(K + 1) * NB] -= Lnp[(I, K)].T @ y[I * NB:(I + 1) * NB]
        y[K * NB:(K + 1) * NB] = Linp[K].T @ y[K * NB:(K + 1) * NB]
    return y


def tile_err(X, R, keys=None):
    """max |X - R| / max |R| over the tiles `keys` (default: R's)."""
    keys = list(R.keys()) if keys is None else keys
    num = max(float(np.abs(np.asarray(X[k], dtype=LD) - np.asarray(R[k], dtype=LD)).max()) for k in keys)
    den = max(float(np.abs(np.asarray(R[k], dtype=np.float64)).max()) for k in keys)
    return num / den


def vec_err(x, r):
    return float(np.abs(np.asarray(x, dtype=LD) - r).max() / np.abs(np.asarray(r, dtype=np.float64)).max())


def referee(e_gpu, e_np, floor):
    """The project's referee rule: the device is at most 8 x as far from the reference as numpy fp64, or below a floor."""
    return e_gpu <= max(8.0 * e_np, floor)
