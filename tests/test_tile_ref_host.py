"""The references and bounds of the tile Cholesky tests (tests/tile_ref.py) on the CPU: the exact construction is exact,
the long double references are far closer to a 40-digit mpmath reference than fp64 is, and every bound rejects a factor
that is wrong in the ways a kernel goes wrong (a missed update term, a pivot whose Newton step is missing) -- so the GPU
assertions in tests/test_gpu_tile_cholesky.py can fail."""
import numpy as np
import pytest

import tile_ref as tr

NB = tr.NB


@pytest.mark.parametrize("name", ["nt1", "band", "arrow", "blockdiag", "dense"])
def test_exact_construction_is_exact(name):
    rng = np.random.default_rng(7)
    pat = {"nt1": tr.dense(1), "band": tr.band(3), "arrow": tr.arrow(3), "blockdiag": tr.block_diagonal(3), "dense": tr.dense(3)}[name]
    kw = dict(q=20, pivots={15: -20}) if name == "nt1" else dict(diag_exp=(-3, 4))
    M, q = tr.exact_factor(pat, rng, **kw)
    Ai = tr.product_int(M, pat)
    A, L0 = tr.exact_case(pat, np.random.default_rng(7), **kw)
    for k, a in A.items():
        assert np.array_equal(a * 2.0 ** (2 * q), Ai[k].astype(np.float64))      # A 2^(2q) is the int64 product, exactly
        assert np.array_equal(np.ldexp(a, 2 * q).astype(np.int64), Ai[k])
    # graded: D A D has the factor D L0 (power-of-two scaling is exact)
    e = np.random.default_rng(1).integers(-200, 201, size=pat.shape[0] * NB)
    As, Ls = tr.scale_rows(A, e), tr.scale_rows(L0, e, cols=False)
    for k in A:
        assert np.array_equal(np.ldexp(As[k], -e[k[0] * NB:(k[0] + 1) * NB, None] - e[None, k[1] * NB:(k[1] + 1) * NB]), A[k])
    assert tr.factor_ratio(As, Ls, pat, L0=Ls) == 0.0


def _mp_chol_inv(a, dps=40):
    import mpmath as mp

    mp.mp.dps = dps
    n = a.shape[0]
    A = mp.matrix([[mp.mpf(float(a[i, j])) for j in range(n)] for i in range(n)])
    L = mp.cholesky(A)
    Li = mp.inverse(L)
    return L, Li, mp


def test_long_double_references_beat_fp64_against_mpmath():
    """chol_ld / tri_inv_ld / the refined solve on one small SPD case each, at least 1e3 x closer to mpmath than fp64."""
    from scipy.linalg import cho_solve

    rng = np.random.default_rng(3)
    n = 40
    B = rng.integers(-9, 10, size=(n, n)).astype(np.float64)
    a = B @ B.T + np.diag(np.ldexp(1.0, -rng.integers(0, 20, size=n)))   # exact integers + dyadic diagonal, kappa ~ 1e6
    L, Li, mp = _mp_chol_inv(a)

    def mpld(v):   # (through a 30-digit string: no fp64 rounding on the way)
        return tr.LD(mp.nstr(v, 30))
    Lm = np.array([[mpld(L[i, j]) for j in range(n)] for i in range(n)], dtype=tr.LD)
    Lim = np.array([[mpld(Li[i, j]) for j in range(n)] for i in range(n)], dtype=tr.LD)
    def err(x, ref):
        return float(np.abs(np.asarray(x, dtype=tr.LD) - ref).max() / np.abs(ref.astype(np.float64)).max())
    Lld, Lnp = tr.chol_ld(a), np.linalg.cholesky(a)
    assert err(Lld, Lm) * 1e3 <= err(Lnp, Lm)
    assert err(tr.tri_inv_ld(Lm), Lim) * 1e3 <= err(np.linalg.inv(Lnp.astype(np.float64)), Lim)
    # x: one case through the refined tile solve (one 144 tile: a padded copy of the 40 x 40 system)
    A = np.eye(NB)
    A[:n, :n] = a
    b = np.zeros(NB)
    b[:n] = rng.standard_normal(n)
    pat = tr.dense(1)
    Lt, Lit = tr.tile_cholesky({(0, 0): A}, pat)
    x = tr.refined_solve({(0, 0): A}, Lt, Lit, b, pat)
    xm = mp.lu_solve(mp.matrix(a.tolist()), mp.matrix(b[:n].tolist()))
    xm = np.array([mpld(v) for v in xm], dtype=tr.LD)
    xnp = cho_solve((Lnp, True), b[:n])
    assert tr.vec_err(x[:n], xm) * 1e3 <= tr.vec_err(xnp, xm)
    # Z: where L0 is exact (a = L0 L0^T with integer L0) the long double reference is L0^-T L0^-1 (tile_ref.selected_inverse)
    L0 = np.tril(rng.integers(-4, 5, size=(n, n)), -1).astype(np.float64) + np.diag(np.ldexp(1.0, rng.integers(-6, 4, size=n)))
    a = L0 @ L0.T
    L0t = np.eye(NB)
    L0t[:n, :n] = L0
    Z = tr.selected_inverse({(0, 0): L0t}, {0: tr.tri_inv_ld(L0t)}, pat)[(0, 0)][:n, :n]
    _, Limp, _ = _mp_chol_inv(a)
    Zmp = Limp.T * Limp
    Zm = np.array([[mpld(Zmp[i, j]) for j in range(n)] for i in range(n)], dtype=tr.LD)
    assert err(Z, Zm) * 1e3 <= err(np.linalg.inv(a), Zm)


def _case():
    rng = np.random.default_rng(5)
    pat = tr.band(3)
    A, L0 = tr.exact_case(pat, rng)
    return pat, A, L0


def test_factor_bound_rejects_a_missed_update_term():
    pat, A, L0 = _case()
    assert tr.factor_ratio(A, L0, pat, L0=L0) == 0.0
    assert tr.factor_ratio(A, L0, pat) <= 1.0          # (the long double path agrees: the exact factor meets the bound)
    # L(1,0)[i, j] as if the update of A(1,0)[i, j] by one term L(1,0)[i, k] L(0,0)[j, k] (k < j) had been left out
    i, j, k = 37, 20, 3
    bad = dict(L0)
    t = L0[(1, 0)].copy()
    t[i, j] += L0[(1, 0)][i, k] * L0[(0, 0)][j, k] / L0[(0, 0)][j, j]
    bad[(1, 0)] = t
    assert tr.factor_ratio(A, bad, pat, L0=L0) > 1.0
    assert tr.factor_ratio(A, bad, pat) > 1.0
    Xs = {K: np.asarray(tr.tri_inv_ld(L0[(K, K)]), dtype=np.float64) for K in range(3)}
    assert tr.factor_ratio(A, L0, pat, L0=L0, X=Xs) == 0.0
    assert tr.factor_ratio(A, bad, pat, L0=L0, X=Xs) > 1.0   # (the bound of the inverse-based panel solve still rejects it)
    # a missed last update of a diagonal tile: L(1,1) from A(1,1) without the L(1,0) L(1,0)^T term
    bad2 = dict(L0)
    bad2[(1, 1)] = np.linalg.cholesky(A[(1, 1)] - L0[(1, 0)] @ L0[(1, 0)].T + np.outer(L0[(1, 0)][:, 5], L0[(1, 0)][:, 5]))
    assert tr.factor_ratio(A, bad2, pat) > 1.0


def test_bounds_reject_a_pivot_without_its_newton_step():
    """A pivot off by 1e-8 relative (what a missing Newton step after the approximate rsq leaves) fails the factor bound,
    the Linv residual and the solve bound."""
    pat, A, L0 = _case()
    Li = {K: np.asarray(tr.tri_inv_ld(L0[(K, K)]), dtype=np.float64) for K in range(3)}
    assert max(tr.linv_ratio(L0[(K, K)], Li[K]) for K in range(3)) <= 1.0
    r = 17
    bad = dict(L0)
    t = L0[(1, 1)].copy()
    t[r, r] *= 1 + 1e-8
    bad[(1, 1)] = t
    assert tr.factor_ratio(A, bad, pat, L0=L0) > 1.0
    assert tr.factor_ratio(A, bad, pat, L0=L0, X=Li) > 1.0
    X = Li[1].copy()
    X[r, :] *= 1 - 1e-8   # row r of L^-1 scaled by the wrong 1 / L_rr
    assert tr.linv_ratio(L0[(1, 1)], X) > 1.0
    nt = 3
    b = np.random.default_rng(2).standard_normal(nt * NB)
    x = np.asarray(tr.refined_solve(A, L0, Li, b, pat), dtype=np.float64)
    assert tr.solve_ratio(A, L0, x, b, nt) <= 1.0
    xb = x.copy()
    xb[NB + r] *= 1 + 1e-8
    assert tr.solve_ratio(A, L0, xb, b, nt) > 1.0
    y = np.asarray(tr.matvec_ld(A, x, nt), dtype=np.float64)
    assert tr.matvec_ratio(A, x, y, nt) <= 1.0
    y[5] *= 1 + 1e-10
    assert tr.matvec_ratio(A, x, y, nt) > 1.0


def test_selected_inverse_reference_on_a_fill_pattern():
    """The long double Takahashi recurrence on a pattern with fill matches numpy's dense inverse to fp64 accuracy."""
    pat = tr.star_of_chains(2, 2)
    A = tr.dominant_case(pat, np.random.default_rng(4))
    L, Li = tr.tile_cholesky(A, pat)
    Z = tr.selected_inverse(L, Li, pat)
    Zd = np.linalg.inv(tr.dense_of(A, pat.shape[0]))
    for (I, J), z in Z.items():
        ref = Zd[I * NB:(I + 1) * NB, J * NB:(J + 1) * NB]
        assert np.abs(np.asarray(z, dtype=np.float64) - ref).max() <= 1e-13 * np.abs(Zd).max()
    assert tr.factor_ratio(A, {k: np.asarray(v, dtype=np.float64) for k, v in L.items()}, pat) <= 1.0


def test_tile_hook_fails_loudly_without_gpu():
    import torch

    import apex_solver_amd as pkg

    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    with pytest.raises(pkg.capi.LinAlgError) as e:
        pkg.capi.TileCholesky(tr.band(2))
    assert e.value.kind == "DeviceError"
