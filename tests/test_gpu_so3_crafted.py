"""The SO3 instantiations of the row-owned assembly (k_pg2_assemble<So3Manifold, *>, k_pg2_priors<So3Manifold>, k_pg_cost_partial,
k_pg_jv_gram) on crafted graphs (so3_ref.crafted) against the long double block reference of tests/pg_asm_ref.py, 3 x 3 block by
block and vertex row by vertex row, exactly as tests/test_gpu_pg_crafted.py holds SE2 and SE3 (needs a real MI355X: `pytest -m gpu`):

    err <= max(8 e_np, gamma(P + C0) M)      per block of H (diagonal, lower, upper read separately), per row of g, cost, jv-Gram

with P the number of terms summed into the block, M their magnitude and C0 = so3_ref.c0 (pg_asm_ref's count with SO3's
linearisation chain, derived in so3_ref.py).  One term is added to pg_asm_ref's rule, in so3_ref.asm_reference: an edge's magnitudes
carry max(1, kappa), kappa = |s rho''/rho'| the condition number of the loss's weight -- 1 everywhere except on an edge next to
a cut-off (nv97-tukey has one 3 % inside Tukey's: rho' = 4.3e-4, kappa = 65; without the term its block sat at 1.45 times the bound,
every other block of every run below 0.07).  Pairs without an edge must hold exactly 0, a vertex without a live term exactly
lambda I and a zero gradient row.  The reference is built from the blocks the handle exports, so the linearisation is not on trial
here (tests/test_gpu_so3_parity.py holds it); where the kernels put the products is.  Every run prints one PGASM line."""
import numpy as np
import pytest

import pg_asm_ref as pr
import so3_ref as sr
from apex_solver_amd.pose_graph import GpuSparseCholeskySolver, PoseGraphProblem, create_loss_function

pytestmark = pytest.mark.gpu
LAM = 0.5
SHAPES = ("loop", "multi", "isolated", "hub_lo", "hub_hi", "cross", "nv47", "nv48", "nv49", "nv97", "ne255", "ne256", "ne257")
POLICIES = ("none", "cauchy", "weighted")
RUNS = [(n, p) for n in SHAPES for p in POLICIES] + [("isolated", "tukey"), ("nv97", "tukey"), ("loop", "andrews"), ("multi", "huber")]
SOLVED = ("loop", "hub_hi", "cross")


def problem(name, pol):
    d = sr.crafted(name)
    kw = {}
    if pol == "huber":
        kw["huber_delta"] = 0.4
    elif pol in ("cauchy", "weighted"):
        kw["loss"] = create_loss_function("cauchy", 1.0)
    elif pol == "tukey":
        kw["loss"] = create_loss_function("tukey", 1.5)
    elif pol == "andrews":
        kw["loss"] = create_loss_function("andrews", 1.2)
    if pol == "weighted":
        kw["information"] = sr.random_information(d.n_e)
    prob = PoseGraphProblem(d, manifold="so3", **kw)
    prob.add_prior("x0").add_prior("x1", data=d.poses[1] * 0.95 + 0.05, huber_delta=0.05).add_prior("x1", data=d.poses[1] * 0.9)
    return d, prob


@pytest.mark.parametrize("name,pol", RUNS, ids=[f"{n}-{p}" for n, p in RUNS])
def test_crafted_graph(name, pol):
    d, prob = problem(name, pol)
    D, col = 3, prob.pose_col
    s = GpuSparseCholeskySolver()
    if name == "cross":      # the premise is stated on the caller's order: keep it the device's (three tiles are not dissected anyway)
        s.with_option("nested_dissection", 0)
        t = d.e_from.astype(int) // sr.VPT - d.e_to.astype(int) // sr.VPT
        assert (t > 0).any() and (t < 0).any()
    s.initialize_structure(prob)
    s.set_parameters(d.poses)
    P = sr.So3Problem.from_problem(prob)
    J, r = s.get_jacobian_blocks(), s.get_residual()
    rn, Jn = P.edge_blocks()
    # the policy that was asked for is the one that ran (loosely: the parity file pins the exports)
    assert np.abs(r - rn).max() <= 1e-9 * max(1.0, np.abs(rn).max()) and np.abs(J - Jn).max() <= 1e-9 * max(1.0, np.abs(Jn).max())
    info = s.get_information()
    assert (info is None) if prob.information is None else np.array_equal(info, prob.information)
    pres = s.get_prior_residual()
    assert np.abs(pres - P.prior_blocks()[0]).max() <= 1e-13
    ld, f64 = sr.asm_reference(P, J, r, LAM, prior_residuals=pres)
    kernel = sr.kernel_policy(P)
    assert kernel == {"none": "legacy", "huber": "legacy", "weighted": "weighted"}.get(pol, "general")
    if pol == "tukey":
        dead = ~ld.mags["live"]
        assert dead.any() and not r[dead].any() and not J[dead].any() and r[~dead].any(axis=1).all()
    if pol == "andrews":
        assert (P.arms == 2).any()
    C0 = sr.c0(kernel)

    H, g = s.get_hessian(LAM)
    H, g = H.copy(), g.copy()
    H4 = pr.blocks_of(H, col, D)
    ratios, bad, stray = pr.h_check(H4, ld, f64, C0)
    ratios["g"] = pr.g_check(pr.rows_of(g, col, D), ld, f64, C0)
    ratios["cost"] = pr.scalar_check(s.compute_cost(), ld.cost, f64.cost, ld.M_cost, ld.n_terms, C0)
    rng = np.random.default_rng(7)
    a, b = rng.normal(size=(2, ld.n_v, D))
    ac, bc = pr.to_columns(a, col, D), pr.to_columns(b, col, D)
    jv = s.jv_gram(ac, bc)
    jl, jmag = ld.jv_gram(a, b)
    j64, _ = f64.jv_gram(a, b)
    ratios["jv"] = pr.scalar_check(jv, jl, j64, jmag, ld.n_terms, C0 + D)
    jv2 = s.jv_gram(ac, bc)
    H2, g2 = s.get_hessian(LAM)
    step = None
    if name in SOLVED:
        step = s.solve_augmented_equation(LAM)
        ratios["grad"] = pr.g_check(pr.rows_of(s.get_gradient().copy(), col, D), ld, f64, C0)
    pr.report(f"so3 {name}-{pol}" + (f" (worst kappa {ld.mags['kappa'].max():.3g})" if "kappa" in ld.mags else ""), ratios)
    s.close()

    assert not bad, [(t, int(ld.P_d[t[1]])) for t in bad[:8]]
    assert stray == 0                                                        # pairs without an edge: exactly 0
    assert np.array_equal(H, H.T)
    quiet = np.nonzero(~ld.touched)[0]
    assert (H4[quiet, quiet] == LAM * np.eye(D)).all() and not pr.rows_of(g, col, D)[ld.P_g == 0].any()
    if name == "isolated":
        assert {3, 9} <= set(quiet.tolist())
    if pol == "tukey":
        ef, et = d.e_from.astype(int), d.e_to.astype(int)
        all_cut = [v for v in range(2, d.n_v) if ((ef == v) | (et == v)).any() and dead[(ef == v) | (et == v)].all()]
        assert set(all_cut) <= set(quiet.tolist()) and (name != "nv97" or all_cut)      # a vertex whose every edge is cut is quiet
    for k in ("g", "cost", "jv") + (("grad",) if step is not None else ()):
        v, at = pr.worst(ratios[k])
        assert v <= 1.0, (k, v, at)
    assert jv2 == jv and np.array_equal(H, H2) and np.array_equal(g, g2)     # row-owned: a fixed order
    if step is not None:                                                     # what is factorised is what was exported
        res = pr.matvec(ld, pr.rows_of(step, col, D)) + ld.g
        assert np.linalg.norm(np.asarray(res, dtype=np.float64)) <= 1e-12 * np.linalg.norm(np.asarray(ld.g, dtype=np.float64))
