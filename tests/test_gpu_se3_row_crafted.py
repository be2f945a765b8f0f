"""The row-owned SE3 assembly (k_pg6_assemble, k_pg2_priors<Se3Manifold> of csrc/pg_kernels.hip: the option "row_owned_assembly"
on an SE3 handle) on every SE3 crafted graph of tests/pg_asm_cases.py, with the checks tests/test_gpu_pg_crafted.py applies to
the atomic assembly -- the long double reference of tests/pg_asm_ref.py, D x D block by block and vertex row by vertex row:
err <= max(8 e_np, gamma(P + C0) M) -- and, because every sum now has a fixed order, a second assembly on the same handle that
is equal to the first bit for bit.  tests/test_se3_row_host.py replays the same row function on the CPU.  Every run prints one
PGASM line with the worst ratio of each checked quantity."""
import numpy as np
import pytest

import pg_asm_cases as pc
import pg_asm_ref as pr
from apex_solver_amd.pose_graph import GpuSparseCholeskySolver

pytestmark = pytest.mark.gpu
SOLVED = ("straddle", "loops", "hub_hi")
RUNS = [(n, p, nd) for n, p, m in pc.all_runs() if m == "se3" for nd in ((0, 1) if n == "permuted" else (None,))]


def _id(run):
    n, p, nd = run
    return f"{n}-{p}-se3-row" + ("" if nd is None else f"-nd{nd}")


@pytest.mark.parametrize("run", RUNS, ids=[_id(r) for r in RUNS])
def test_crafted_graph_row_owned(run):
    name, pol, nd = run
    man = "se3"
    c, p = pc.build(name, man), pc.policy(name, man, pol)
    D, lam, col = c.D, pc.LAM, p.prob.pose_col
    s = GpuSparseCholeskySolver().with_option("row_owned_assembly", 1)
    if nd is not None:
        s.with_option("nested_dissection", nd)
    s.initialize_structure(p.prob)
    s.set_parameters(c.d.poses)
    J, r = s.get_jacobian_blocks(), s.get_residual()
    nb = pc.numpy_blocks(name, man, pol)
    assert np.abs(r - nb.r).max() <= 1e-9 * max(1.0, np.abs(nb.r).max()) and np.abs(J - nb.J).max() <= 1e-9 * max(1.0, np.abs(nb.J).max())
    info = s.get_information()
    assert (info is None) if p.info is None else np.array_equal(info, p.info)
    priors = None
    if c.priors:
        pv, pres_np, psc = pc.numpy_blocks(name, man, "none").priors
        pres = s.get_prior_residual()
        assert np.abs(pres - pres_np).max() <= 1e-13                       # in the caller's order, though the device holds them sorted
        priors = (pv, pres, psc)
    ld, f64 = pc.reference(name, man, pol, J, r, priors, lam)
    if pol == "tukey":
        dead = ~ld.mags["live"]
        assert dead.any() and not r[dead].any() and not J[dead].any() and r[~dead].any(axis=1).all()
    C0 = pr.c0(D, p.kernel)

    H, g = s.get_hessian(lam)
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
    H2, g2 = s.get_hessian(lam)                                              # a second assembly on the same handle
    H2, g2 = H2.copy(), g2.copy()

    step = grad = None
    if name in SOLVED:
        step = s.solve_augmented_equation(lam)
        grad = s.get_gradient().copy()
        ratios["grad"] = pr.g_check(pr.rows_of(grad, col, D), ld, f64, C0)
    scaled = None
    if name == "straddle":                                                   # Jacobi scaling: H := D H D, then lambda
        norms = s.compute_column_norms()
        ld0, f640 = pc.reference(name, man, pol, J, r, priors, 0.0)
        ratios["norms"] = pr.norms_check(pr.rows_of(norms, col, D), ld0, f640, C0)
        scal = 1.0 / (1.0 + norms)
        s.apply_column_scaling(scal)
        Hs, gs = s.get_hessian(lam)
        lds, f64s = pc.reference(name, man, pol, J, r, priors, lam, scaling=pr.rows_of(scal, col, D))
        Cs = pr.c0(D, p.kernel, scaled=True)
        rs, bads, strays = pr.h_check(pr.blocks_of(Hs, col, D), lds, f64s, Cs)
        ratios["H_scaled"] = np.concatenate([rs["diag"], rs["lower"], rs["upper"]])
        ratios["g_scaled"] = pr.g_check(pr.rows_of(gs, col, D), lds, f64s, Cs)
        scaled = (bads, strays, np.array_equal(Hs, Hs.T))
    pr.report(_id(run), ratios)
    s.close()

    assert not bad, [(t, int(ld.P_d[t[1]])) for t in bad[:8]]
    assert stray == 0                                                        # pairs without an edge: exactly 0, inside touched tiles too
    assert np.array_equal(H, H.T)
    quiet = np.nonzero(~ld.touched)[0]
    assert (H4[quiet, quiet] == lam * np.eye(D)).all() and not pr.rows_of(g, col, D)[ld.P_g == 0].any()
    if name == "isolated":
        assert set(c.facts.isolated) <= set(quiet.tolist())
    if name == "straddle" and pol == "tukey":
        assert c.facts.rejected_vertex in quiet
    for k in ("g", "cost", "jv") + (("grad",) if step is not None else ()) + (("norms", "g_scaled") if scaled else ()):
        v, at = pr.worst(ratios[k])
        assert v <= 1.0, (k, v, at)
    assert jv2 == jv
    assert np.array_equal(H, H2) and np.array_equal(g, g2)                   # row-owned: a fixed order, the same bits
    if step is not None:                                                     # what is factorised is what was exported
        res = pr.matvec(ld, pr.rows_of(step, col, D)) + ld.g
        assert np.linalg.norm(np.asarray(res, dtype=np.float64)) <= 1e-12 * np.linalg.norm(np.asarray(ld.g, dtype=np.float64))
    if scaled:
        assert not scaled[0] and scaled[1] == 0 and scaled[2], scaled[0][:8]
