"""The camera priors of bundle adjustment (csrc/ba_prior_kernels.hip) prior by prior on the crafted sets of
tests/ba_prior_cases.py, against the long double reference of tests/ba_prior_ld.py (needs a real MI355X: `pytest -m gpu`).

The priors are added behind the graded kernels, so ONE handle assembled without and with them isolates their part exactly:
  a  premise   two assemblies without priors give the same bits of S, g_red and the gradient (no block adds atomically:
               tests/test_ba_prior_cases_host.py reads that off the pair lists)
  b  bits      with priors, every off-diagonal entry of S, every diagonal entry of a column with p = 0 and every g entry of
               such a column keep their bits; on `unobserved` S_ii is exactly lambda without a prior
  c  the part  S_ii - S0_ii against p_i, gradient - g0 against q_i, g_red - g_red0 against -q_i:
               err <= max(8 e_np, bound_i) + u |value the part was added onto|   (ba_prior_ld.py: bound, C0 = 35)
  d  the other consumers under the same rule, each with the roundings of its own last steps (written where they are used):
               both S x, the Gram sums, the cost, the column norms (as squares), prior_residuals() block by block
  e  the trial cost of eval_step at the retracted parameters (the cost-only path on the other parameter set), and clearing:
               S, g_red and the gradient return to the first run's bits
Each case prints one BAPRIOR line with the worst ratio (error / bound) of every quantity; every ratio must be <= 1.

Worst measured ratio over the cases, MI355X: S 0.95, gradient 0.95, g_red 0.96, matrix-free S x 0.98 (cost257: the one rounding
of the addition onto the larger entry is most of the bound there), explicit S x 0.0035, Gram 0.76, cost 0.27, norms 0.39,
residuals 0.27 / 0.094, trial cost 0.47, the step 0.029.  No defect was found in the kernels, the lists or the call sites.

Left out on purpose (tests/test_gpu_ba_priors.py holds them): LM / Dog-Leg histories, covariances, the three variants' full
steps, the scaled solve.  The one step checked is `unobserved`, where it is -q_i / (lambda + p_i) on the camera's columns."""
import numpy as np
import pytest

import ba_prior_cases as pc
import ba_prior_ld as pl
from apex_solver_amd import capi
from apex_solver_amd.solver import GpuSchurComplementSolver, OptimizationType, Problem

pytestmark = pytest.mark.gpu
LAM = pc.LAM
U = pl.U
OPT = {pc.SELFCAL: OptimizationType.SelfCalibration, pc.BA: OptimizationType.BundleAdjustment}


def snapshot(s, x, a, b):
    out = dict(step=s.solve_augmented_equation(LAM))
    out["grad"] = s.get_gradient().copy()
    out["S"], out["gred"] = s.get_schur()
    out["ye"], out["yi"] = s.schur_matvec(LAM, x)
    out["gram"] = np.array(s.jv_gram(a, b))
    out["cost"] = s.compute_cost()
    out["norms"] = s.compute_column_norms()
    return out


@pytest.mark.parametrize("name", pc.CASES)
def test_prior_by_prior(name):
    mode, d, pp, ip = pc.case(name)
    dc = pc.width(name)
    n_cam = d.n_cam
    prob = Problem(d, OPT[mode], 1.0)            # (no gauge mask: lambda carries it)
    lay = prob.layout
    cols = np.concatenate([lay.pose_col[:, None] + np.arange(6)[None], lay.intr_col[:, None] + np.arange(3)[None]], axis=1)
    nc = lay.cam_dof
    rng = np.random.default_rng(7)
    x = rng.normal(size=nc); a, b = rng.normal(size=(2, lay.total_dof))
    n_obs_cam = np.bincount(d.cam_idx.astype(int), minlength=n_cam)
    ld, f64 = pl.pair(d.poses, d.intr, pp, ip)
    has = ld.k > 0                                # (n_cam, 9): the columns that take a prior
    assert not has[:, dc:].any()
    s = GpuSchurComplementSolver(0).initialize_structure(prob)
    try:
        s.set_parameters(d.poses, d.intr, d.points)
        # ---- a: the premise
        A = snapshot(s, x, a, b)
        A2 = snapshot(s, x, a, b)
        for k in ("S", "gred", "grad", "step"):
            assert np.array_equal(A[k], A2[k]), k
        same = {k: np.array_equal(A[k], A2[k]) for k in ("ye", "yi", "gram", "cost")}
        del A2
        # ---- with the priors
        s.set_priors(pp, ip if dc == 9 else None)
        B = snapshot(s, x, a, b)
        rp, ri = s.prior_residuals()
        # ---- b: what keeps its bits
        changed = B["S"] != A["S"]
        diag = np.zeros_like(changed); diag[cols[has], cols[has]] = True
        assert not (changed & ~diag).any()        # nothing but the diagonal entries of the columns with a prior
        assert np.array_equal(B["S"], B["S"].T)
        keep = np.ones(lay.total_dof, dtype=bool); keep[cols[has]] = False
        assert np.array_equal(B["grad"][keep], A["grad"][keep]) and np.array_equal(B["gred"][keep[:nc]], A["gred"][keep[:nc]])
        if same["yi"]:
            assert np.array_equal(B["yi"][keep[:nc]], A["yi"][keep[:nc]])     # y += p x touches its own column only
        S0d, S1d = A["S"][cols, cols], B["S"][cols, cols]
        if name == "unobserved":
            assert (S0d[[3, 6]] == LAM).all() and (S1d[6] == LAM).all() and (S1d[3] > LAM).all()
            assert not A["S"][cols[3]][:, np.delete(np.arange(nc), cols[3])].any()
        ratios = {}
        # ---- c: the part the prior adds
        ratios["S"] = pl.check(S1d - S0d, ld.p, f64.p, ld.pb, onto=S1d)
        g0, g1 = A["grad"][cols], B["grad"][cols]
        ratios["grad"] = pl.check(g1 - g0, ld.q, f64.q, ld.qb, onto=g1)
        r0, r1 = A["gred"][cols], B["gred"][cols]
        ratios["gred"] = pl.check(r1 - r0, -ld.q, -f64.q, ld.qb, onto=r1)
        # ---- d: the other consumers
        # S x = y0 + p x.  The product is one rounding more (two where it is fused into a sum).  Matrix-free: one addition onto
        # y0.  Explicit: p sits inside S_ii, one term of a row sum of at most n_c + 144 terms whose later partial sums all
        # round anew: twice gamma(n_c + 144) of the row's magnitude (|S| |x|)_i.  A path that does not repeat its own bits
        # without priors (never seen; `same`) takes the any-order allowance too.
        xs = x[cols]
        px_ld, px_64 = ld.p * np.asarray(xs, dtype=pl.LD), f64.p * xs
        mag = (np.abs(B["S"]) @ np.abs(x))[cols]
        pxb = (ld.pb + pl.gam(2) * ld.pmag) * np.abs(xs)
        any_order = 2.0 * pl.gam(nc + 144) * mag
        ratios["mv_explicit"] = pl.check(B["ye"][cols] - A["ye"][cols], px_ld, px_64, pxb + any_order)
        ratios["mv_implicit"] = pl.check(B["yi"][cols] - A["yi"][cols], px_ld, px_64, pxb + (0.0 if same["yi"] else any_order), onto=B["yi"][cols])
        # Gram sums: sum_i p_i a_i b_i over the n_c columns, a product of three (2 roundings) summed in a tree, added onto the
        # observations' sum (one rounding; 2 gamma(2 n_obs + 256) of the sums' magnitude where that sum does not repeat its bits)
        av, bv = a[cols], b[cols]
        gram = lambda R, u_, v_: np.sum(R.p * np.asarray(u_ * v_, dtype=R.T))
        g_ld = np.array([gram(ld, av, av), gram(ld, av, bv), gram(ld, bv, bv)])
        g_64 = np.array([gram(f64, av, av), gram(f64, av, bv), gram(f64, bv, bv)], dtype=np.float64)
        w = ld.pb + pl.gam(2 + dc * n_cam) * ld.pmag
        gb = np.array([np.sum(w * av * av), np.sum(w * np.abs(av * bv)), np.sum(w * bv * bv)])
        gmag = np.array([B["gram"][0], np.sqrt(B["gram"][0] * B["gram"][2]), B["gram"][2]])
        ratios["gram"] = pl.check(B["gram"] - A["gram"], g_ld, g_64, gb + (0.0 if same["gram"] else 2.0 * pl.gam(2 * d.n_obs + 256) * gmag), onto=gmag)
        # cost = 0.5 sqrt(ss)^2 (cost_from_sumsq): a root and a square on either side (3 u each, no credit for the root), one
        # addition of the priors' sum onto ss: 7 roundings relative to 2 cost; 8 allowed
        total, cost_b = ld.total_cost()
        assert same["cost"]
        ratios["cost"] = pl.check(2.0 * (B["cost"] - A["cost"]), total, f64.total_cost()[0], cost_b, onto=2.0 * B["cost"], roundings=8)
        # column norms, compared as squares: the observations' sum is atomic (tests/test_gpu_column_order.py: two orders of a
        # sum of k non-negative terms differ by at most 2 (k - 1) u relative), a root and a square on either side 4 u, the
        # addition of p one: (2 k_c + 5) u n^2, k_c the camera's observations
        n0, n1 = A["norms"][cols] ** 2, B["norms"][cols] ** 2
        ratios["norms"] = pl.check(n1 - n0, ld.p, f64.p, ld.pb, onto=np.maximum(n0, n1), roundings=(2 * n_obs_cam + 5)[:, None])
        # corrected residuals in the caller's order: 17 roundings of C0's count; a quaternion row carries QX u j |x_a| more
        jp = np.abs(np.asarray(ld.P.j, dtype=np.float64))[:, None] * np.concatenate([np.zeros((len(pp), 3)), ld.P.xa[:, 3:]], axis=1) if pp else 0.0
        ratios["rp"] = pl.check(rp, ld.rp, f64.rp, pl.gam(17 + 2 * ld.P.e)[:, None] * np.abs(rp) + pl.gam(pl.QX) * jp)
        ratios["ri"] = pl.check(ri, ld.ri, f64.ri, pl.gam(17) * np.abs(ri))
        if name == "threshold":                   # ON the boundary the block is not corrected: its residual is delta e_a exactly
            for label, (c, kind, row, side) in pc.THRESHOLD_BLOCKS.items():
                got = (rp if kind == "pose" else ri)[[q[0] for q in (pp if kind == "pose" else ip)].index(c)]
                if row is not None and side == 0:
                    want = np.zeros_like(got); want[row] = pc.DELTA_T
                    assert np.array_equal(got, want), label
                elif row is not None:
                    assert 0 < got[row] < pc.DELTA_T * (1 + 2.0 ** -40) and np.count_nonzero(got) == 1, label
        if name == "unobserved":
            # the camera is decoupled: step_i = g_red_i / S_ii = -q_i / (lambda + p_i): p and q under their bounds, the addition
            # of lambda, the root, a division (or reciprocal and product) in each sweep: 6 roundings
            c = 3
            want = lambda R: -R.q[c] / (R.T(LAM) + R.p[c])
            w64 = np.abs(np.asarray(want(ld), dtype=np.float64))
            rel = ld.qb[c] / np.maximum(np.abs(np.asarray(ld.q[c], dtype=np.float64)), 1e-300) + ld.pb[c] / (LAM + np.asarray(ld.p[c], dtype=np.float64))
            ratios["step"] = pl.check(B["step"][cols[c]], want(ld), want(f64), w64 * (rel + pl.gam(6)))
            assert not B["step"][cols[6]].any()
        # ---- e: the trial cost, then clearing
        s.solve_augmented_equation(LAM)
        trial = s.eval_step()
        s.commit_step()
        poses1, intr1, pts1 = s.get_parameters()
        here = s.compute_cost()
        s.set_priors([], [] if dc == 9 else None)
        assert s.prior_residuals()[0].shape == (0, 7)
        here0 = s.compute_cost()
        ld1, f641 = pl.pair(poses1, intr1, pp, ip)
        t1, t1b = ld1.total_cost()
        ratios["trial"] = pl.check(2.0 * (trial - here0), t1, f641.total_cost()[0], t1b, onto=2.0 * trial, roundings=8)
        ratios["cost_there"] = pl.check(2.0 * (here - here0), t1, f641.total_cost()[0], t1b, onto=2.0 * here, roundings=8)
        assert float(t1) != float(total)          # (the step moved the cameras that hold priors)
        s.set_parameters(d.poses, d.intr, d.points)
        C = snapshot(s, x, a, b)
        for k in ("S", "gred", "grad", "step"):
            assert np.array_equal(C[k], A[k]), k
        assert C["cost"] == A["cost"]
        if name == "as_coded":                    # w = 0: ba_prior_refusal does not accept it; the text, and the handle as it was
            with pytest.raises(capi.LinAlgError) as e:
                s.set_priors([(1, pp[0][1], None, 0.0)], None)
            assert "set_pose_priors: the weight of prior 0 must be finite and positive" in str(e.value)
            assert s.prior_residuals()[0].shape == (0, 7)
    finally:
        s.close()
    worst = {k: pl.worst(v) for k, v in ratios.items()}
    print(f"BAPRIOR {name} d_c {dc} cameras {n_cam} priors {len(pp)}+{len(ip)} repeat {''.join('y' if v else 'n' for v in same.values())}: "
          + "  ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 1.0, (k, v)
