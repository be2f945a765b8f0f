"""The option "diag_update_lower" (default on): a trailing update whose target is a DIAGONAL tile, C_II -= L_IK L_IK^T, computes
the 48 x 48 blocks on and left of the diagonal only -- in k_tile_gemm_nt (strips dealt again over the four waves),
k_tile_gemm_nt_small (the three units right of the diagonal return) and k_factor_flow (kind 2: wait and publish only; kind 3: 54 of
the 81 16 x 16 blocks).  Every computed element is summed as before, so against the option off (all nine blocks):
  - the lower triangle of every factor tile, all of Linv and a solution are bit-identical;
  - the lower triangle meets the bounds and the referee rule of the crafted-SPD tests (test_gpu_tile_cholesky.check_case);
  - a large finite sentinel in the 48 x 48 blocks right of the diagonal of every diagonal tile of the INPUT changes nothing:
    nobody reads what is no longer maintained;
  - the selected inverse, a bundle-adjustment step and cost and an SE3 pose-graph step and cost are bit-identical.
Shapes (tile columns): dense(3) -- the smallest in which one diagonal tile takes two updates from different source columns, and
the smallest whose dataflow launch (default cost model; dense(2) already has one, 20 units) holds a whole-tile unit on a diagonal
target beside the 48 x 48 units -- with the dataflow launch and with factor_flow = 0; arrow(4): the last diagonal tile takes four
updates, the others none; 57 independent pairs, factor_flow = 0: one launch of 57 diagonal-target updates, the smallest batch
over the 56 of the small-batch kernel (launch_tile_gemm_nt), so k_tile_gemm_nt's own strips run."""
import numpy as np
import pytest

import tile_ref as tr
from test_gpu_tile_cholesky import _mk, _run, check_case

pytestmark = pytest.mark.gpu

NB = tr.NB
SENTINEL = 2.0 ** 100


def _pairs(m):
    return tr.pattern_from_edges(2 * m, [(2 * i + 1, 2 * i) for i in range(m)])


# The sweeps whose x is the same bits in every run, so that two handles can be compared: level by level (tri_dataflow 0) where
# every block of a level has one writer; on the arrow the four leaves add to the border block in one launch, with atomics in the
# level form -- there the dataflow sweeps, which fold a block's products in list order.
SHAPES = {
    "dense3_flow": (lambda: tr.dense(3), dict(tri_dataflow=0)),
    "dense3_levels": (lambda: tr.dense(3), dict(tri_dataflow=0, factor_flow=0)),
    "arrow4": (lambda: tr.arrow(4), dict(tri_dataflow=1)),
    "arrow4_levels": (lambda: tr.arrow(4), dict(tri_dataflow=1, factor_flow=0)),
    "pairs57_large_kernel": (lambda: _pairs(57), dict(tri_dataflow=0, factor_flow=0)),
}


@pytest.fixture(scope="module")
def cases():
    """name -> (pattern, options, A, L0, right-hand side): built once, never written."""
    out = {}
    for i, (name, (mk, opts)) in enumerate(SHAPES.items()):
        pat = mk()
        A, L0 = tr.exact_case(pat, np.random.default_rng(700 + i), q=14, diag_exp=(-4, 4))
        b = np.random.default_rng(800 + i).standard_normal((1, pat.shape[0] * NB))
        out[name] = (pat, opts, A, L0, b)
    return out


def _poisoned(A, nt, value=SENTINEL):
    """A with the 48 x 48 blocks right of the diagonal of every diagonal tile set to `value` (default: large and finite)."""
    P = dict(A)
    for K in range(nt):
        t = A[(K, K)].copy()
        for bi in range(3):
            t[48 * bi:48 * bi + 48, 48 * (bi + 1):] = value
        P[(K, K)] = t
    return P


def _same(a, b, what):
    for k in ("L", "Linv", "x"):
        assert np.array_equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize("name", list(SHAPES))
def test_lower_triangle_linv_and_solution_are_the_bits_of_full_updates(name, cases):
    from apex_solver_amd import capi

    pat, opts, A, L0, b = cases[name]
    nt = pat.shape[0]
    units = capi.plan_lists(pat, "units", factor_flow=opts.get("factor_flow", -1))
    if name == "dense3_flow":   # columns of "units": ... kind at 13, C / A / B tiles before it; a diagonal target has A == B
        kinds = {int(u[13]) & 15 for u in units if (u[2], u[3]) == (u[4], u[5]) and (int(u[13]) & 15) in (2, 3)}
        assert kinds == {2, 3}, kinds
    flow = opts.get("factor_flow", -1) != 0
    if not flow:
        assert len(units) == 0
    with _mk(pat, diag_update_lower=0, **opts) as full, _mk(pat, diag_update_lower=1, **opts) as low:
        assert (low.flow_units > 0) == flow
        r_full = _run(full, A, z=False, rhs=b)
        r_low = _run(low, A, z=False, rhs=b)
        assert r_full["failed"] == 0 and r_low["failed"] == 0
        _same(r_full, r_low, name)
        # the sentinel: in the input of the run with the option on
        r_p = _run(low, _poisoned(A, nt), z=False, rhs=b)
        assert r_p["failed"] == 0
        _same(r_full, r_p, name + " poisoned")
        # ... and the lower triangle against the exact factor, by the rules of the crafted-SPD tests: all of check_case on the
        # small shapes; on the 114 tiles of the large batch its factor checks (the backward bound, the referee rule with numpy's
        # tile factor and the floor 8 n u), whose references cost nothing
        if nt <= 8:
            check_case(f"diag_update_lower {name}", low, pat, A, L0=L0, n_rhs=1, repeat=False)
        else:
            keys = tr.filled_pattern(pat)
            Lh = tr.from_slots(r_low["L"], low, keys)
            r_f = tr.factor_ratio(A, Lh, pat, L0=L0, X=r_low["Linv"])
            Lnp, _ = tr.tile_cholesky(A, pat, ld=False)
            Lref = {k: np.asarray(v, dtype=tr.LD) for k, v in L0.items()}
            e_l, e_lnp = tr.tile_err(Lh, Lref), tr.tile_err(Lnp, Lref)
            print(f"TILECHOL diag_update_lower {name}: factor {r_f:.3g} | e_L {e_l:.2e} (np {e_lnp:.2e})")
            assert r_f <= 1.0 and tr.referee(e_l, e_lnp, 8 * nt * NB * tr.U), (r_f, e_l, e_lnp)


def test_raw_upper_blocks_are_left_alone(cases):
    """The saving is real: with 1.0 in the blocks right of the diagonal 48 x 48 blocks of the input, the last diagonal tile -- four
    updates -- still holds it there with the option on, while full updates have written those blocks."""
    pat, opts, A, L0, b = cases["arrow4_levels"]
    nt = pat.shape[0]
    P = _poisoned(A, nt, 1.0)
    with _mk(pat, diag_update_lower=1, **opts) as low, _mk(pat, diag_update_lower=0, **opts) as full:
        for dev, kept in ((low, True), (full, False)):
            dev.set(tr.touched_array(P, dev))
            assert dev.factor() == 0
            t = dev.get("tiles")[dev.slot[nt - 1, nt - 1]]
            up = np.concatenate([t[48 * bi:48 * bi + 48, 48 * (bi + 1):].ravel() for bi in range(2)])
            assert bool((up == 1.0).all()) == kept


def test_selected_inverse_is_identical(cases):
    pat, opts, A, L0, b = cases["arrow4"]
    with _mk(pat, diag_update_lower=0) as full, _mk(pat, diag_update_lower=1) as low:
        z = [_run(d, A, z=True)["Z"] for d in (full, low)]
    assert np.array_equal(z[0], z[1])


def test_ba_step_and_cost_are_identical():
    import apex_solver_amd as pkg
    from apex_solver_amd.solver import GpuSchurComplementSolver, OptimizationType, Problem

    d = pkg.synthetic.make_problem(40, 1500, 3, 7, config_id=1)
    prob = Problem.bundle_adjustment(d, OptimizationType.SelfCalibration)
    out = []
    for on in (0, 1):
        s = GpuSchurComplementSolver(0).with_option("diag_update_lower", on).initialize_structure(prob)
        s.set_parameters(d.poses, d.intr, d.points)
        step = s.solve_augmented_equation(1e-3)
        info = s.info()
        out.append((np.array(step), s.eval_step()))
        s.close()
    assert info["n_update_diag"] > 0 and info["n_update_diag"] < info["n_update"]
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]


def test_se3_step_and_cost_are_identical():
    import apex_solver_amd as pkg
    from apex_solver_amd.pose_graph import GpuSparseCholeskySolver, PoseGraphProblem

    g = pkg.synthetic.make_sphere(10, 12)
    prob = PoseGraphProblem.pose_graph(g)
    out = []
    for on in (0, 1):   # (row-owned assembly: H and the gradient are the same bits in both runs)
        s = GpuSparseCholeskySolver(0).with_option("row_owned_assembly", 1).with_option("diag_update_lower", on).initialize_structure(prob)
        s.set_parameters(g.poses)
        step = s.solve_augmented_equation(1e-3)
        info = s.info()
        out.append((np.array(step), s.eval_step()))
        s.close()
    assert info["n_update_diag"] > 0
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]
