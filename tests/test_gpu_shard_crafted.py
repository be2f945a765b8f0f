"""The sharded bundle-adjustment path rank by rank on the crafted structures of tests/shard_cases.py, all ranks
in ONE process on one GPU: sharded handles without a communicator export their partial systems, and
apexgpu_debug_lockstep_solve plays the exchanges of the distributed factorisation.  Every rank's partial S, g_red, H_ll^-1, g_l,
S x and cost are held to the long double reference of THAT rank's observations (schur_ref.pair over the landmarks
owned_landmarks() reports, lambda where the design puts it), under the bounds of tests/test_gpu_schur_crafted.py
(max(8 e_np, gamma(k) M)), the 1e-12 cost bound of tests/test_gpu_ba_loss.py, the 1e-13 backward error of
tests/test_gpu_parity.py and tile_ref.referee for the step.  The premises of the cases and the sensitivity of the bounds are
in tests/test_shard_cases_host.py.  Each test prints one SHARDREF line with its worst ratios.

Where lambda sits in a rank's partial: the explicit S (get_schur, the explicit S x) carries it on rank 0 under range sharding
and on the owner of the camera's tile column under tree sharding (lam_mask; rank 0 for the shared top); the matrix-free S x
carries it on rank 0 under either sharding; the columns no factor touches (six-column modes) on rank 0.

Reached through the lockstep solve only: the assembly of a tree-sharded rank FOR its factorisation (it clears and completes
only its own and the top tiles, solver.hip assemble_local, so its tiles are no partial S to export), the identity on the
padding rows of a partial last tile (pad_rank; the dense export stops at the last camera column), the summed top tiles, the
pivot flag and the two vector exchanges.

Worst measured ratio (error / bound, 1 fails) of every checked quantity over the cases, MI355X:
  partial, per rank   S 0.16 (arrow_pad_2 w2 form 3 cauchy; the same a second time)   g_red 0.046   H_ll^-1 0.017   g_l 0.014
                      S x explicit 0.0038   S x matrix-free 0.0039   cost 0.032 of 1e-12 (boundary3_1_2)
  partial, summed     S 0.16   g_red 0.036   cost 0.0016 of 1e-12
  lockstep            backward error 0.016 of 1e-13   forward error 3.5e-4 of the referee bound (kappa 5e7 .. 7e7, e_np 1e-9)
                      landmark step 0.011; seven of the ten cases assemble without atomics and repeat bit for bit (arrow_3,
                      whose camera 3 sees a landmark twice, adds atomically)
An empty rank (empty_heavy rank 2, empty_world8) faulted in the matrix-free S x when these cases first ran inside the whole
suite: k_implicit_cam's first loads are unconditional on a clamped index and read entry 0 of an observation list that was
empty and never written; DeviceBuffer::upload now clears an empty list's allocation (device_buffer.h)."""
import functools

import numpy as np
import pytest

import shard_cases as shc
import schur_ref as sr
import tile_ref as tr
from apex_solver_amd import capi
from apex_solver_amd.solver import GpuSchurComplementSolver, OptimizationType, Problem

pytestmark = pytest.mark.gpu
LAM = shc.LAM

# (case, world, Schur form, loss, tree sharding)
PARTIAL = ([(f"boundary_{c}", 2, 4, "huber", 1) for c in shc.CUTS]
           + [(f"boundary3_{k}", 3, 3, "huber", 1) for k in shc.CUTS3]
           + [("boundary3_129_257", 3, 4, "cauchy", 1), ("boundary_128", 2, 3, "cauchy", 1),
              ("empty_heavy", 4, 4, "huber", 1), ("empty_heavy", 4, 3, "cauchy", 1), ("empty_world8", 8, 4, "huber", 1),
              ("six_20", 2, 3, "huber", 1), ("six_25", 3, 3, "huber", 1), ("six_25", 3, 3, "cauchy", 1),
              ("arrow_2", 2, 4, "huber", 1), ("arrow_2", 2, 4, "huber", 0), ("arrow_pad_3", 3, 4, "huber", 1),
              ("arrow_pad_2", 2, 3, "cauchy", 1)])
LOCKSTEP = ([(name, shc.structure(name)[4][0], "huber", tree) for name in shc.ARROWS for tree in (1, 0)]
            + [("arrow_3", 3, "cauchy", 1), ("arrow_pad_2", 2, "cauchy", 0)])


def _solver(name, loss, shard=None, **options):
    n_cam, lists, lam, mode, worlds = shc.structure(name)
    d = shc.problem(name)
    ot = OptimizationType.SelfCalibration if mode == "selfcal" else OptimizationType.BundleAdjustment
    # Huber as the problem's own delta (the huber_delta kernels), the redescending loss through set_loss (the general ones)
    prob = Problem.bundle_adjustment(d, ot, 1.0) if loss == "huber" else Problem.bundle_adjustment(d, ot, None, loss=shc.LOSSES[loss])
    s = GpuSchurComplementSolver(0)
    for k, v in options.items():
        s.with_option(k, v)
    if shard:
        s.with_shard(*shard)
    s.initialize_structure(prob)
    s.set_parameters(d.poses, d.intr, d.points)
    return prob, s


@functools.lru_cache(maxsize=None)
def _blocks(name, loss):
    """The single-rank handle's corrected blocks, computed once per (case, loss), shared, never modified."""
    _, s = _solver(name, loss)
    jc, jl = s.get_jacobian_blocks()
    r = s.get_residual()
    s.close()
    for a in (jc, jl, r):
        a.setflags(write=False)
    return jc, jl, r


@functools.lru_cache(maxsize=None)
def _whole(name, loss):
    d = shc.problem(name)
    jc, jl, r = _blocks(name, loss)
    ld, f64 = sr.pair(d.n_cam, d.n_pt, d.cam_idx, d.pt_idx, jc, jl, r, LAM)
    assert ld.cond.max() <= 1e8, ld.cond.max()
    return ld, f64


def _worst(ratios):
    return {k: sr.worst(v)[0] for k, v in ratios.items()}


def _report(label, ratios):
    parts = [f"{k} {sr.worst(v)[0]:.3g}@{','.join(str(a) for a in sr.worst(v)[1])}" for k, v in ratios.items()]
    print(f"SHARDREF {label}: " + "  ".join(parts))


def _merge(total, ratios):
    for k, v in ratios.items():
        v = np.atleast_1d(np.asarray(v, dtype=np.float64))
        total[k] = v if k not in total or sr.worst(v)[0] > sr.worst(total[k])[0] else total[k]


@pytest.mark.parametrize("name,world,form,loss,tree", PARTIAL, ids=[f"{n}-w{w}-form{f}-{l}-{'tree' if t else 'range'}" for n, w, f, l, t in PARTIAL])
def test_partial_assembly_rank_by_rank(name, world, form, loss, tree):
    n_cam, lists, lam, mode, worlds = shc.structure(name)
    d = shc.problem(name)
    dc = 9 if mode == "selfcal" else 6
    jc1, jl1, r1 = _blocks(name, loss)
    whole_ld, whole_64 = _whole(name, loss)
    pi = d.pt_idx.astype(int)
    x = np.random.default_rng(3).normal(size=9 * n_cam)
    owned_sum = np.zeros(d.n_pt, dtype=int)
    worst, refs, S_sum, g_sum, cost_sum = {}, [], 0.0, 0.0, 0.0
    ye_sum, yi_sum = 0.0, 0.0
    for r in range(world):
        prob, s = _solver(name, loss, shard=(r, world), schur_form=form, tree_sharding=tree)
        try:
            lay, n = prob.layout, prob.layout.cam_dof
            cols = sr.cam_cols(lay, n_cam, dc)
            rest = np.setdiff1d(np.arange(n), cols.ravel())
            info = s.info()
            hs = shc.host(name, world, r, tree)
            assert info["schur_form"] == form and info["tree_sharded"] == bool(hs["tree_sharded"]) and info["dist_top_columns"] == hs["top_columns"]
            owned = s.owned_landmarks()
            assert np.array_equal(owned, hs["owned"])
            owned_sum += owned
            sel = owned[pi]
            assert info["local_obs"] == int(sel.sum())
            # the shard's own linearisation: the single-rank handle's bits on its observations, zero elsewhere
            jc, jl = s.get_jacobian_blocks()
            res = s.get_residual().reshape(-1, 2)
            assert np.array_equal(jc[sel], jc1[sel]) and np.array_equal(jl[sel], jl1[sel]) and np.array_equal(res[sel], r1.reshape(-1, 2)[sel])
            assert not jc[~sel].any() and not jl[~sel].any() and not res[~sel].any()
            cost = s.compute_cost()
            s.assemble(LAM)
            S, gred = s.get_schur()
            S, gred = S.copy(), gred.copy()
            hinv, gl = s.get_landmark_blocks()
            ye, yi = s.schur_matvec(LAM, x)
            S2, g2 = s.get_schur()
        finally:
            s.close()
        lam_cams = shc.lambda_cameras(name, world, r, tree)
        ld, f64 = shc.rank_reference(d, jc, jl, res, LAM, owned, lam_cams)
        refs.append((ld, f64))
        S4 = sr.blocks_of(S, cols)
        ratios = {}
        ratios["S"], bad = sr.block_check(S4, ld, f64)
        assert not bad, (r, [(b, float(ratios["S"][b]), int(ld.P[b])) for b in bad[:8]])
        # camera pairs without an owned common landmark exactly zero, the diagonal of a camera that carries lambda and has
        # no owned observation exactly lambda I; S exactly symmetric; untouched columns: lambda on rank 0 only
        none = ld.P == 0
        lone = none & np.eye(n_cam, dtype=bool) & lam_cams[:, None]
        assert (S4[none & ~lone] == 0.0).all() and all(np.array_equal(S4[c, c], LAM * np.eye(dc)) for c in np.flatnonzero(np.diag(lone)))
        assert np.array_equal(S, S.T)
        off = S.copy(); off[rest, rest] = 0.0
        assert (S[rest, rest] == (LAM if r == 0 else 0.0)).all() and not off[rest].any() and not off[:, rest].any()
        ratios["gred"] = sr.vec_check(gred[cols], ld.gred, f64.gred, ld.gred_mag, ld.gred_terms)
        assert not gred[rest].any()
        if owned.any():                                                         # (an empty rank owns no landmark record)
            ratios["hinv"] = sr.vec_check(hinv[owned], ld.Hinv[owned], f64.Hinv[owned], ld.hinv_mag[owned], ld.k_l[owned])
            ratios["gl"] = sr.vec_check(gl[owned], ld.gl[owned], f64.gl[owned], ld.gl_mag[owned], ld.k_l[owned])
        # S x: the explicit tiles carry lambda as S does, the matrix-free operator on rank 0
        y_ld, mag = ld.matvec(x[cols]); y_64, _ = f64.matvec(x[cols])
        ratios["mv_explicit"] = sr.vec_check(ye[cols], y_ld, y_64, mag, ld.matvec_terms())
        mf = shc.rank_reference(d, jc, jl, res, LAM, owned, np.full(n_cam, r == 0), dense=False)
        y_ld, mag = mf[0].matvec(x[cols]); y_64, _ = mf[1].matvec(x[cols])
        ratios["mv_implicit"] = sr.vec_check(yi[cols], y_ld, y_64, mag, ld.matvec_terms())    # (the same structure: the same terms)
        for y in (ye, yi):
            assert np.array_equal(y[rest], (LAM if r == 0 else 0.0) * x[rest])
        ref_cost = shc.rank_cost(d, owned, shc.LOSSES[loss])
        ratios["cost"] = np.array([abs(cost - ref_cost) / ref_cost / 1e-12 if ref_cost > 0 else (0.0 if cost == 0.0 else np.inf)])
        # a second assembly on the same handle: the same bits unless a block adds atomically
        if sel.any():
            ci, pl_pi = d.cam_idx[sel], d.pt_idx[sel]
            pl = capi.pair_lists_queued(n_cam, d.n_pt, ci, pl_pi, 9) if form == 4 else capi.pair_lists(n_cam, d.n_pt, dc, ci, pl_pi)
            atomic = bool(len(pl["blocks"])) and bool((pl["blocks"][:, 3] & 1).any())
        else:
            atomic = False
        ratios["S_again"], bad2 = sr.block_check(sr.blocks_of(S2, cols), ld, f64)
        assert not bad2
        if not atomic:
            assert np.array_equal(S, S2) and np.array_equal(gred, g2)
        for k, v in _worst(ratios).items():
            assert v <= 1.0, (r, k, v)
        _merge(worst, ratios)
        S_sum = S_sum + S; g_sum = g_sum + gred; cost_sum += cost; ye_sum = ye_sum + ye; yi_sum = yi_sum + yi
    # the sum over the ranks against the whole problem, block by block, under the sum of the ranks' own bounds
    assert (owned_sum == 1).all()
    worst["S_sum"] = shc.sum_check(sr.blocks_of(S_sum, cols), whole_ld, refs)
    err = np.abs(np.asarray(g_sum[cols], dtype=sr.LD) - whole_ld.gred).max(axis=1).astype(np.float64)
    gb = lambda ld, f64: np.maximum(8.0 * np.abs(np.asarray(f64.gred, dtype=sr.LD) - ld.gred).max(axis=1).astype(np.float64), sr.gamma(ld.gred_terms) * ld.gred_mag)
    worst["gred_sum"] = sr._ratio(err, sum(gb(*p) for p in refs))
    whole_cost = shc.rank_cost(d, np.ones(d.n_pt, dtype=bool), shc.LOSSES[loss])
    worst["cost_sum"] = np.array([abs(cost_sum - whole_cost) / whole_cost / 1e-12])
    _report(f"partial {name} world {world} form {form} {loss} {'tree' if tree else 'range'}", worst)
    assert (S_sum[rest, rest] == LAM).all() and np.array_equal(ye_sum[rest], LAM * x[rest]) and np.array_equal(yi_sum[rest], LAM * x[rest])
    for k in ("S_sum", "gred_sum", "cost_sum"):
        assert sr.worst(worst[k])[0] <= 1.0, (k, sr.worst(worst[k]))


def _solve_ld(S, g):
    """x of S x = g in long double: Cholesky, two sweeps, one refinement step."""
    A = np.asarray(S, dtype=sr.LD)
    L = tr.chol_ld(A)
    n = len(g)

    def sweep(b):
        y = np.array(b, dtype=sr.LD)
        for j in range(n):
            y[j] = (y[j] - L[j, :j] @ y[:j]) / L[j, j]
        for j in reversed(range(n)):
            y[j] = (y[j] - L[j + 1:, j] @ y[j + 1:]) / L[j, j]
        return y
    x = sweep(g)
    return x + sweep(np.asarray(g, dtype=sr.LD) - A @ x)


@functools.lru_cache(maxsize=None)
def _solved(name, loss):
    """The whole problem's reference S, g_red (dense, camera-major columns) and its long double and numpy solves, once per case."""
    ld, f64 = _whole(name, loss)
    n_cam, dc = ld.n_cam, ld.dc
    ident = np.arange(n_cam * dc).reshape(n_cam, dc)
    S_ld = sr.dense_of(ld.S4, ident, n_cam * dc)
    S_64 = np.asarray(S_ld, dtype=np.float64)
    kappa = float(np.linalg.cond(S_64))
    assert kappa <= 1e8, kappa
    x_ld = _solve_ld(S_ld, ld.gred.ravel())
    x_np = np.linalg.solve(S_64, np.asarray(ld.gred, dtype=np.float64).ravel())
    return S_ld, S_64, x_ld, x_np, kappa, float(np.linalg.norm(S_64, 2))


@pytest.mark.parametrize("name,world,loss,tree", LOCKSTEP, ids=[f"{n}-w{w}-{l}-{'tree' if t else 'range'}" for n, w, l, t in LOCKSTEP])
def test_lockstep_solve_on_an_arrow(name, world, loss, tree):
    n_cam, lists, lam, mode, worlds = shc.structure(name)
    d = shc.problem(name)
    ld, f64 = _whole(name, loss)
    S_ld, S_64, x_ld, x_np, kappa, norm2 = _solved(name, loss)
    ranks = []
    try:
        for r in range(world):
            prob, s = _solver(name, loss, shard=(r, world), tree_sharding=tree)
            ranks.append(s)
        lay, nc = prob.layout, prob.layout.cam_dof
        cols = sr.cam_cols(lay, n_cam, 9)
        infos = [s.info() for s in ranks]
        hosts = [shc.host(name, world, r, tree) for r in range(world)]
        for i, hs in zip(infos, hosts):
            assert i["dist_top_columns"] == hs["top_columns"] == 1 and i["tree_sharded"] == bool(tree) == bool(hs["tree_sharded"])
        assert abs(sum(i["dist_local_fraction"] for i in infos) - 1.0) < 1e-9
        owned = np.stack([s.owned_landmarks() for s in ranks])
        assert (owned.sum(axis=0) == 1).all() and all(np.array_equal(owned[r], hosts[r]["owned"]) for r in range(world))
        GpuSchurComplementSolver.lockstep_solve(ranks, LAM)
        steps = [s.export_step()[0] for s in ranks]
        GpuSchurComplementSolver.lockstep_solve(ranks, LAM)
        again = [s.export_step()[0] for s in ranks]
    finally:
        for s in ranks:
            s.close()
    for r in range(1, world):                                       # the camera step is bit-identical on every rank
        assert np.array_equal(steps[r][:nc], steps[0][:nc])
    x = steps[0][cols].ravel()
    # backward error against the REFERENCE's S, forward error by the referee rule
    g = np.asarray(ld.gred, dtype=np.float64).ravel()
    res = np.asarray(S_ld @ np.asarray(x, dtype=sr.LD) - ld.gred.ravel(), dtype=np.float64)
    bwd = np.linalg.norm(res) / (norm2 * np.linalg.norm(x) + np.linalg.norm(g))
    nx = float(np.linalg.norm(np.asarray(x_ld, dtype=np.float64)))
    e_dev = float(np.linalg.norm(np.asarray(x - x_ld, dtype=np.float64))) / nx
    e_np = float(np.linalg.norm(np.asarray(x_np - x_ld, dtype=np.float64))) / nx
    floor = 8 * len(x) * sr.U * kappa
    # the landmark step of every owned landmark from its owner: the device's camera step through the reference's back-substitution
    dcam = steps[0][cols]
    dl_ld, dl_mag = ld.back_substitute(dcam); dl_64, _ = f64.back_substitute(dcam)
    pcols = lay.pt_col[:, None] + np.arange(3)[None]
    dl = np.zeros((d.n_pt, 3))
    for r in range(world):
        dl[owned[r]] = steps[r][pcols][owned[r]]
    ratios = dict(bwd=np.array([bwd / 1e-13]), fwd=np.array([e_dev / max(8.0 * e_np, floor)]),
                  dl=sr.vec_check(dl, dl_ld, dl_64, dl_mag, 2 * ld.k_l))
    # a second lockstep solve on the same handles: the same bits where no rank's assembly adds atomically
    atomic = False
    for r in range(world):
        sel = owned[r][d.pt_idx.astype(int)]
        if sel.any():
            pl = capi.pair_lists_queued(n_cam, d.n_pt, d.cam_idx[sel], d.pt_idx[sel], 9)
            atomic = atomic or (bool(len(pl["blocks"])) and bool((pl["blocks"][:, 3] & 1).any()))
    _report(f"lockstep {name} world {world} {loss} {'tree' if tree else 'range'}" + (" (atomic)" if atomic else "")
            + f" kappa {kappa:.2g} e_np {e_np:.2g} e_dev {e_dev:.2g}", ratios)
    assert tr.referee(e_dev, e_np, floor), (e_dev, e_np, floor)
    for k, v in _worst(ratios).items():
        assert v <= 1.0, (k, v)
    if not atomic:
        for r in range(world):
            assert np.array_equal(again[r], steps[r])
