"""The tile Cholesky (TilePlan: k_potrf_inv_mf, the panel / update GEMMs, k_factor_flow, the sweeps, the selected inverse) on
matrices the test chooses, through the test hook apexgpu_debug_tiles_* (capi.TileCholesky), against the references and
bounds of tests/tile_ref.py:
  - backward bounds (Higham Thm 10.3 / 10.4, the Linv right residual, the matvec bound) with ratio measured / bound <= 1;
  - forward errors against exact factors (L0, by construction) or long double references, by the referee rule
    e_gpu <= max(8 e_np, floor) with e_np numpy / scipy fp64's distance from the same reference;
  - bits: repeated runs, the schedule forms that claim the same per-element order, NaN in the fill tiles.
Every case prints one TILECHOL line with its worst ratios."""
import numpy as np
import pytest

import tile_ref as tr

pytestmark = pytest.mark.gpu

NB = tr.NB


def _dev(present, **opts):
    from apex_solver_amd import capi

    return capi.TileCholesky(present, **opts)


def _refs(A, pat, L0=None, z_cols="all"):
    """Reference L (exact L0 or long double), its diagonal inverses, numpy fp64's factor, the reference Z."""
    if L0 is not None:
        Lref = {k: np.asarray(v, dtype=tr.LD) for k, v in L0.items()}
        Liref = {K: tr.tri_inv_ld(L0[(K, K)]) for K in range(pat.shape[0])} if z_cols else None
    else:
        Lref, Liref = tr.tile_cholesky(A, pat)
    Lnp, Linp = tr.tile_cholesky(A, pat, ld=False)
    return Lref, Liref, Lnp, Linp


def _run(dev, A, n_valid=None, add_diag=0.0, fill_mode=0, z=True, rhs=None):
    dev.set(tr.touched_array(A, dev), n_valid=n_valid, add_diag=add_diag, fill_mode=fill_mode)
    f = dev.factor()
    out = dict(failed=f)
    if f == 0:
        out["L"] = dev.get("L")
        out["Linv"] = dev.get("Linv")
        if rhs is not None:
            out["x"] = dev.solve(rhs)
        if z:
            out["Z"] = dev.get("Z")
    return out


def check_case(label, dev, pat, A, L0=None, z_cols="all", n_rhs=2, seed=0, repeat=True, bound_keys=None, linv_cols=None, kappa=None):
    """Factor / Linv / solve / Z / matvec checks of one SPD case; returns the run's arrays."""
    nt = pat.shape[0]
    keys = tr.filled_pattern(pat)
    rng = np.random.default_rng(seed)
    b = rng.standard_normal((n_rhs, nt * NB))
    # matvec on the unfactored tiles
    dev.set(tr.touched_array(A, dev))
    xv = rng.standard_normal(nt * NB)
    r_mv = tr.matvec_ratio(A, xv, dev.matvec(xv), nt)
    run = _run(dev, A, z=bool(z_cols), rhs=b)
    assert run["failed"] == 0, (label, run["failed"])
    Lh = tr.from_slots(run["L"], dev, keys)
    assert all(np.isfinite(t).all() for t in Lh.values()), label
    Lref, Liref, Lnp, Linp = _refs(A, pat, L0, z_cols)
    # factor: backward bound, forward error
    r_f = tr.factor_ratio(A, Lh, pat, L0=L0, keys=bound_keys, X=run["Linv"])
    dense_ok = nt * NB <= 2304
    Ad = tr.dense_of(A, nt) if dense_ok else None
    if dense_ok:   # numpy's own dense factor (LAPACK), as the rule says
        Lnp_d = np.linalg.cholesky(Ad)
        Lnp_e = {(I, J): Lnp_d[I * NB:(I + 1) * NB, J * NB:(J + 1) * NB] for I, J in keys}
    else:
        Lnp_e = Lnp
    e_l, e_lnp = tr.tile_err(Lh, Lref), tr.tile_err(Lnp_e, Lref)
    # The floor: 8 n u, times kappa(A).  On the exact constructions numpy often rounds nowhere (dyadic entries of few bits:
    # its sums are exact, and LAPACK's correctly rounded sqrt / division return the exact L0), so e_np is 0 or tiny while a
    # backward-stable factor built on rsq + Newton differs in the last bit; such a factor and the solves with it are off by
    # up to the first-order perturbation bound ~ kappa(A) x backward error (Higham Thm 7.2, 10.4).  The backward bounds
    # above are the sharp checks; the forward comparisons guard the well-conditioned cases.
    if kappa is None:
        kappa = float(np.linalg.cond(Ad)) if nt * NB <= 576 else 1.0
    floor = 8 * nt * NB * tr.U * max(1.0, kappa)
    # Linv: right residual; its 16 x 16 blocks above the diagonal and the upper triangles of its diagonal blocks are zero
    r_i = 0.0
    for K in (range(nt) if linv_cols is None else linv_cols):
        X = run["Linv"][K]
        assert not np.triu(X, 1).any(), (label, K)
        r_i = max(r_i, tr.linv_ratio(Lh[(K, K)], X))
    # solves
    r_s, e_x, e_xnp = 0.0, 0.0, 0.0
    Liref_x = Liref if Liref is not None else {K: tr.tri_inv_ld(Lref[(K, K)]) for K in range(nt)}
    for k in range(n_rhs):
        x = run["x"][k]
        r_s = max(r_s, tr.solve_ratio(A, Lh, x, b[k], nt))
        xr = tr.refined_solve(A, Lref, Liref_x, b[k], pat)
        e_x = max(e_x, tr.vec_err(x, xr))
        e_xnp = max(e_xnp, tr.vec_err(tr.np_solve(Lnp, Linp, b[k], pat), xr))
    # Z on every tile of the pattern of the wanted columns
    e_z = e_znp = 0.0
    if z_cols:
        cw = None if z_cols == "all" else z_cols
        Zref = tr.selected_inverse(Lref, Liref_x, pat, cols_wanted=cw)
        if dense_ok:   # numpy's dense inverse
            Zd = np.linalg.inv(Ad)
            Znp = {(I, J): Zd[I * NB:(I + 1) * NB, J * NB:(J + 1) * NB] for I, J in Zref}
        else:          # (too large for a dense inverse: the same recurrence in fp64 on numpy's factor)
            Znp = tr.selected_inverse(Lnp, Linp, pat, dtype=np.float64, cols_wanted=cw)
        Zh = tr.from_slots(run["Z"], dev, list(Zref.keys()))
        e_z, e_znp = tr.tile_err(Zh, Zref), tr.tile_err(Znp, Zref)
    print(f"TILECHOL {label} (kappa {kappa:.1e}): factor {r_f:.3g} Linv {r_i:.3g} solve {r_s:.3g} matvec {r_mv:.3g} | e_L {e_l:.2e} (np {e_lnp:.2e}) "
          f"e_x {e_x:.2e} (np {e_xnp:.2e}) e_Z {e_z:.2e} (np {e_znp:.2e})")
    assert r_f <= 1.0 and r_i <= 1.0 and r_s <= 1.0 and r_mv <= 1.0, (label, r_f, r_i, r_s, r_mv)
    assert tr.referee(e_l, e_lnp, floor), (label, e_l, e_lnp, kappa)
    assert tr.referee(e_x, e_xnp, floor), (label, e_x, e_xnp)
    if z_cols:
        assert tr.referee(e_z, e_znp, floor), (label, e_z, e_znp)
    if repeat:   # the same bits again on the same handle (x too where the sweeps run level by level)
        again = _run(dev, A, z=bool(z_cols), rhs=b)
        for k in ("L", "Linv") + (("Z",) if z_cols else ()):
            assert np.array_equal(again[k], run[k]), (label, k)
        x_bits = not dev_opts(dev).get("tri_dataflow", 1)
        if x_bits:
            assert np.array_equal(again["x"], run["x"]), label
        else:
            assert all(tr.solve_ratio(A, Lh, again["x"][k], b[k], nt) <= 1.0 for k in range(n_rhs)), label
    return run


def dev_opts(dev):
    return getattr(dev, "_test_opts", {})


def _mk(present, **opts):
    d = _dev(present, **opts)
    d._test_opts = opts
    return d


# ---------------------------------------------------------------------------------------------------------------------


def test_single_tile_pivot_positions_and_conditioning():
    """nt = 1: one small pivot at rows around the pivot pairs, the 16-row blocks, the last block step and Linv's last row,
    kappa 1e1 .. 1e12 (exact factor, q = 20)."""
    pat = tr.dense(1)
    rows = [0, 1, 14, 15, 16, 17, 127, 142, 143]
    exps = [-2, -5, -8, -11, -14, -17, -20, -20, -12]
    with _mk(pat) as dev:
        for i, (r, e) in enumerate(zip(rows, exps)):
            A, L0 = tr.exact_case(pat, np.random.default_rng(100 + i), q=20, pivots={r: e})
            check_case(f"nt1 pivot row {r} 2^{e}", dev, pat, A, L0=L0, seed=i)


def test_single_tile_graded():
    """D A D with D = 2^e, e over +-200: rsq + Newton far from 1; the factor is exactly D L0."""
    pat = tr.dense(1)
    A, L0 = tr.exact_case(pat, np.random.default_rng(11), diag_exp=(-6, 6))
    e = np.random.default_rng(12).integers(-200, 201, size=NB)
    As, Ls = tr.scale_rows(A, e), tr.scale_rows(L0, e, cols=False)
    with _mk(pat) as dev:
        # (the factor's rounding does not see a diagonal scaling by powers of two: the floor takes kappa of the unscaled A)
        check_case("nt1 graded 2^+-200", dev, pat, As, L0=Ls, kappa=float(np.linalg.cond(A[(0, 0)])))


def test_block_diagonal_96_tiles():
    """96 different diagonal tiles: one potrf launch of 96 workgroups (the helper waves' LDS counter at full occupancy)."""
    pat = tr.block_diagonal(96)
    A, L0 = tr.exact_case(pat, np.random.default_rng(21), q=16, diag_exp=(-6, 5))
    with _mk(pat, tri_dataflow=0) as dev:
        check_case("blockdiag 96", dev, pat, A, L0=L0, z_cols=[0, 17, 47, 95], n_rhs=2)


def test_arrow_panel_batches_give_the_same_bits():
    """56 vs 57 leaves, border last, factor_flow 0: the leaves' panel solves go to the small-batch kernel (56) or the large
    TRI kernel (57).  The shared leaves' panel tiles must be bit-identical (the same per-element k order in every form)."""
    rng = np.random.default_rng(31)
    p57 = tr.arrow(57)
    M, q = tr.exact_factor(p57, rng, q=14, diag_exp=(-4, 4))
    p56 = tr.arrow(56)
    M56 = {}
    for (I, J), t in M.items():
        if I == 56 or J == 56:
            continue
        M56[(56 if I == 57 else I, 56 if J == 57 else J)] = t
    A57 = {k: v.astype(np.float64) * 2.0 ** (-2 * q) for k, v in tr.product_int(M, p57).items()}
    A56 = {k: v.astype(np.float64) * 2.0 ** (-2 * q) for k, v in tr.product_int(M56, p56).items()}
    L57 = tr.to_float(M, q)
    with _mk(p56, factor_flow=0) as d56, _mk(p57, factor_flow=0) as d57:
        r56 = _run(d56, A56, z=False)
        assert r56["failed"] == 0
        r57 = check_case("arrow 57 (large TRI)", d57, p57, A57, L0=L57, z_cols=[0, 30, 56, 57], linv_cols=[0, 30, 56, 57])
        for j in range(56):
            assert np.array_equal(r56["L"][d56.slot[56, j]], r57["L"][d57.slot[57, j]]), j
            assert np.array_equal(r56["L"][d56.slot[j, j]], r57["L"][d57.slot[j, j]]), j
            assert np.array_equal(r56["Linv"][j], r57["Linv"][j]), j
        L56 = tr.from_slots(r56["L"], d56, tr.filled_pattern(p56))
        assert tr.factor_ratio(A56, L56, p56, L0=tr.to_float(M56, q), X=r56["Linv"]) <= 1.0


@pytest.mark.parametrize("shape", ["band16", "dense8"])
def test_deep_and_dense_trees_factor_flow_forms_agree(shape):
    """A deep elimination tree (band) and a dense one; the top taken by k_factor_flow or not: factor_flow 0 / default / 64
    give identical bits."""
    pat = tr.band(16) if shape == "band16" else tr.dense(8)
    A, L0 = tr.exact_case(pat, np.random.default_rng(41), q=14, diag_exp=(-4, 4))
    outs = []
    for ff in (0, -1, 64):
        with _mk(pat, factor_flow=ff) as dev:
            if ff == -1:
                run = check_case(f"{shape} factor_flow default (units {dev.flow_units})", dev, pat, A, L0=L0,
                                 z_cols="all" if shape == "band16" else [0, 6, 7], linv_cols=None)
            else:
                run = _run(dev, A, z=False)
                assert run["failed"] == 0
            if ff == 64:
                assert dev.flow_units > 0, "factor_flow 64 put nothing into the dataflow launch"
            outs.append(run)
    for o in outs[1:]:
        assert np.array_equal(o["L"], outs[0]["L"]) and np.array_equal(o["Linv"], outs[0]["Linv"])


FILL = {"grid4x4": lambda: tr.grid(4, 4), "star3x3": lambda: tr.star_of_chains(3, 3), "nd2": lambda: tr.nested_dissection(2)}


@pytest.mark.parametrize("name", list(FILL))
def test_fill_patterns_never_read_their_fill_tiles(name):
    """Fill tiles set to quiet NaN before the factorisation (the plan flags their first writers, which do not read them):
    the same bits as with the fill tiles cleared, all finite, within the bounds; a subset of schedule switches agrees."""
    pat = FILL[name]()
    assert tr.has_fill(pat)
    A = tr.dominant_case(pat, np.random.default_rng(51))
    keys = tr.filled_pattern(pat)
    with _mk(pat) as dev:
        assert dev.first_writers_flagged and dev.n_slots > dev.n_touched
        run0 = check_case(f"fill {name}", dev, pat, A, z_cols="all" if name != "grid4x4" else None,
                          bound_keys=None if name != "grid4x4" else keys[:: max(1, len(keys) // 24)])
        run1 = _run(dev, A, fill_mode=1, z=False)
        assert run1["failed"] == 0
        assert np.isfinite(run1["L"]).all() and np.isfinite(run1["Linv"]).all()
        assert np.array_equal(run1["L"], run0["L"]) and np.array_equal(run1["Linv"], run0["Linv"])
    if name == "nd2":
        return
    for opts in (dict(two_side=0), dict(two_side=2), dict(split_u1=0), dict(update_overlap=0), dict(graphs=0), dict(factor_flow=0)):
        with _mk(pat, **opts) as dev:
            fm = 1 if dev.first_writers_flagged else 0
            r = _run(dev, A, fill_mode=fm, z=False)
            assert r["failed"] == 0
            assert np.array_equal(r["L"], run0["L"]) and np.array_equal(r["Linv"], run0["Linv"]), opts


@pytest.mark.parametrize("shape", ["grid3x4", "band48"])
def test_device_plan_is_the_host_value(shape):
    """The plan TilePlan::build makes on the device's tile addresses against the host value built with no device on stand-in
    addresses (plan_lists.h; apexgpu_debug_plan_lists): the slot map, the slot / touched / level-group counts, the first-writer
    verdict, the dataflow units and groups.  grid(3, 4): 12 tiles with fill; band(48, 3): 48 level groups, no fill.  Then one
    factorisation + solve on that plan (the exact-reference cases of this file run on plans built the same way)."""
    from apex_solver_amd import capi

    pat = tr.grid(3, 4) if shape == "grid3x4" else tr.band(48, 3)
    nt = pat.shape[0]
    assert tr.has_fill(pat) == (shape == "grid3x4")
    sc = capi.plan_lists(pat, "scalars")[0]
    slot = np.full((nt, nt), -1, dtype=np.int32)
    rows = capi.plan_lists(pat, "slots")
    slot[rows[:, 0], rows[:, 1]] = rows[:, 2]
    with _mk(pat) as dev:
        assert np.array_equal(dev.slot, slot)
        assert (dev.n_slots, dev.n_touched, dev.levels) == (int(sc[3]), int(sc[4]), int(sc[0]))
        assert dev.first_writers_flagged == bool(sc[9])
        assert dev.flow_units == int(sc[13] + sc[17]) and dev.flow_groups == int((sc[11] - sc[10]) + (sc[15] - sc[14]))
        assert dev.flow_units == len(capi.plan_lists(pat, "units"))
        A = tr.dominant_case(pat, np.random.default_rng(61))
        if shape == "grid3x4":
            check_case("host-value plan grid3x4", dev, pat, A, z_cols=None)
        else:
            run = _run(dev, A, z=False, rhs=np.random.default_rng(62).standard_normal((1, nt * NB)))
            assert run["failed"] == 0 and np.isfinite(run["L"]).all() and np.isfinite(run["x"]).all()
            Lh = tr.from_slots(run["L"], dev, tr.filled_pattern(pat))
            assert tr.factor_ratio(A, Lh, pat) <= 1.0


_SCHED_ON = dict(two_side=2, update_overlap=1, split_u1=1, flood_gate=2)
_sched_case = {}


def _schedule_case():
    """grid(4, 4) (fill, 16 level groups), its matrix and the bits of the fully serial schedule: computed once."""
    if not _sched_case:
        pat = tr.grid(4, 4)
        A = tr.dominant_case(pat, np.random.default_rng(51))
        with _mk(pat, update_overlap=0, flood_gate=0, two_side=0, factor_flow=0, graphs=0) as dev:
            ref = _run(dev, A, z=False)
        assert ref["failed"] == 0
        _sched_case.update(pat=pat, A=A, ref=ref)
    return _sched_case["pat"], _sched_case["A"], _sched_case["ref"]


@pytest.mark.parametrize("factor_flow", [0, 64])
@pytest.mark.parametrize("graphs", [0, 1])
def test_issued_schedule_gives_the_serial_bits(graphs, factor_flow):
    """Every kind of call of the factorisation's schedule (factor_schedule.h) played by TilePlan::issue, directly and through a
    captured graph.  On grid(4, 4) with every switch on and gates from two tasks up, the level launches use all four streams,
    event records and waits, gates on both side streams and the clear of the arrival counters (factor_flow 0); factor_flow 64
    takes all groups into the dataflow launch behind the clear of its version counters -- read off
    apexgpu_debug_schedule_ops below.  L and Linv carry the bits of the serial schedule (main stream only, no gate, no
    graph), and a second factorisation on the same handle (the graph's replay) gives them again."""
    from apex_solver_amd import capi

    pat, A, ref = _schedule_case()
    rows = capi.schedule_ops(pat, two_side=2, overlap=1, split_u1=1, flood_gate=2, factor_flow=factor_flow)
    kinds, launches = set(rows[:, 0].tolist()), rows[rows[:, 0] == 0]
    if factor_flow == 0:
        assert kinds == {0, 1, 2, 3, 4} and set(launches[:, 1].tolist()) == {0, 1, 2, 3} and set(launches[:, 3].tolist()) == {0, 1, 2}
        assert set(rows[rows[:, 0] == 3][:, 1].tolist()) == {1, 2}
    else:
        assert kinds == {0, 4, 5} and launches[:, 3].tolist() == [3]
    with _mk(pat, graphs=graphs, factor_flow=factor_flow, **_SCHED_ON) as dev:
        assert (dev.flow_units > 0) == (factor_flow != 0)
        for again in (0, 1):
            run = _run(dev, A, z=False)
            assert run["failed"] == 0
            for k in ("L", "Linv"):
                assert np.array_equal(run[k], ref[k]), (k, graphs, factor_flow, again)


def test_padding_rows_are_identity():
    """The last tile with 37 padding rows: add_diag makes them identity; x is 0 there; the rest meets the bounds."""
    pat = tr.band(3)
    n_pad = 3 * NB
    nv = n_pad - 37
    M, q = tr.exact_factor(pat, np.random.default_rng(61), q=14, diag_exp=(-3, 3))
    t = M[(2, 2)]
    t[NB - 37:, :] = 0
    t[:, NB - 37:] = 0
    M[(2, 1)][NB - 37:, :] = 0
    A = {k: v.astype(np.float64) * 2.0 ** (-2 * q) for k, v in tr.product_int(M, pat).items()}   # padding rows / columns 0
    L0 = tr.to_float(M, q)
    idx = np.arange(NB - 37, NB)
    L0[(2, 2)][idx, idx] = 1.0
    A1 = {k: v.copy() for k, v in A.items()}
    A1[(2, 2)][idx, idx] = 1.0
    with _mk(pat, tri_dataflow=0) as dev:
        b = np.random.default_rng(62).standard_normal((2, n_pad))
        b[:, nv:] = 0
        dev.set(tr.touched_array(A, dev), n_valid=nv)
        assert dev.factor() == 0
        L = tr.from_slots(dev.get("L"), dev, tr.filled_pattern(pat))
        assert np.array_equal(L[(2, 2)][NB - 37:, NB - 37:], np.eye(37)) and not L[(2, 2)][NB - 37:, :NB - 37].any()
        assert tr.factor_ratio(A1, L, pat, L0=L0, X=dev.get("Linv")) <= 1.0
        x = dev.solve(b)
        assert not x[:, nv:].any()
        for k in range(2):
            assert tr.solve_ratio(A1, L, x[k], b[k], 3) <= 1.0


def test_selected_inverse_is_current_exactly_until_the_tiles_are_written():
    """grid(4, 4): 16 tile columns, fill, several level groups, Z_sr^T products.  Z read twice is computed once; every write of
    the tiles the handle can reach -- set, a factorisation that fails on a non-positive pivot, pcg -- voids it (InvalidState);
    a fresh factor of the same tiles recomputes it to the same bits."""
    from apex_solver_amd.capi import LinAlgError

    pat = tr.grid(4, 4)
    A = tr.dominant_case(pat, np.random.default_rng(101))
    bad = {k: v.copy() for k, v in A.items()}
    bad[(0, 0)][0, 0] = -A[(0, 0)][0, 0]   # the first pivot of tile column 0
    with _mk(pat) as dev:
        T = tr.touched_array(A, dev)

        def refactor():
            dev.set(T)
            assert dev.factor() == 0
            z = dev.get("Z")
            assert dev.z_recomputed
            return z

        def void():
            with pytest.raises(LinAlgError) as e:
                dev.get("Z")
            assert e.value.kind == "InvalidState"

        Z0 = refactor()
        assert dev.levels > 2 and tr.has_fill(pat)
        Z1 = dev.get("Z")
        assert not dev.z_recomputed and np.array_equal(Z1, Z0)
        dev.set(T)
        void()
        assert np.array_equal(refactor(), Z0)
        dev.set(tr.touched_array(bad, dev))
        assert dev.factor() == 1
        void()
        assert np.array_equal(refactor(), Z0)
        dev.pcg(np.ones(dev.n_pad), 1, 1e-8)
        void()
        assert np.array_equal(refactor(), Z0)


@pytest.mark.parametrize("factor_flow", [0, -1])
def test_indefinite_pivot_is_reported_in_its_column(factor_flow):
    """One clearly negative pivot (exactly <= -1e-3 of its diagonal) in tile column K of a chain: failed_at == K + 1 (the
    columns after K see NaN but run later).  After set() with add_diag = reg the factor succeeds within the bounds of
    A + reg I."""
    pat = tr.band(3)
    A, L0 = tr.exact_case(pat, np.random.default_rng(71), q=14, diag_exp=(-2, 2))
    with _mk(pat, factor_flow=factor_flow) as dev:
        for g in (0, 15, NB + 16, NB + 143, 2 * NB + 1, 2 * NB + 142):
            K, r = divmod(g, NB)
            B = {k: v.copy() for k, v in A.items()}
            d = L0[(K, K)][r, r] ** 2
            delta = d + 2.0 ** np.ceil(np.log2(2e-3 * A[(K, K)][r, r]))   # pivot = d - delta <= -1e-3 A_rr, exactly
            B[(K, K)][r, r] -= delta
            dev.set(tr.touched_array(B, dev))
            assert dev.factor() == K + 1, (g, factor_flow)
            reg = 2.0 * delta
            Breg = {k: v.copy() for k, v in B.items()}
            for J in range(3):
                Breg[(J, J)][np.arange(NB), np.arange(NB)] += reg
            dev.set(tr.touched_array(B, dev), add_diag=reg)
            assert dev.factor() == 0, g
            L = tr.from_slots(dev.get("L"), dev, tr.filled_pattern(pat))
            assert tr.factor_ratio(Breg, L, pat, X=dev.get("Linv")) <= 1.0, g


def test_nan_entry_is_reported_as_failed():
    """A NaN in one entry of the lower triangle (an off-diagonal tile, or a diagonal tile below its diagonal): the
    factorisation reports a failed column, never a silent finite L."""
    pat = tr.band(3)
    A, _ = tr.exact_case(pat, np.random.default_rng(81), q=14)
    with _mk(pat) as dev:
        for key, (i, j) in (((1, 0), (5, 140)), ((2, 2), (100, 3)), ((0, 0), (17, 16)), ((2, 1), (143, 0))):
            B = {k: v.copy() for k, v in A.items()}
            B[key][i, j] = np.nan
            if key[0] == key[1]:
                B[key][j, i] = np.nan
            dev.set(tr.touched_array(B, dev))
            f = dev.factor()
            assert f != 0, key
            assert key[1] + 1 <= f <= 3, (key, f)


def test_tiny_but_positive_pivot_is_not_a_failure():
    """SPD with one pivot 1e-8 of its row's diagonal (exact L0): not reported as failed; the bounds hold."""
    pat = tr.band(2)
    g = NB + 77
    A, L0 = tr.exact_case(pat, np.random.default_rng(91), q=20, pivots={g: -15})
    rel = L0[(1, 1)][77, 77] ** 2 / A[(1, 1)][77, 77]
    assert 1e-9 < rel < 1e-7, rel
    with _mk(pat) as dev:
        check_case("tiny pivot 1e-8", dev, pat, A, L0=L0)
