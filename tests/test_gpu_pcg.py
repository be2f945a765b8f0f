"""The device conjugate-gradient loop of the explicit Schur variants (TilePcg::solve behind TilePlan::pcg, csrc/tile_pcg.hip; csrc/pcg_kernels.hip:
k_pcg_init, k_sym_tile_products, k_sym_tile_gather, k_pcg_step1, k_pcg_step2, k_pcg_close_iteration; csrc/pcg_loop.h: the host
loop that reads the scalars one iteration behind and enqueues the next iteration on speculation) on systems the test chooses, through the hook apexgpu_debug_tiles_pcg
(capi.TileCholesky.pcg), against the long double restatement of the reference's loop (tests/pcg_ref.py):
  - every iterate x_k (the loop capped at k), by the referee rule e_gpu <= max(8 e_np, 8 n u max(1, kappa_J)) with e_np numpy
    fp64's distance from the same long double iterate, and the iteration count, exactly;
  - bits: a cap at, one past, two past and far past the converged count return the same x, count and device scalars -- the
    speculative iteration behind a met termination test changes nothing;
  - finite termination in r + 1 iterations on a matrix with r + 1 distinct preconditioned eigenvalues;
  - the three absolute exits (p.Ap, the residual, rz_old), a NaN matrix entry, the preconditioner's cut-off, padding rows,
    and sizes at which the strided reductions of k_pcg_step1 / k_pcg_step2 take a second trip.
The margins that make the exact counts safe are asserted on the CPU (tests/test_pcg_ref_host.py).  Every case prints PCGCASE
lines with its measured numbers (profiles/pcg_tests.txt keeps those of one run)."""
import numpy as np
import pytest

import pcg_ref as pr
import tile_ref as tr

pytestmark = pytest.mark.gpu

NB = tr.NB


def _dev(c):
    from apex_solver_amd import capi

    dev = capi.TileCholesky(c.pat)
    dev.set(tr.touched_array(c.A, dev), n_valid=c.n_valid, fill_mode=c.fill_mode)
    return dev


def _refs(c, cap=5000):
    return c.run(cap, pr.LD, keep_x=True), c.run(cap, np.float64, keep_x=True)


def check_iterates(c, dev, caps, ld, f64, floor=None):
    """The loop capped at every k of caps: the count min(k, k_conv), x against the long double x_k, padding rows exactly 0."""
    floor = c.floor() if floor is None else floor
    for k in dict.fromkeys(caps):
        x, it, sc = dev.pcg(c.b, k, c.tol)
        want = min(k, ld.iters)
        e_gpu = e_np = 0.0
        if want > 0 and it == want:
            e_gpu, e_np = tr.vec_err(x[:c.n], ld.xs[it - 1]), tr.vec_err(f64.xs[it - 1], ld.xs[it - 1])
        print(f"PCGCASE {c.label} n {c.n} cap {k}: iterations {it} (reference {want}) e_gpu {e_gpu:.2e} e_np {e_np:.2e} floor {floor:.2e} "
              f"scal rz_old {sc[0]:.3e} pAp {sc[1]:.3e} rr {sc[2]:.3e} rz {sc[3]:.3e} frozen {sc[4]:g}")
        assert it == want, (c.label, k, it, want)
        assert not x[c.n:].any(), (c.label, k)
        if want == 0:
            assert not x.any(), (c.label, k)
        else:
            assert np.isfinite(x).all() and tr.referee(e_gpu, e_np, floor), (c.label, k, e_gpu, e_np, floor)


def _bits(out):
    x, it, sc = out
    return x.tobytes(), it, sc.tobytes()


def check_speculation_bits(c, dev, k_conv):
    """Caps at, one past, two past and far past the converged count, and a repeat: the same bits of x, the same count, the same
    five scalars; below the count, the same cap twice."""
    runs = {k: dev.pcg(c.b, k, c.tol) for k in (k_conv, k_conv + 1, k_conv + 2, 5000)}
    again = dev.pcg(c.b, 5000, c.tol)
    first = runs[k_conv]
    assert first[1] == k_conv, (c.label, first[1], k_conv)
    same = {k: _bits(v) == _bits(first) for k, v in runs.items()}
    print(f"PCGCASE {c.label} bits: caps {sorted(runs)} equal to cap {k_conv}: {same}, repeat {_bits(again) == _bits(first)}, "
          f"scal {first[2].tolist()}")
    assert all(same.values()) and _bits(again) == _bits(first), (c.label, same)
    if k_conv > 2:
        a, b = dev.pcg(c.b, k_conv - 2, c.tol), dev.pcg(c.b, k_conv - 2, c.tol)
        assert _bits(a) == _bits(b) and a[1] == k_conv - 2, c.label


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", list(pr.ITERATE))
def test_every_iterate_and_the_speculation_bits(label):
    """Every iterate and the speculation bits on band(6), arrow(5), dense(3) and nested_dissection(2) with NaN in its fill tiles (PCG reads the unfactored
    tiles: a fill tile is never one of them)."""
    c = pr.case(label)
    ld, f64 = _refs(c)
    assert ld.iters == pr.K_CONV
    with _dev(c) as dev:
        check_iterates(c, dev, (0, 1, 2, 3, 5, ld.iters), ld, f64)
        check_speculation_bits(c, dev, ld.iters)


@pytest.mark.parametrize("r", [1, 3, 7])
def test_finite_termination_after_r_plus_one_iterations(r):
    c = pr.case(f"lowrank_r{r}")
    ld, f64 = _refs(c)
    assert ld.iters == r + 1
    with _dev(c) as dev:
        check_iterates(c, dev, (1, r, r + 1, 5000), ld, f64)
        check_speculation_bits(c, dev, r + 1)


def test_diagonal_matrix_one_iteration_exact_bits():
    """Every operation of the first iteration is exact on this matrix (pcg_ref.diagonal_case: dyadic d, small integer b, sums of
    exact terms that stay exact in any order), so alpha = 1 and x = b / d to the last bit -- numpy fp64 has no error either
    (tests/test_pcg_ref_host.py)."""
    c = pr.case("diagonal")
    with _dev(c) as dev:
        x, it, sc = dev.pcg(c.b, 5000, c.tol)
    want = c.b / pr.tile_diag(c.A, c.nt)
    print(f"PCGCASE diagonal: iterations {it} entries off {int((x != want).sum())} scal {sc.tolist()}")
    assert it == 1 and np.array_equal(x, want)
    # frozen by the residual test with r = 0 exactly; rz_old keeps the start's r.z, which equals p.Ap here
    assert sc[4] == 1.0 and sc[0] == sc[1] and sc[2] == 0.0


def test_absolute_threshold_exits():
    """The absolute thresholds on one dominant system: a zero right-hand side, the p.Ap exit (not counted, x untouched), the residual exit after one
    iteration below an absolute abs_tol -- and nothing frozen or non-finite survives in the scalars for the next solve."""
    base = pr.threshold_base()
    zero, pap, tiny = (pr.case(f"dense3_thresholds_{k}") for k in pr.THRESHOLDS)
    with _dev(base) as dev, _dev(base) as fresh:
        x, it, sc = dev.pcg(zero.b, 5000, zero.tol)
        print(f"PCGCASE {zero.label}: iterations {it} scal {sc.tolist()}")
        assert it == 0 and not x.any() and np.isfinite(sc).all()
        after, ref = dev.pcg(base.b, 5000, base.tol), fresh.pcg(base.b, 5000, base.tol)
        assert ref[1] == pr.K_CONV and _bits(after) == _bits(ref)
        x, it, sc = dev.pcg(pap.b, 5000, pap.tol)
        print(f"PCGCASE {pap.label}: iterations {it} scal {sc.tolist()}")
        assert it == 0 and not x.any() and abs(sc[1]) < pr.TINY / 8
        assert _bits(dev.pcg(base.b, 5000, base.tol)) == _bits(ref)
        ld, f64 = _refs(tiny)
        assert (ld.iters, ld.exit) == (1, "residual")
        check_iterates(tiny, dev, (5000, 1), ld, f64)


def test_rz_old_exit():
    """explicit_schur.rs:741-743: rz_old = 2^-103 (10.1 x below 1e-30) while p.Ap = 8.6e-30 (8.6 x above) -- the right-hand side
    is the top eigenvector of the Jacobi-scaled operator, whose Rayleigh quotient 87.2 separates the two (pcg_ref.rz_old_case;
    the margins are asserted in tests/test_pcg_ref_host.py).  tol = 0: only this exit can end the loop; it counts."""
    c = pr.case("rz_old_exit")
    ld, f64 = _refs(c)
    assert (ld.iters, ld.exit) == (1, "rz_old")
    with _dev(c) as dev:
        check_iterates(c, dev, (5000, 1, 2), ld, f64)
        x, it, sc = dev.pcg(c.b, 5000, c.tol)
        assert sc[4] == 1.0 and abs(sc[0]) < pr.TINY / 8 and abs(sc[1]) > 8 * pr.TINY


def test_nan_entry_ends_by_the_cap():
    c = pr.case("dense3")
    A = dict(c.A)
    t = A[(2, 1)].copy()
    t[17, 40] = np.nan
    A[(2, 1)] = t
    bad = pr.Case("dense3_nan", c.pat, A, c.b, tol=c.tol)
    with _dev(bad) as dev:
        x, it, sc = dev.pcg(bad.b, 8, bad.tol)
        print(f"PCGCASE dense3_nan: iterations {it} finite entries {int(np.isfinite(x).sum())} scal {sc.tolist()}")
        assert it == 8 and not np.isfinite(x).all() and sc[4] == 0.0


def test_preconditioner_cutoff():
    """A third of the diagonal is 9.3e-16 <= 1e-12; those rows are preconditioned with 1.  kappa_J of the matrix as the
    reference preconditions it is ~1e17, so the referee rule's usual floor 8 n u kappa_J is 4.6e4 and could not fail for a
    relative error.  The rule is therefore applied with the floor of a perfectly conditioned system, 8 n u: the sensitivity
    of iterate k to rounding is what numpy fp64's own distance e_np from the long double iterate samples (it runs the same
    recurrence on the same matrix), so e_gpu <= max(8 e_np, 8 n u) holds the device to the rule's factor 8 of that, at
    every cap -- a stricter statement than the one with kappa_J, which it implies.  Next to it, what does not depend on the
    conditioning at all: x_1 = alpha (pre b) is collinear with pre b, entry by entry, up to the three roundings of 1/d, pre b
    and alpha p (each entry's ratio to the long double pre b within 8 u of their median)."""
    c = pr.case("cutoff_rows")
    ld, f64 = _refs(c, cap=5)
    with _dev(c) as dev:
        check_iterates(c, dev, (1, 2, 3, 5), ld, f64, floor=8 * c.n * tr.U)
        x1, it, sc = dev.pcg(c.b, 1, c.tol)
    pb = pr.jacobi_weights(pr.tile_diag(c.A, c.nt)) * np.asarray(c.b, dtype=tr.LD)
    q = np.asarray(x1, dtype=tr.LD) / pb
    alpha = np.median(q)
    spread = float(np.abs(q / alpha - 1).max())
    a_ref = ld.rz_old[0] / ld.pap[0]
    print(f"PCGCASE cutoff_rows collinearity: alpha {float(alpha):.17g} (reference {a_ref:.17g}) spread {spread:.2e} bound {8 * tr.U:.2e}")
    assert spread <= 8 * tr.U


def test_padding_rows():
    """A partial last tile, n_valid = 400 of 432.  The padding rows (diagonal 1, right-hand side 0) keep x = 0 exactly at every cap
    (check_iterates) and the valid part follows the reference on the 400 x 400 matrix."""
    c = pr.case("padded_400_of_432")
    ld, f64 = _refs(c)
    assert ld.iters == pr.K_CONV
    with _dev(c) as dev:
        check_iterates(c, dev, (0, 1, 2, 3, 5, ld.iters, 5000), ld, f64)
        check_speculation_bits(c, dev, ld.iters)


@pytest.mark.parametrize("label", list(pr.SHAPES))
def test_shapes_that_make_the_reductions_loop(label):
    """One tile; two tiles (n = 288: two 256-blocks, the second partial); band(460): nt = 460 > 256 tile rows for the
    row_dot sum of k_pcg_step1 and 259 > 256 block partials for k_pcg_step2."""
    c = pr.case(label)
    ld, f64 = _refs(c)
    assert ld.iters == c.expect_iters
    with _dev(c) as dev:
        if label == "band460":
            assert dev.nt > 256 and (dev.n_pad + 255) // 256 > 256
        check_iterates(c, dev, (1, 3, ld.iters), ld, f64)
        check_speculation_bits(c, dev, ld.iters)


def test_pcg_voids_the_factor():
    """After pcg the tiles no longer count as a factor: solve answers InvalidState until the next factor()."""
    from apex_solver_amd import capi

    c = pr.case("dense3")
    with _dev(c) as dev:
        assert dev.factor() == 0
        x0 = dev.solve(c.b)
        dev.pcg(c.b, 1, c.tol)
        with pytest.raises(capi.LinAlgError) as ei:
            dev.solve(c.b)
        assert ei.value.kind == "InvalidState"
        dev.set(tr.touched_array(c.A, dev))
        assert dev.factor() == 0
        x1 = dev.solve(c.b)   # (the factor is back; both solves lie within the floor of the exact x)
        assert np.isfinite(x1).all() and tr.vec_err(x1, np.asarray(x0, dtype=tr.LD)) <= 2 * c.floor()
