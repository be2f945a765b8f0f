"""The task lists of the selected inversion (sinv_lists.cpp) checked without a GPU, through apexgpu_debug_sinv_lists.

1. They are the lists of the commit before they became a value: tests/golden/sinv_lists.json holds, per tile structure, the
   SHA-256 of the rows and the product counts, recorded by tools/record_sinv_lists.py from that commit.  The device sums in
   list order, so equal rows are equal bits.  Re-record only from a commit whose lists are the wanted ones.
2. They are right: replayed in numpy fp64 on numpy's own factor, C = sum +-op(A) op(B) in list order, they give Z = A^-1 on
   the filled pattern as closely as the same recurrence written directly (tile_ref.selected_inverse in fp64), both measured
   against the long double reference -- the project's referee rule, with the floor tests/test_gpu_tile_cholesky.py uses
   for Z.
3. The builder refuses a pattern that is not closed under fill (no plan produces one: symbolic fill closes every pattern)."""
import importlib.util
import json
import os

import numpy as np
import pytest

import apex_solver_amd as pkg
import tile_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_sinv_lists", os.path.join(ROOT, "tools", "record_sinv_lists.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

NB = tr.NB
L_, LINV, Z_, Y_ = range(4)          # SinvRef::array
TRANS_A, TRANS_B, NEG = 1, 2, 4      # SinvProd::op bits
PRODUCT = 3                          # row kind of a product; 0 / 1 / 2: a Y / off-diagonal Z / diagonal Z task


def test_every_recorded_list_is_reproduced():
    with open(os.path.join(ROOT, "tests", "golden", "sinv_lists.json")) as f:
        golden = json.load(f)
    seen = []
    for name, p in rec.cases():
        assert rec.entry(p) == golden[name], name
        seen.append(name)
    assert sorted(seen) == sorted(golden) and len(seen) == len(rec.tsh.structures())


SHAPES = {"grid4x4": lambda: tr.grid(4, 4), "arrow5": lambda: tr.arrow(5), "nd2": lambda: tr.nested_dissection(2),
          "band6_2": lambda: tr.band(6, 2), "dense4": lambda: tr.dense(4)}


def replay(rows, slot, Lnp, Linp):
    """Z by slot from the rows, in fp64, launch by launch.  Inside a launch no task may read what another writes (the tasks
    of a launch run side by side on the device): asserted, and what makes the serial replay the device's result."""
    tasks, prods = rows[rows[:, 0] != PRODUCT], rows[rows[:, 0] == PRODUCT]
    assert (rows[:len(tasks), 0] != PRODUCT).all()   # every task first
    by_slot = {int(slot[k]): k for k in zip(*np.nonzero(slot >= 0))}
    Z, Y, n_used = {}, {}, 0

    def tile(array, t):
        if array == L_:
            return Lnp[by_slot[t]]
        return Linp[t] if array == LINV else (Z[t] if array == Z_ else Y[t])

    launches = sorted({(int(t[1]), int(t[0])) for t in tasks})
    assert (np.diff(tasks[:, 1]) >= 0).all()   # group by group, root group first
    for g, kind in launches:
        if kind == 0:
            Y = {}   # the Y block is the group's own
        mine = tasks[(tasks[:, 1] == g) & (tasks[:, 0] == kind)]
        written = {(int(t[2]), int(t[3])) for t in mine}
        assert len(written) == len(mine), (g, kind)
        for t in mine:
            acc = np.zeros((NB, NB))
            assert t[4] == n_used   # the product list is consumed in order, without gaps
            for p in prods[t[4]:t[4] + t[5]]:
                assert (int(p[1]), int(p[2])) not in written and (int(p[3]), int(p[4])) not in written, (g, kind, p)
                A, B = tile(p[1], int(p[2])), tile(p[3], int(p[4]))
                term = (A.T if p[5] & TRANS_A else A) @ (B.T if p[5] & TRANS_B else B)
                acc = acc - term if p[5] & NEG else acc + term
            n_used += int(t[5])
            assert int(t[2]) == (Y_ if kind == 0 else Z_)
            (Y if kind == 0 else Z)[int(t[3])] = acc
    assert n_used == len(prods)
    return {by_slot[s]: z for s, z in Z.items()}


@pytest.mark.parametrize("name", list(SHAPES))
def test_replayed_lists_give_the_selected_inverse(name):
    pat = SHAPES[name]()
    nt = pat.shape[0]
    rng = np.random.default_rng(5)
    A = tr.dominant_case(pat, rng) if tr.has_fill(pat) else tr.exact_case(pat, rng)[0]
    rows, counts, slot = pkg.capi.sinv_lists(pat, with_slots=True)
    keys = tr.filled_pattern(pat)
    assert sorted(zip(*np.nonzero(slot >= 0))) == sorted(keys)
    cols = tr.symbolic_cols(pat)
    m = np.array([len(c) for c in cols])
    assert counts[:3].tolist() == [m.sum(), (m * m).sum(), (m + 1).sum()]   # one Y per tile, |I_j|^2 and 1 + |I_j| products per column
    Lnp, Linp = tr.tile_cholesky(A, pat, ld=False)
    Zr = replay(rows, slot, Lnp, Linp)
    assert sorted(Zr) == sorted(keys)
    Lref, Liref = tr.tile_cholesky(A, pat)
    Zref = tr.selected_inverse(Lref, Liref, pat, dtype=tr.LD)
    e_replay = tr.tile_err(Zr, Zref)
    e_np = tr.tile_err(tr.selected_inverse(Lnp, Linp, pat, dtype=np.float64), Zref)
    floor = 8 * nt * NB * tr.U   # (test_gpu_tile_cholesky.check_case: 8 n u, times kappa(A) only up to four tiles)
    print(f"SINV LISTS {name}: e_replay {e_replay:.2e} e_np {e_np:.2e} floor {floor:.2e}")
    assert tr.referee(e_replay, e_np, floor), (name, e_replay, e_np, floor)


def test_a_pattern_not_closed_under_fill_is_refused():
    """Column 0 has the rows {1, 2}; without the tile (2, 1) the recurrence of column 0 would need a Z tile that does not
    exist.  With it the lists build."""
    def slots(keys):
        s = np.full((3, 3), -1, dtype=np.int32)
        for i, k in enumerate(keys):
            s[k] = i
        return s
    groups = [[0], [1], [2]]
    open_keys = [(0, 0), (1, 0), (2, 0), (1, 1), (2, 2)]
    with pytest.raises(pkg.capi.LinAlgError) as e:
        pkg.capi.sinv_lists_direct(slots(open_keys), groups)
    assert e.value.kind == "InvalidState"
    assert "tile (2, 1) of column 0's rows is not a tile of the factor: the tile structure is not closed under fill" in str(e.value)
    rows, counts = pkg.capi.sinv_lists_direct(slots(open_keys + [(2, 1)]), groups)
    assert counts.tolist() == [3, 5, 6, 2] and len(rows) == 3 + 3 + 3 + 14
