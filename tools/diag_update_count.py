"""Host only: how many trailing updates of a bundle-adjustment workload's tile Cholesky target a DIAGONAL tile (A == B), per
level group, separately for the level launches and for the dataflow launch, and the flops "diag_update_lower" leaves out
(three 48 x 48 blocks of 2 * 48 * 48 * 144 flop per such update).  The plan is the one apexgpu_set_structure builds: the
camera order of apexgpu_debug_host_structure, the lists of apexgpu_debug_plan_lists.

    python tools/diag_update_count.py final-13682 ladybug-1723 [--mode selfcal]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import apex_solver_amd as pkg  # noqa: E402
from apex_solver_amd import capi  # noqa: E402

NB = 144
SKIPPED_FLOP = 3 * 2 * 48 * 48 * NB      # per diagonal-target update
UPDATE_FLOP = 2 * NB ** 3


def tile_structure(d, mode):
    """(present, stats): the lower-triangular tile structure of S in the solver's camera order."""
    import scipy.sparse as sp

    hs = capi.host_structure(d.n_cam, d.n_pt, d.cam_idx, d.pt_idx, mode=mode)
    dc = 9 if mode in (1, 4, 5, 6) else 6
    nt = int(hs["tile_rows"])
    tile = (hs["cmap"].astype(np.int64)[np.asarray(d.cam_idx, dtype=np.int64)] * dc) // NB
    inc = sp.csr_matrix((np.ones(len(tile), dtype=np.int32), (np.asarray(d.pt_idx, dtype=np.int64), tile)), shape=(d.n_pt, nt))
    inc.data[:] = 1
    cov = (inc.T @ inc).tocoo()
    present = np.zeros((nt, nt), dtype=np.uint8)
    present[np.maximum(cov.row, cov.col), np.minimum(cov.row, cov.col)] = 1
    present[np.arange(nt), np.arange(nt)] = 1
    return present, hs


def count(name, mode):
    d = pkg.datasets.load_named(name, 1.0)[0]
    present, hs = tile_structure(d, mode)
    assert int(present.sum()) == int(hs["touched_tiles"]), (int(present.sum()), hs["touched_tiles"])
    sc = capi.plan_lists(present, "scalars")[0]
    n_groups, flow_g0, flow_g1 = int(sc[0]), int(sc[10]), int(sc[11])
    lv = capi.plan_lists(present, "levels")
    rounds = capi.plan_lists(present, "upd_rounds")
    upd = capi.plan_lists(present, "upd")          # C array, C tile, first writer, A array, A tile, B array, B tile
    units = capi.plan_lists(present, "units")
    groups = capi.plan_lists(present, "group_cols")
    cols_of = np.bincount(groups[:, 0], minlength=n_groups)
    diag = (upd[:, 3] == upd[:, 5]) & (upd[:, 4] == upd[:, 6])
    print(f"{name} ({mode}): {present.shape[0]} tile rows, {int(sc[3])} tiles in {n_groups} level groups; dataflow launch over groups [{flow_g0}, {flow_g1})")
    print("  group  columns  updates  diagonal-target   (level launches)")
    tot = [0, 0]
    for g in range(min(flow_g0, n_groups)):
        r0, r1 = int(lv[g][3]), int(lv[g + 1][3])
        q0 = int(rounds[r0][0]) if r0 < len(rounds) else len(upd)
        q1 = int(rounds[r1][0]) if r1 < len(rounds) else len(upd)
        n, nd = q1 - q0, int(diag[q0:q1].sum())
        tot[0] += n; tot[1] += nd
        print(f"  {g:5d}  {cols_of[g]:7d}  {n:7d}  {nd:7d}")
    k = units[:, 13] & 15
    tile_unit = (k == 3) | ((k == 2) & (units[:, 14] == 0))
    udiag = (units[:, 2] == units[:, 4]) & (units[:, 3] == units[:, 5])
    fn, fd = int(tile_unit.sum()), int((tile_unit & udiag).sum())
    fd3 = int(((k == 3) & udiag).sum())
    print(f"  dataflow launch: {fn} updates, {fd} diagonal-target ({fd3} of them whole-tile units, {fd - fd3} as nine 48 x 48 units)")
    n_all, n_diag = tot[0] + fn, tot[1] + fd
    share = n_diag * SKIPPED_FLOP / (n_all * UPDATE_FLOP)
    print(f"  total: {n_all} updates, {n_diag} diagonal-target ({100.0 * n_diag / n_all:.1f} %); level launches {tot[1]} of {tot[0]}")
    print(f"  flops left out: {n_diag * SKIPPED_FLOP / 1e9:.2f} GFLOP of {n_all * UPDATE_FLOP / 1e9:.1f} GFLOP of updates = {100.0 * share:.2f} %")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("workloads", nargs="+")
    ap.add_argument("--mode", default="selfcal", choices=["selfcal", "ba"])
    a = ap.parse_args()
    for w in a.workloads:
        count(w, 1 if a.mode == "selfcal" else 0)
