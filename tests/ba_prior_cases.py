"""Crafted sets of camera priors for the add-on kernels of csrc/ba_prior_kernels.hip:
tests/test_ba_prior_cases_host.py proves the premises on the host, tests/test_gpu_ba_prior_crafted.py runs them on the device.

A case is (mode, problem data, pose priors, intrinsics priors); a prior is (camera, data, Huber delta or None, weight) as
Problem.add_pose_prior lists it.  The numbers in the names are the decision points they sit on: 64 lanes per workgroup of
k_ba_prior_eval, 256 threads per block of k_ba_prior_cost_add / _add_system / _add_blocks / _matvec, 144 columns per tile of S
(16 nine-column / 24 six-column cameras), 24 tile rows before hub cameras are ordered last (ba_structure.hip).

Every structure is a chain -- landmarks seen by two or three neighbouring cameras, each once -- so that no block of the Schur
reduction adds atomically and two assemblies of one handle give the same bits (the host test reads the flag off the pair lists).
Translations are rounded to multiples of 2^-10, so that a datum at a dyadic distance gives an exact residual; the cameras of
`threshold` see no landmark and sit at the identity rotation, where the prepared quaternion is (1, 0, 0, 0) in any arithmetic."""
import functools

import numpy as np

import ba_prior_ref as br
from ba_custom import custom_problem

LAM = 1.0
SELFCAL, BA = "selfcal", "ba"
EDGE_COUNTS = (64, 65, 129)
HUB, PERMUTED_CAMS = 5, 384          # 24 tile rows of 16 cameras; camera 5 shares landmarks with far tiles
DELTA_T = 0.25                       # the Huber delta of `threshold`: s = delta^2 = 2^-4 exactly
RUN = 200

CASES = ([f"edge{n}_{w}" for n in EDGE_COUNTS for w in (9, 6)]
         + ["cost257", "straddle", "pose_only", "intr_only", "disjoint", "permuted", "unobserved", "run200", "threshold", "as_coded"])


def chain(n, skip=()):
    cams = [c for c in range(n) if c not in skip]
    return [[cams[i], cams[i + 1]] for i in range(len(cams) - 1)] + [[cams[i], cams[i + 1], cams[i + 2]] for i in range(len(cams) - 2)]


def _data(n_cam, lists):
    d = custom_problem(n_cam, lists, seed=31, noise=0.7, outlier_every=5)
    d.poses = d.poses.copy(); d.intr = d.intr.copy()
    d.poses[:, :3] = np.round(d.poses[:, :3] * 1024.0) / 1024.0
    return d


def _pose(d, rng, c, delta, w, sigma=0.03):
    return (int(c), br.pose_vector(d.poses)[c] + rng.normal(0, sigma, 7), delta, float(w))


def _intr(d, rng, c, delta, w):
    return (int(c), d.intr[c] + rng.normal(0, [3.0, 1e-3, 1e-4]), delta, float(w))


def _on(d, rng, cams, intr):
    """one pose prior (and one intrinsics prior) per camera: Huber on every second one, weights 1, 0.25, 7"""
    W = (1.0, 0.25, 7.0)
    pp = [_pose(d, rng, c, 0.05 if k % 2 else None, W[k % 3]) for k, c in enumerate(cams)]
    ip = [_intr(d, rng, c, None if k % 2 else 2.0, W[(k + 1) % 3]) for k, c in enumerate(cams)] if intr else []
    return pp, ip


@functools.lru_cache(maxsize=None)
def case(name):
    """(mode, d, pose_priors, intr_priors) of a named case; shared, never modified."""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name.startswith("edge"):
        n, w = (int(x) for x in name[4:].split("_"))
        d = _data(n, chain(n))
        cams = sorted({0, 63, min(64, n - 1), n - 1})
        return (SELFCAL if w == 9 else BA, d) + _on(d, rng, cams, w == 9)
    if name == "cost257":
        d = _data(257, chain(257))
        return (BA, d) + _on(d, rng, range(257), False)
    if name == "straddle":
        d = _data(29, chain(29))
        return (SELFCAL, d) + _on(d, rng, (15, 16, 28), True)
    if name in ("pose_only", "intr_only", "disjoint"):
        d = _data(20, chain(20))
        A, B = (3, 17, 9), (7, 16, 12)
        pp = [_pose(d, rng, c, 0.05 if k == 1 else None, (1.0, 0.25, 7.0)[k]) for k, c in enumerate(A)]
        ip = [_intr(d, rng, c, 2.0 if k == 1 else None, (7.0, 1.0, 0.25)[k]) for k, c in enumerate(B)]
        return SELFCAL, d, [] if name == "intr_only" else pp, [] if name == "pose_only" else ip
    if name == "permuted":
        n = PERMUTED_CAMS
        # neighbouring tiles share 55 landmarks, the hub one landmark with each of four far tiles: under strong_edge_frac = 0.02
        # of the heaviest edge those four are long-range matches, and their cover is camera 5
        heavy = [[b - 1, b] for b in range(16, n, 16) for _ in range(52)]
        d = _data(n, chain(n) + heavy + [[HUB, c] for c in (100, 180, 260, 340)])
        # the caller's order is neither the caller's camera order nor the internal one; 300 and 6 hold two blocks each
        cams = (300, HUB, 6, 383, 300, 0, 6, 150)
        pp, ip = _on(d, rng, cams, True)
        return SELFCAL, d, pp, ip[::-1]
    if name == "unobserved":
        d = _data(10, chain(10, skip=(3, 6)))
        pp = [_pose(d, rng, 3, None, 0.5), _pose(d, rng, 3, 0.05, 2.0), _pose(d, rng, 8, None, 1.0)]
        ip = [_intr(d, rng, 3, 2.0, 1.0), _intr(d, rng, 1, None, 0.25)]
        return SELFCAL, d, pp, ip
    if name == "run200":
        d = _data(6, chain(6))
        w = 2.0 ** rng.integers(-6, 7, RUN)
        # Huber at delta = 0.075 w, the median of |r| = 0.03 w chi_7: about half of the blocks are corrected
        pp = [_pose(d, rng, 2, (0.075 * w[k]) if k % 8 else None, w[k]) for k in range(RUN)]
        pp += [_pose(d, rng, 4, None, 1.0)]
        ip = [_intr(d, rng, 2, 4.0 * w[k], w[k]) for k in range(5)]
        return SELFCAL, d, pp, ip
    if name == "threshold":
        return _threshold()
    if name == "as_coded":
        d = _data(6, chain(6))
        d.poses[4, 3:7] *= 1.0 + 1e-3                      # a parameter quaternion off the sphere: the prior sees the prepared one
        x = br.pose_vector(d.poses)
        neg = lambda c: np.concatenate([x[c, :3] + 0.25, -x[c, 3:7]])   # the double cover: data = -q, r = 2 q on the quaternion rows
        pp = [(1, neg(1), None, 1.0), (1, neg(1), 0.5, 2.0), (2, x[2] + 0.01, 0.0, 1.0), (2, x[2] + 0.02, -3.0, 0.5),
              (4, x[4] + rng.normal(0, 0.03, 7), None, 1.0), (4, neg(4), 1.0, 0.25)]
        ip = [_intr(d, rng, 4, 0.0, 1.0), _intr(d, rng, 4, None, 3.0)]
        return SELFCAL, d, pp, ip
    raise KeyError(name)


# ---- threshold --------------------------------------------------------------------------------------------------------------
# Cameras 0..3 are an ordinary chain; cameras 4.. see no landmark and hold one block each, so that p, q and the cost of a block
# can be read off its camera alone.  label -> (camera, set, row, side): side 0 sits ON the boundary (s == delta^2 bitwise, the
# test s > delta^2 is false, rho' = 1), side 1 one ulp of the datum further (s > delta^2, corrected).
THRESHOLD_BLOCKS = {"t0_on": (4, "pose", 0, 0), "t0_over": (5, "pose", 0, 1), "qz_on": (6, "pose", 6, 0), "qz_over": (7, "pose", 6, 1),
                    "row6_decides": (8, "pose", None, 1), "row6_spares": (9, "pose", None, 0),
                    "f_on": (10, "intr", 0, 0), "f_over": (11, "intr", 0, 1), "k2_on": (12, "intr", 2, 0), "k2_over": (13, "intr", 2, 1)}
THRESHOLD_CAMS = 14


def _next_over(x, datum):
    """the nearest datum below `datum` whose fp64 residual x - datum exceeds x - `datum` (one ulp of the datum, or of the
    residual where that is the coarser of the two)"""
    r, out = x - datum, datum
    while x - out == r:
        out = np.nextafter(out, -np.inf)
    return out


def _threshold():
    n = THRESHOLD_CAMS
    d = _data(n, chain(n, skip=range(4, n)))
    d.poses[4:, 3:7] = [1.0, 0.0, 0.0, 0.0]
    d.poses[4:, :3] = [1.5, -0.75, 2.0]
    d.intr[4:] = [512.0, 2.0 ** -6, 2.0 ** -10]
    x = br.pose_vector(d.poses)
    pp, ip = [], []
    for label, (c, kind, row, side) in THRESHOLD_BLOCKS.items():
        if kind == "pose":
            data = x[c].copy()
            if row is None:   # rows 0..5 alone give s = 2^-6 < delta^2; with row 6 at 0.25 s = 5 * 2^-6 > delta^2 (`decides`),
                data[0] -= 0.125   # with row 6 at 0.125 s = 2^-5 < delta^2 (`spares`)
                data[6] -= 0.25 if side else 0.125
            else:
                data[row] -= DELTA_T
                if side:
                    data[row] = _next_over(x[c][row], data[row])
            pp.append((c, data, DELTA_T, 1.0))
        else:
            data = d.intr[c].copy()
            data[row] -= DELTA_T
            if side:
                data[row] = _next_over(d.intr[c][row], data[row])
            ip.append((c, data, DELTA_T, 1.0))
    return SELFCAL, d, pp, ip


def width(name):
    return 9 if case(name)[0] == SELFCAL else 6


def host_structure(name):
    """What set_structure derives on the host for the case (nested dissection and hubs-last on, the defaults)."""
    from apex_solver_amd import capi

    mode, d, _, _ = case(name)
    return capi.host_structure(d.n_cam, d.n_pt, d.cam_idx, d.pt_idx, mode=1 if mode == SELFCAL else 0)
