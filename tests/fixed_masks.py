"""Per-DOF fixed-variable masks shared by tests/test_fixed_dofs_host.py (CPU) and tests/test_gpu_fixed_dofs.py (device),
so that both check the same inputs.  A BA mask set is a dict of uint8 arrays in the CALLER's numbering,
{"pose": (n_cam, 6), "intr": (n_cam, 3), "pt": (n_pt, 3)}; a pose-graph mask is one (n_v, 6) array.

The patterns are chosen to expose index mix-ups: a single DOF of a single variable (a shifted or permuted index moves it to
another variable), and asymmetric patterns in which every masked variable fixes a DIFFERENT subset of its DOF (a transposed
row/column or a mask read in another order changes which addends are zeroed)."""
import numpy as np


def empty(n_cam, n_pt):
    return {"pose": np.zeros((n_cam, 6), np.uint8), "intr": np.zeros((n_cam, 3), np.uint8), "pt": np.zeros((n_pt, 3), np.uint8)}


def with_gauge(m):
    """The gauge of Problem.bundle_adjustment on top of a pattern: all six DOF of camera 0."""
    m = {k: v.copy() for k, v in m.items()}
    m["pose"][0, :] = 1
    return m


def single(n_cam, n_pt, kind, index, dof):
    m = empty(n_cam, n_pt)
    m[kind][index, dof] = 1
    return m


def _subset(k, width):
    """The k-th proper non-empty subset of `width` DOF as a 0/1 row; consecutive k give different rows, and no row is
    all-ones or all-zeros (1 .. 2^width - 2, cyclic)."""
    code = 1 + (k % (2 ** width - 2))
    return np.array([(code >> a) & 1 for a in range(width)], np.uint8)


def asymmetric(n_cam, n_pt, seed, n_pose=7, n_intr=5, n_ptv=40):
    """A handful of variables of every kind, spread over the index range (first, last and random ones in between), each with
    its own subset of DOF.  The pose rows run through subsets of six DOF that are never symmetric under t <-> omega."""
    rng = np.random.default_rng(seed)
    m = empty(n_cam, n_pt)

    def pick(n, k):
        k = min(k, n)
        mid = rng.choice(np.arange(1, max(n - 1, 2)), size=max(k - 2, 0), replace=False) if n > 2 else np.zeros(0, int)
        return np.unique(np.concatenate([[0, n - 1], mid]).astype(np.int64))

    for k, c in enumerate(pick(n_cam, n_pose)):
        m["pose"][c] = _subset(5 * k + 2, 6)
    for k, c in enumerate(pick(n_cam, n_intr)):
        m["intr"][c] = _subset(k, 3)
    for k, l in enumerate(pick(n_pt, n_ptv)):
        m["pt"][l] = _subset(k + 1, 3)
    return m


def random_mask(n_cam, n_pt, seed, frac=0.3):
    """Every DOF of every variable fixed with probability `frac`."""
    rng = np.random.default_rng(seed)
    return {"pose": (rng.random((n_cam, 6)) < frac).astype(np.uint8), "intr": (rng.random((n_cam, 3)) < frac).astype(np.uint8),
            "pt": (rng.random((n_pt, 3)) < frac).astype(np.uint8)}


def all_of(n_cam, n_pt, kind):
    """Every DOF of every variable of one kind ("pt": all landmarks fixed, "intr": all intrinsics fixed)."""
    m = empty(n_cam, n_pt)
    m[kind][:] = 1
    return m


def on_variables(n_cam, n_pt, cams=(), pts=(), seed=0):
    """Asymmetric subsets on the given cameras (pose and intrinsics, different subsets) and landmarks."""
    m = empty(n_cam, n_pt)
    for k, c in enumerate(cams):
        m["pose"][c] = _subset(7 * k + seed + 3, 6)
        m["intr"][c] = _subset(k + seed, 3)
    for k, l in enumerate(pts):
        m["pt"][l] = _subset(k + seed, 3)
    return m


def count(m):
    return {k: int(v.sum()) for k, v in m.items()}


def apply_to_problem(prob, m):
    """Set a mask set on an apex_solver_amd.solver.Problem through Problem.fix_variable, name by name (the path a caller of the
    reference's interface takes), and return the problem."""
    for kind, fmt in (("pose", "pose_{:04d}"), ("intr", "intr_{:04d}"), ("pt", "pt_{:05d}")):
        for i, a in zip(*np.nonzero(m[kind])):
            prob.fix_variable(fmt.format(int(i)), int(a))
    return prob


# ---- pose graph -----------------------------------------------------------------------------------------------------------------
def pg_empty(n_v):
    return np.zeros((n_v, 6), np.uint8)


def pg_single(n_v, vertex, dof):
    m = pg_empty(n_v)
    m[vertex, dof] = 1
    return m


def pg_asymmetric(n_v, seed, n=9):
    rng = np.random.default_rng(seed)
    m = pg_empty(n_v)
    vs = np.unique(np.concatenate([[1, n_v - 1], rng.choice(np.arange(2, n_v - 1), size=min(n, n_v - 3), replace=False)]))
    for k, v in enumerate(vs):
        m[v] = _subset(5 * k + 2, 6)
    return m


def pg_random(n_v, seed, frac=0.3):
    return (np.random.default_rng(seed).random((n_v, 6)) < frac).astype(np.uint8)


def pg_apply_to_problem(prob, fix):
    """Through PoseGraphProblem.fix_variable by name (`x<id>`: the id, not the row)."""
    for v, a in zip(*np.nonzero(fix)):
        prob.fix_variable(f"x{int(prob.data.ids[v])}", int(a))
    return prob
