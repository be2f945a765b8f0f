"""Pose-graph path, SE3, SE2 and SO3 (BASELINE.json configs[1]): Python mirror of what bin/pose_graph_g2o.rs drives --
`G2oLoader` (crates/apex-io/src/g2o.rs) over the library's C++ reader, the `Problem` of BetweenFactor<SE3>
blocks with the first vertex fixed, and the `SparseCholesky` linear solver on the device
(`GpuSparseCholeskySolver`, src/linalg/sparse/cholesky.rs:159-230).  Every numeric path calls
libapexgpu.so; there is no CPU fallback.

SE2 (the 2D half of bin/pose_graph_g2o.rs, :314-700): the same classes on 3-wide data -- pose / measurement / prior data
= [x, y, theta], three tangent columns per vertex.  The manifold is picked from the width of `data.poses`.

SO3 (rotation averaging, BetweenFactor<SO3>: src/factors/between_factor.rs:13,55): the same classes on 4-wide data -- vertex /
measurement / prior data = [qw, qx, qy, qz], three tangent columns per vertex; `PoseGraphProblem(data, manifold="so3")`."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import capi
from .handle_solver import HandleSolver
from .loss import Loss, create_loss_function   # (both front ends use them; exported from here as before)
from .synthetic import PoseGraphData

G2O_ERROR_NAMES = {-30: "Io", -31: "Parse", -32: "MissingFields", -33: "InvalidNumber", -34: "DuplicateVertex",
                   -35: "InvalidQuaternion"}


class G2oError(RuntimeError):
    """Mirror of apex_io::IoError for the G2O reader: `.kind` is the variant name."""

    def __init__(self, code: int, message: str):
        self.code = code
        self.kind = G2O_ERROR_NAMES.get(code, f"Error({code})")
        super().__init__(f"{self.kind}: {message}")


@dataclass
class G2oGraph:
    """apex_io::Graph restricted to SE3 (crates/apex-io/src/lib.rs:336-341), columnar, file order."""

    vertex_ids: np.ndarray      # (n_v,) int64
    vertex_poses: np.ndarray    # (n_v, 7) [t, qw,qx,qy,qz]
    edge_from: np.ndarray       # (n_e,) int64 vertex ids
    edge_to: np.ndarray
    edge_measurements: np.ndarray  # (n_e, 7)
    edge_information: np.ndarray   # (n_e, 6, 6)
    n_vertices_se2: int = 0
    n_edges_se2: int = 0
    _problem: PoseGraphData | None = field(default=None, repr=False)
    # the SE2 content (VertexSE2 / EdgeSE2, crates/apex-io/src/lib.rs), file order
    vertex_ids_se2: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))
    poses_se2: np.ndarray = field(default_factory=lambda: np.zeros((0, 3)))          # (n, 3) [x, y, theta]
    edge_from_se2: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))
    edge_to_se2: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))
    edge_meas_se2: np.ndarray = field(default_factory=lambda: np.zeros((0, 3)))
    edge_info_se2: np.ndarray = field(default_factory=lambda: np.zeros((0, 3, 3)))
    _problem_se2: PoseGraphData | None = field(default=None, repr=False)
    _problem_se2_error: tuple | None = field(default=None, repr=False)   # (code, message) the SE2 problem builder answered

    def vertex_count(self) -> int:
        return int(self.vertex_ids.shape[0]) + self.n_vertices_se2

    def edge_count(self) -> int:
        return int(self.edge_from.shape[0]) + self.n_edges_se2

    def to_problem_data(self, name: str = "g2o", manifold: str | None = None, use_information: bool = False) -> PoseGraphData:
        """manifold "se3" | "se2" | "so3"; None: "se2" for a file with SE2 content only, else "se3".  use_information: the file's
        edge information matrices go along as `information`, in the problem's edge order (default: None, they are not used).
        "so3": the rotation part of the file's SE3 content -- the quaternions [qw, qx, qy, qz] of the vertices and of the edges'
        measurements, and with use_information the rotational 3 x 3 block of every 6 x 6 matrix (tangent order [rho; theta])."""
        if manifold is None:
            manifold = "se2" if (self.vertex_ids.shape[0] == 0 and self.n_vertices_se2 > 0) else "se3"
        if manifold not in ("se3", "se2", "so3"):
            raise ValueError(manifold)
        if manifold == "so3":
            p = self._problem
            if p is None or p.n_v == 0:
                raise ValueError("to_problem_data(manifold=\"so3\"): the file holds no SE3 content to take rotations from")
            info = None if (not use_information or p.information is None) else np.ascontiguousarray(p.information[:, 3:6, 3:6])
            return PoseGraphData(ids=p.ids.copy(), poses=np.ascontiguousarray(p.poses[:, 3:7]), e_from=p.e_from.copy(),
                                 e_to=p.e_to.copy(), meas=np.ascontiguousarray(p.meas[:, 3:7]), name=name, information=info)
        if manifold == "se2" and self._problem_se2_error is not None:
            # (e.g. an EDGE_SE2 that names a vertex the file does not hold: the file still loads, as it did when SE2 lines
            # were only counted; the error belongs to whoever asks for the SE2 problem)
            raise G2oError(*self._problem_se2_error)
        p = self._problem_se2 if manifold == "se2" else self._problem
        assert p is not None
        info = None if (not use_information or p.information is None) else p.information.copy()
        return PoseGraphData(ids=p.ids.copy(), poses=p.poses.copy(), e_from=p.e_from.copy(), e_to=p.e_to.copy(),
                             meas=p.meas.copy(), name=name, information=info)


class G2oLoader:
    @staticmethod
    def load(path) -> G2oGraph:
        L = capi.load()
        h = C.c_void_p()
        rc = L.apexgpu_g2o_open(str(path).encode(), C.byref(h))
        if rc != 0:
            raise G2oError(rc, L.apexgpu_g2o_last_error().decode())
        try:
            nv, ne, nv2, ne2 = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
            L.apexgpu_g2o_sizes(h, C.byref(nv), C.byref(ne), C.byref(nv2), C.byref(ne2))
            nv, ne = nv.value, ne.value
            ids = np.zeros(nv, np.int64); poses = np.zeros((nv, 7)); ef = np.zeros(ne, np.int64); et = np.zeros(ne, np.int64)
            meas = np.zeros((ne, 7)); info = np.zeros((ne, 6, 6))
            L.apexgpu_g2o_raw(h, capi.ptr(ids), capi.ptr(poses), capi.ptr(ef), capi.ptr(et), capi.ptr(meas), capi.ptr(info))
            sid = np.zeros(nv, np.int64); sp = np.zeros((nv, 7)); pf = np.zeros(ne, np.uint32); pt = np.zeros(ne, np.uint32)
            pm = np.zeros((ne, 7))
            rc = L.apexgpu_g2o_problem(h, capi.ptr(sid), capi.ptr(sp), capi.ptr(pf), capi.ptr(pt), capi.ptr(pm), None, None)
            if rc != 0:
                raise G2oError(rc, L.apexgpu_g2o_last_error().decode())
            pi = np.zeros((ne, 6, 6))
            L.apexgpu_g2o_problem_information(h, capi.MANIFOLD_SE3, capi.ptr(pi))
            prob = PoseGraphData(ids=sid, poses=sp, e_from=pf, e_to=pt, meas=pm, information=pi)
            nv2, ne2 = nv2.value, ne2.value
            ids2 = np.zeros(nv2, np.int64); poses2 = np.zeros((nv2, 3)); ef2 = np.zeros(ne2, np.int64); et2 = np.zeros(ne2, np.int64)
            meas2 = np.zeros((ne2, 3)); info2 = np.zeros((ne2, 3, 3))
            L.apexgpu_g2o_raw_se2(h, capi.ptr(ids2), capi.ptr(poses2), capi.ptr(ef2), capi.ptr(et2), capi.ptr(meas2), capi.ptr(info2))
            sid2 = np.zeros(nv2, np.int64); sp2 = np.zeros((nv2, 3)); pf2 = np.zeros(ne2, np.uint32); pt2 = np.zeros(ne2, np.uint32)
            pm2 = np.zeros((ne2, 3))
            rc = L.apexgpu_g2o_problem_se2(h, capi.ptr(sid2), capi.ptr(sp2), capi.ptr(pf2), capi.ptr(pt2), capi.ptr(pm2), None, None)
            err2 = (rc, L.apexgpu_g2o_last_error().decode()) if rc != 0 else None
            pi2 = np.zeros((ne2, 3, 3))
            L.apexgpu_g2o_problem_information(h, capi.MANIFOLD_SE2, capi.ptr(pi2))
            prob2 = None if err2 else PoseGraphData(ids=sid2, poses=sp2, e_from=pf2, e_to=pt2, meas=pm2, information=pi2)
            return G2oGraph(ids, poses, ef, et, meas, info, nv2, ne2, prob, ids2, poses2, ef2, et2, meas2, info2, prob2, err2)
        finally:
            L.apexgpu_g2o_close(h)


def write_g2o(path, data: PoseGraphData, information: np.ndarray | None = None):
    """G2oLoader::write for SE3 graphs (g2o.rs:20-135): vertices sorted by id, `{:.17e}` numbers,
    21 upper-triangular information values per edge (identity unless given)."""
    def fmt(x):
        return f"{float(x):.17e}"
    if data.poses.shape[1] == 3:   # SE2: VERTEX_SE2 id x y theta, EDGE_SE2 from to dx dy dtheta + 6 upper-triangular values
        with open(path, "w") as f:
            f.write("# G2O file written by Apex Solver\n")
            f.write(f"# SE2 vertices: {data.n_v}, SE3 vertices: 0, SE2 edges: {data.n_e}, SE3 edges: 0\n\n")
            for k in np.argsort(data.ids, kind="stable"):
                f.write("VERTEX_SE2 %d %s\n" % (data.ids[k], " ".join(fmt(v) for v in data.poses[k])))
            for e in range(data.n_e):
                I = np.eye(3) if information is None else information[e]
                iu = [I[i, j] for i in range(3) for j in range(i, 3)]
                f.write("EDGE_SE2 %d %d %s %s\n" % (data.ids[data.e_from[e]], data.ids[data.e_to[e]],
                        " ".join(fmt(v) for v in data.meas[e]), " ".join(fmt(v) for v in iu)))
        return
    with open(path, "w") as f:
        f.write("# G2O file written by Apex Solver\n")
        f.write(f"# SE2 vertices: 0, SE3 vertices: {data.n_v}, SE2 edges: 0, SE3 edges: {data.n_e}\n\n")
        order = np.argsort(data.ids, kind="stable")
        for k in order:
            p = data.poses[k]
            f.write("VERTEX_SE3:QUAT %d %s\n" % (data.ids[k], " ".join(fmt(v) for v in (p[0], p[1], p[2], p[4], p[5], p[6], p[3]))))
        for e in range(data.n_e):
            m = data.meas[e]
            I = np.eye(6) if information is None else information[e]
            iu = [I[i, j] for i in range(6) for j in range(i, 6)]
            f.write("EDGE_SE3:QUAT %d %d %s %s\n" % (data.ids[data.e_from[e]], data.ids[data.e_to[e]],
                    " ".join(fmt(v) for v in (m[0], m[1], m[2], m[4], m[5], m[6], m[3])), " ".join(fmt(v) for v in iu)))


def pose_graph_columns(ids: np.ndarray, dof: int = 6) -> np.ndarray:
    """First global column of `x{id}` in sorted-name order (src/optimizer/mod.rs:530-536); dof 6 (SE3) | 3 (SE2, SO3: the
    3-column layout is the same, apexgpu_pose_graph_columns_se2 serves both)."""
    L = capi.load()
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    out = np.zeros(ids.shape[0], np.int64)
    fn = L.apexgpu_pose_graph_columns_se2 if dof == 3 else L.apexgpu_pose_graph_columns
    rc = fn(ids.shape[0], capi.ptr(ids), capi.ptr(out))
    if rc != 0:
        raise G2oError(rc, L.apexgpu_g2o_last_error().decode())
    return out


def se3_as_vector(pose7) -> np.ndarray:
    """SE3::from(DVector).to_vector(): [t, w, i, j, k] with the quaternion normalised (se3.rs:200-206, 107-113)."""
    p = np.asarray(pose7, dtype=np.float64).reshape(7).copy()
    q = p[3:7]
    q = q / np.sqrt(np.dot(q, q))
    q = q / np.sqrt(np.dot(q, q))
    p[3:7] = q
    return p


def se2_as_vector(pose3) -> np.ndarray:
    """SE2::from(DVector) -> DVector: [x, y, theta] with theta = atan2(sin, cos) (se2.rs:48-63); a theta already in
    (-pi, pi] is its own image."""
    p = np.asarray(pose3, dtype=np.float64).reshape(3).copy()
    if not (-np.pi < p[2] <= np.pi):
        p[2] = np.arctan2(np.sin(p[2]), np.cos(p[2]))
    return p


def so3_as_vector(quat4) -> np.ndarray:
    """SO3::from(DVector) -> DVector: [w, i, j, k] normalised (so3.rs:225-235), with the two passes an SE3 pose's quaternion gets."""
    q = np.asarray(quat4, dtype=np.float64).reshape(4).copy()
    q = q / np.sqrt(np.dot(q, q))
    q = q / np.sqrt(np.dot(q, q))
    return q


_MANIFOLD_SIZES = {"se3": (6, 7), "se2": (3, 3), "so3": (3, 4)}   # (dof, ambient)
_MANIFOLD_IDS = {"se3": capi.MANIFOLD_SE3, "se2": capi.MANIFOLD_SE2, "so3": capi.MANIFOLD_SO3}


@dataclass
class PoseGraphProblem:
    """The factor graph bin/pose_graph_g2o.rs:748-830 builds: variables `x{id}` (SE3), one
    BetweenFactor(measurement) per edge on (x{from}, x{to}), optional loss on every block."""

    data: PoseGraphData
    huber_delta: float | None = None
    fix: np.ndarray = field(default=None)
    priors: list = field(default_factory=list)   # (vertex index, data[7], huber delta or None) per PriorFactor block
    loss: Loss | None = None   # the loss of every BetweenFactor block; mutually exclusive with huber_delta
    information: np.ndarray | None = None   # (n_e, dof, dof) edge information matrices; None: data.information (None: not used)
    manifold: str | None = None   # "se3" | "se2" | "so3"; None: from the width of data.poses (7 | 3 | 4)

    def __post_init__(self):
        if self.loss is not None and self.huber_delta is not None:
            raise ValueError("PoseGraphProblem: give either loss or huber_delta, not both")
        if self.manifold is None:
            self.manifold = self.data.manifold
        if self.manifold not in _MANIFOLD_SIZES:
            raise ValueError(f"PoseGraphProblem: unknown manifold {self.manifold!r}")
        self.dof, self.ambient = _MANIFOLD_SIZES[self.manifold]
        if self.data.poses.shape[1] != self.ambient or self.data.meas.shape[1] != self.ambient:
            raise ValueError(f"PoseGraphProblem: a {self.manifold} graph has {self.ambient}-wide poses and measurements")
        if self.information is None:
            self.information = self.data.information
        if self.information is not None:
            self.information = np.ascontiguousarray(self.information, dtype=np.float64)
            if self.information.shape != (self.data.n_e, self.dof, self.dof):
                raise ValueError(f"information must be ({self.data.n_e}, {self.dof}, {self.dof})")
        if self.fix is None:
            self.fix = np.zeros((self.data.n_v, self.dof), dtype=np.uint8)
        self.pose_col = pose_graph_columns(self.data.ids, self.dof)

    def add_prior(self, name: str, data=None, huber_delta: float | None = None):
        """`problem.add_residual_block(&[name], PriorFactor { data }, loss)` (src/factors/prior_factor.rs:53-113): the
        gauge of the reference's pose-graph integration test (tests/integration_tests.rs:98-118, Huber(1.0), data = the
        variable's initial value).  r = to_vector(x) - data, seven rows; the linearizer keeps the first six columns of the
        7 x 7 identity Jacobian (src/linearizer/cpu/sparse.rs:201-204)."""
        if not name.startswith("x"):
            raise KeyError(name)
        hit = np.nonzero(self.data.ids == int(name[1:]))[0]
        if hit.size == 0:
            raise KeyError(name)
        v = int(hit[0])
        if self.manifold == "se2":   # r = [x, y, theta] - data, three rows, Jacobian I3 (integration_tests.rs:213-231)
            x = se2_as_vector(self.data.poses[v]) if data is None else np.asarray(data, dtype=np.float64).reshape(3)
        elif self.manifold == "so3":   # r = [w, i, j, k] - data, four rows; the linearizer keeps three columns of I4 (sparse.rs:201-204)
            x = so3_as_vector(self.data.poses[v]) if data is None else np.asarray(data, dtype=np.float64).reshape(4)
        else:
            x = se3_as_vector(self.data.poses[v]) if data is None else np.asarray(data, dtype=np.float64).reshape(7)
        self.priors.append((v, x, huber_delta))
        return self

    @classmethod
    def pose_graph(cls, data: PoseGraphData, huber_delta: float | None = None, loss: Loss | None = None,
                   information: np.ndarray | None = None) -> "PoseGraphProblem":
        """The LM set-up: all six DOF of the first vertex fixed (pose_graph_g2o.rs:790-797).  information: the edges'
        information matrices (n_e, dof, dof); None: data.information."""
        p = cls(data, huber_delta, loss=loss, information=information)
        for dof in range(p.dof):
            p.fix_variable(f"x{int(data.ids[0])}", dof)
        return p

    def fix_variable(self, name: str, dof: int):
        """Problem::fix_variable (src/core/problem.rs:609-616)."""
        if not name.startswith("x"):
            raise KeyError(name)
        hit = np.nonzero(self.data.ids == int(name[1:]))[0]
        if hit.size == 0:
            raise KeyError(name)
        self.fix[hit[0], dof] = 1

    @property
    def total_dof(self) -> int:
        return self.dof * self.data.n_v

    @property
    def num_residual_blocks(self) -> int:
        return self.data.n_e + len(self.priors)


@dataclass
class GaussNewtonConfig:
    """Defaults of gauss_newton.rs:236-255; fields the loop never reads (min_diagonal, max_condition_number) are not reproduced."""

    max_iterations: int = 50
    cost_tolerance: float = 1e-6
    parameter_tolerance: float = 1e-8
    gradient_tolerance: float = 1e-10
    timeout: float | None = None
    min_cost_threshold: float | None = None
    use_jacobi_scaling: bool = False
    variant: int = 0   # the sparse Cholesky solver; anything else is refused

    def to_c(self) -> capi.GnConfigC:
        return capi.GnConfigC(self.max_iterations, self.cost_tolerance, self.parameter_tolerance, self.gradient_tolerance,
                              -1.0 if self.min_cost_threshold is None else self.min_cost_threshold,
                              -1.0 if self.timeout is None else float(self.timeout), int(self.variant),
                              1 if self.use_jacobi_scaling else 0)


@dataclass
class DogLegConfig:
    """Defaults of dog_leg.rs:353-399; fields the loop never reads (trust_region_increase_factor -- the radius grows by the
    literal 3 --, min_step_quality, min_relative_decrease, max_condition_number) are not reproduced."""

    max_iterations: int = 50
    cost_tolerance: float = 1e-6
    parameter_tolerance: float = 1e-8
    gradient_tolerance: float = 1e-10
    timeout: float | None = None
    trust_region_radius: float = 1e4
    trust_region_min: float = 1e-12
    trust_region_max: float = 1e12
    trust_region_decrease_factor: float = 0.5
    good_step_quality: float = 0.75
    poor_step_quality: float = 0.25
    use_jacobi_scaling: bool = True
    initial_mu: float = 1e-4
    min_mu: float = 1e-8
    max_mu: float = 1.0
    mu_increase_factor: float = 10.0
    enable_step_reuse: bool = True
    min_cost_threshold: float | None = None
    variant: int = 0   # the sparse Cholesky solver; anything else is refused

    def to_c(self) -> capi.DlConfigC:
        return capi.DlConfigC(self.max_iterations, self.cost_tolerance, self.parameter_tolerance, self.gradient_tolerance,
                              self.trust_region_radius, self.trust_region_min, self.trust_region_max,
                              self.trust_region_decrease_factor, self.good_step_quality, self.poor_step_quality,
                              self.initial_mu, self.min_mu, self.max_mu, self.mu_increase_factor,
                              -1.0 if self.min_cost_threshold is None else self.min_cost_threshold,
                              -1.0 if self.timeout is None else float(self.timeout), int(self.variant),
                              1 if self.use_jacobi_scaling else 0, 1 if self.enable_step_reuse else 0)


class GpuSparseCholeskySolver(HandleSolver):
    """Device counterpart of SparseCholeskySolver (src/linalg/sparse/cholesky.rs) for pose graphs:
    `solve_augmented_equation(lambda)` linearises the BetweenFactors, assembles J^T J + lambda I
    block-sparse and solves by the tile Cholesky.  No Schur complement.  The calls it shares with the bundle-adjustment
    solver are HandleSolver's."""

    _STAGE_NAMES = capi.PG_STAGE_NAMES

    def __init__(self, device: int = 0):
        super().__init__(device)
        self.problem: PoseGraphProblem | None = None

    def _need(self) -> capi.PgHandle:
        return self._h or self._built(-6)

    def _total_dof(self) -> int:
        return self._h.dof * self._h.n_vertices

    def _variant(self) -> int:
        return 0

    def initialize_structure(self, problem: PoseGraphProblem):
        d = problem.data
        self.close()
        h = capi.PgHandle(d.n_v, d.n_e, self.device, _MANIFOLD_IDS[problem.manifold])
        self._apply_options(h)
        ef = np.ascontiguousarray(d.e_from, dtype=np.uint32); et = np.ascontiguousarray(d.e_to, dtype=np.uint32)
        meas = np.ascontiguousarray(d.meas, dtype=np.float64)
        fix = np.ascontiguousarray(problem.fix, dtype=np.uint8)
        col = np.ascontiguousarray(problem.pose_col, dtype=np.int64)
        delta = -1.0 if problem.huber_delta is None else float(problem.huber_delta)
        h.check(h.L.apexgpu_pg_set_structure(h.h, capi.ptr(ef), capi.ptr(et), capi.ptr(meas), capi.ptr(col), capi.ptr(fix), delta))
        self._h, self.problem = h, problem
        if problem.loss is not None:
            self.set_loss(problem.loss)
        if problem.priors:
            self.set_priors(problem.priors)
        if problem.information is not None:
            self.set_information(problem.information)
        return self

    def set_information(self, information):
        """The information matrix of every BetweenFactor block, (n_e, dof, dof) in the problem's edge order: the block is
        whitened by it before the loss acts.  None: none, the handle is what it was before.  Raises LinAlgError (InvalidInput,
        naming the edge) for a matrix that is not finite, not symmetric or not positive definite; the handle keeps what it had."""
        h = self._need()
        a = None
        if information is not None:
            a = np.ascontiguousarray(information, dtype=np.float64)
            if a.shape != (h.n_edges, h.dof, h.dof):
                raise ValueError(f"information must be ({h.n_edges}, {h.dof}, {h.dof})")
        h.check(h.L.apexgpu_pg_set_information(h.h, capi.ptr(a)))

    def get_information(self):
        """The stored information matrices (n_e, dof, dof), full and symmetric; None when the handle has none."""
        h = self._need()
        present = C.c_int(0)
        out = np.zeros((h.n_edges, h.dof, h.dof))
        h.check(h.L.apexgpu_pg_get_information(h.h, C.byref(present), capi.ptr(out)))
        return out if present.value else None

    def set_priors(self, priors):
        """PriorFactor blocks: (vertex index, data[7], huber delta or None) each; replaces the set."""
        h = self._need()
        v = np.ascontiguousarray([q[0] for q in priors], dtype=np.uint32)
        x = np.ascontiguousarray([q[1] for q in priors], dtype=np.float64).reshape(-1, h.ambient)
        dl = np.ascontiguousarray([-1.0 if q[2] is None else float(q[2]) for q in priors], dtype=np.float64)
        h.check(h.L.apexgpu_pg_set_priors(h.h, len(v), capi.ptr(v), capi.ptr(x), capi.ptr(dl)))

    def get_prior_residual(self) -> np.ndarray:
        """Corrected residuals of the prior blocks at the current parameters: [n_prior][7]."""
        h = self._need()
        n = len(self.problem.priors)
        r = np.zeros((n, h.ambient))
        if n: h.check(h.L.apexgpu_pg_get_prior_residual(h.h, capi.ptr(r)))
        return r

    def set_parameters(self, poses):
        h = self._need()
        p = np.ascontiguousarray(poses, dtype=np.float64)
        if p.shape != (h.n_vertices, h.ambient):
            raise ValueError(f"poses must be ({h.n_vertices}, {h.ambient})")
        h.check(h.L.apexgpu_pg_set_params(h.h, capi.ptr(p)))

    def get_parameters(self) -> np.ndarray:
        h = self._need()
        p = np.zeros((h.n_vertices, h.ambient))
        h.check(h.L.apexgpu_pg_get_params(h.h, capi.ptr(p)))
        return p

    def solve_augmented_equation(self, lam: float, want_step: bool = True):
        h = self._need()
        n = self._total_dof()
        step = np.zeros(n) if want_step else None
        self._gradient = np.zeros(n) if want_step else None
        h.check(h.L.apexgpu_pg_solve_augmented(h.h, float(lam), capi.ptr(step), capi.ptr(self._gradient)))
        return step

    def get_residual(self) -> np.ndarray:
        h = self._need()
        r = np.zeros((h.n_edges, h.dof))
        h.check(h.L.apexgpu_pg_get_residual(h.h, capi.ptr(r)))
        return r

    def get_jacobian_blocks(self) -> np.ndarray:
        h = self._need()
        j = np.zeros((h.n_edges, h.dof, 2 * h.dof))
        h.check(h.L.apexgpu_pg_get_jacobian_blocks(h.h, capi.ptr(j)))
        return j

    def get_hessian(self, lam: float = 0.0):
        h = self._need()
        n = h.dof * h.n_vertices
        H = np.zeros((n, n)); g = np.zeros(n)
        h.check(h.L.apexgpu_pg_get_hessian(h.h, float(lam), capi.ptr(H), capi.ptr(g)))
        return H, g

    def pose_covariance_blocks(self) -> np.ndarray:
        """(n_v, 6, 6): the diagonal blocks of the inverse of the matrix the last solve factorised (J^T J + lambda I at its
        point and lambda; scaled variables under Jacobi scaling -- what get_hessian(lambda) returns there), by selected
        inversion of the tile factor.  Caller's vertex order.  Raises LinAlgError (InvalidState) when no factor is held
        (no solve yet, or an assembly / export since)."""
        h = self._need()
        out = np.zeros((h.n_vertices, h.dof, h.dof))
        h.check(h.L.apexgpu_pg_covariance(h.h, capi.ptr(out)))
        return out

    def compute_covariances(self) -> dict:
        """LinearSolver::compute_covariance_matrix + Problem::extract_variable_covariances (src/linalg/mod.rs:165-215,
        src/core/problem.rs:1128-1147): {"x{id}": 6 x 6} for every vertex."""
        blocks = self.pose_covariance_blocks()
        return {f"x{int(i)}": blocks[k].copy() for k, i in enumerate(self.problem.data.ids)}

    def info(self) -> dict:
        h = self._need()
        a = (C.c_double * 9)()
        h.check(h.L.apexgpu_pg_info(h.h, C.byref(a)))
        return {"tile_rows": int(a[0]), "tiles": int(a[1]), "touched_tiles": int(a[2]), "etree_levels": int(a[3]),
                "total_dof": int(a[4]), "n_potrf": int(a[5]), "n_trsm": int(a[6]), "n_update": int(a[7]),
                "n_update_diag": int(a[8])}

    def gn_optimize(self, cfg: GaussNewtonConfig):
        """GaussNewton::optimize (gauss_newton.rs:559-720) on the device: (result, history (n, 8) in LmIterC's columns with
        damping = rho = 0 and accepted = 1, the config as the loop left it)."""
        return self._optimize("gn_optimize", cfg, capi.LmIterC)
