"""ctypes binding of the C-ABI library (include/apexgpu.h).

The library is the product: there is no Python/CPU fallback.  Loading fails loudly when
`libapexgpu.so` is missing; every compute entry point returns an error when no MI355X is visible.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libapexgpu.so")
LIB_PATH = os.environ.get("APEXGPU_LIB", LIB_PATH)   # (A/B of two builds on one box: tools only)

NUM_STAGES = 10
STAGE_NAMES = ("cam_reduce", "landmark_reduce", "schur_scatter", "all_reduce", "factor", "tri_solve",
               "back_substitute", "step_stats", "retract", "cost")

MANIFOLD_SE3, MANIFOLD_SE2, MANIFOLD_SO3 = 0, 1, 2
# (ambient, dof) per APEXGPU_MANIFOLD_*: stored doubles per vertex / measurement / prior, tangent columns per vertex
MANIFOLD_SIZES = {MANIFOLD_SE3: (7, 6), MANIFOLD_SE2: (3, 3), MANIFOLD_SO3: (4, 3)}
# APEXGPU_LOSS_* of include/apexgpu.h, in value order
LOSS_KINDS = ("NONE", "L2", "L1", "HUBER", "CAUCHY", "FAIR", "GEMAN_MCCLURE", "WELSCH", "TUKEY", "ANDREWS", "RAMSAY",
              "TRIMMED_MEAN", "LP_NORM", "BARRON", "T_DISTRIBUTION")
(LOSS_NONE, LOSS_L2, LOSS_L1, LOSS_HUBER, LOSS_CAUCHY, LOSS_FAIR, LOSS_GEMAN_MCCLURE, LOSS_WELSCH, LOSS_TUKEY, LOSS_ANDREWS,
 LOSS_RAMSAY, LOSS_TRIMMED_MEAN, LOSS_LP_NORM, LOSS_BARRON, LOSS_T_DISTRIBUTION) = range(15)
PG_NUM_STAGES = 6
PG_STAGE_NAMES = ("assemble", "factor", "tri_solve", "step_stats", "retract", "cost")

ERROR_NAMES = {
    -1: "FactorizationFailed", -2: "SingularMatrix", -3: "SparseMatrixCreation", -4: "MatrixConversion",
    -5: "InvalidInput", -6: "InvalidState", -10: "DeviceError",
}


class LinAlgError(RuntimeError):
    """Mirror of apex-solver's LinAlgError (src/linalg/mod.rs:76-101): `.kind` is the variant name."""

    def __init__(self, code: int, message: str):
        self.code = code
        self.kind = ERROR_NAMES.get(code, f"Error({code})")
        super().__init__(f"{self.kind}: {message}")


class LmConfigC(C.Structure):
    _fields_ = [
        ("max_iterations", C.c_int), ("cost_tolerance", C.c_double), ("parameter_tolerance", C.c_double),
        ("gradient_tolerance", C.c_double), ("damping", C.c_double), ("damping_min", C.c_double),
        ("damping_max", C.c_double), ("damping_nu", C.c_double), ("trust_region_radius", C.c_double),
        ("min_trust_region_radius", C.c_double), ("min_cost_threshold", C.c_double), ("timeout_s", C.c_double),
        ("variant", C.c_int), ("use_jacobi_scaling", C.c_int),
    ]


class LmIterC(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("cost", "damping", "rho", "accepted", "gradient_norm", "step_norm",
                                          "predicted_reduction", "trial_cost")]


class LmResultC(C.Structure):
    _fields_ = [
        ("status", C.c_int), ("iterations", C.c_int), ("initial_cost", C.c_double), ("final_cost", C.c_double),
        ("final_gradient_norm", C.c_double), ("final_step_norm", C.c_double), ("elapsed_s", C.c_double),
        ("cost_evaluations", C.c_int), ("jacobian_evaluations", C.c_int), ("successful_steps", C.c_int),
        ("unsuccessful_steps", C.c_int),
    ]


class GnConfigC(C.Structure):
    _fields_ = [
        ("max_iterations", C.c_int), ("cost_tolerance", C.c_double), ("parameter_tolerance", C.c_double),
        ("gradient_tolerance", C.c_double), ("min_cost_threshold", C.c_double), ("timeout_s", C.c_double),
        ("variant", C.c_int), ("use_jacobi_scaling", C.c_int),
    ]


class DlConfigC(C.Structure):
    _fields_ = [("max_iterations", C.c_int)] + [(n, C.c_double) for n in (
        "cost_tolerance", "parameter_tolerance", "gradient_tolerance", "trust_region_radius", "trust_region_min",
        "trust_region_max", "trust_region_decrease_factor", "good_step_quality", "poor_step_quality", "mu", "min_mu", "max_mu",
        "mu_increase_factor", "min_cost_threshold", "timeout_s")] + [
        ("variant", C.c_int), ("use_jacobi_scaling", C.c_int), ("enable_step_reuse", C.c_int)]


class DlIterC(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("cost", "radius", "mu", "rho", "accepted", "gradient_norm", "step_norm",
                                          "predicted_reduction", "trial_cost", "step_type", "beta", "reused")]


DL_STEP_TYPES = ("GaussNewton", "SteepestDescent", "DogLeg")   # StepType (dog_leg.rs), the value of step_type

_int, _i64, _dbl, _vp, _str, _P = C.c_int, C.c_int64, C.c_double, C.c_void_p, C.c_char_p, C.POINTER
_opt = [_P(LmResultC), _vp, _int]   # after the handle and the config of an optimise call: result, history, its capacity
_pairs = [_vp] * 8                       # apexgpu_debug_pair_lists*: cam_idx, pt_idx, counts[4], then five outputs

# Every function include/apexgpu.h declares, in its order: name -> (restype, argtypes).  load() applies exactly this table;
# SYMBOLS is its key set (held to the header by tests/test_capi_symbols.py).
API = {
    "apexgpu_create": (_int, [_i64, _i64, _i64, _int, _int, _P(_vp)]),
    "apexgpu_destroy": (None, [_vp]),
    "apexgpu_last_error": (_str, [_vp]),
    "apexgpu_version": (_str, []),
    "apexgpu_trim_host_cache": (_int, [_P(_i64)]),
    "apexgpu_host_cache_bytes": (_i64, []),
    "apexgpu_set_structure": (_int, [_vp] + [_vp] * 9 + [_dbl]),
    "apexgpu_set_cg_params": (_int, [_vp, _int, _dbl]),
    "apexgpu_set_params": (_int, [_vp, _vp, _vp, _vp]),
    "apexgpu_set_loss": (_int, [_vp, _int, _dbl, _dbl]),
    "apexgpu_get_loss": (_int, [_vp, _P(_int), _P(_dbl * 2)]),
    "apexgpu_set_pose_priors": (_int, [_vp, _i64, _vp, _vp, _vp, _vp]),
    "apexgpu_set_intrinsic_priors": (_int, [_vp, _i64, _vp, _vp, _vp, _vp]),
    "apexgpu_get_prior_residual": (_int, [_vp, _vp, _vp]),
    "apexgpu_get_params": (_int, [_vp, _vp, _vp, _vp]),
    "apexgpu_cost": (_int, [_vp, _P(_dbl)]),
    "apexgpu_solve_augmented": (_int, [_vp, _dbl, _int, _vp, _vp]),
    "apexgpu_assemble": (_int, [_vp, _dbl]),
    "apexgpu_step_stats": (_int, [_vp, _P(_dbl * 3)]),
    "apexgpu_eval_step": (_int, [_vp, _P(_dbl)]),
    "apexgpu_commit_step": (_int, [_vp]),
    "apexgpu_discard_step": (_int, [_vp]),
    "apexgpu_parameter_norm": (_int, [_vp, _P(_dbl)]),
    "apexgpu_column_norms": (_int, [_vp, _vp]),
    "apexgpu_set_column_scaling": (_int, [_vp, _vp]),
    "apexgpu_lm_optimize": (_int, [_vp, _P(LmConfigC)] + _opt),
    "apexgpu_get_residual": (_int, [_vp, _vp]),
    "apexgpu_get_jacobian_blocks": (_int, [_vp, _vp, _vp]),
    "apexgpu_get_schur": (_int, [_vp, _vp, _vp]),
    "apexgpu_camera_covariance": (_int, [_vp, _vp]),
    "apexgpu_covariance_stats": (_int, [_vp, _P(_dbl * 6), _vp, _int]),
    "apexgpu_landmark_covariance": (_int, [_vp, _vp]),
    "apexgpu_landmark_covariance_stats": (_int, [_vp, _P(_dbl * 4)]),
    "apexgpu_get_landmark_blocks": (_int, [_vp, _vp, _vp]),
    "apexgpu_debug_invert_blocks": (_int, [_int, _i64, _vp, _vp, _vp]),
    "apexgpu_get_hessian_csc": (_int, [_vp, _vp, _vp, _vp, _vp]),
    "apexgpu_schur_matvec": (_int, [_vp, _dbl, _vp, _vp, _vp]),
    "apexgpu_set_option": (_int, [_vp, _str, _int]),
    "apexgpu_enable_stage_timing": (_int, [_vp, _int]),
    "apexgpu_reset_stage_times": (_int, [_vp]),
    "apexgpu_stage_times": (_int, [_vp, _P(_dbl * NUM_STAGES), _P(_i64 * NUM_STAGES)]),
    "apexgpu_info": (_int, [_vp, _P(_dbl * 17)]),
    "apexgpu_variant_info": (_int, [_vp, _int, _P(_int), _str, _int]),
    "apexgpu_variant_costs": (_int, [_vp, _P(_dbl * 4)]),
    "apexgpu_counters": (_int, [_vp, _P(_i64 * 4)]),
    "apexgpu_debug_get_pair_records": (_int, [_vp, _vp, _i64]),
    "apexgpu_setup_times": (_int, [_vp, _vp, _vp]),
    "apexgpu_get_unique_id": (_int, [_vp]),
    "apexgpu_comm_init": (_int, [_vp, _int, _int, _vp]),
    "apexgpu_comm_init_shm": (_int, [_vp, _int, _int, _str]),
    "apexgpu_set_shard": (_int, [_vp, _int, _int]),
    "apexgpu_debug_lockstep_solve": (_int, [_vp, _int, _dbl]),
    "apexgpu_owned_landmarks": (_int, [_vp, _vp]),
    "apexgpu_debug_partition": (_int, [_int, _vp, _int, _vp]),
    "apexgpu_debug_check_schedule": (_int, [_int, _vp, _int, _int, _vp, _vp, _str, _int]),
    "apexgpu_debug_schedule_ops": (_int, [_int, _vp, _int, _int, _vp, _int, _vp, _int]),
    "apexgpu_debug_plan_lists": (_int, [_int, _vp, _int, _int, _vp, _int, _vp, _int]),
    "apexgpu_debug_sinv_lists": (_int, [_int, _vp, _vp, _int, _vp, _vp]),
    "apexgpu_debug_sinv_lists_direct": (_int, [_int, _vp, _int, _vp, _vp, _vp, _int, _vp, _str, _int]),
    "apexgpu_debug_tiles_create": (_int, [_int, _int, _vp, _vp, _P(_vp)]),
    "apexgpu_debug_tiles_pattern": (_int, [_vp, _vp, _vp]),
    "apexgpu_debug_tiles_set": (_int, [_vp, _vp, _int, _dbl, _int]),
    "apexgpu_debug_tiles_factor": (_int, [_vp, _P(_int)]),
    "apexgpu_debug_tiles_solve": (_int, [_vp, _int, _vp, _vp]),
    "apexgpu_debug_tiles_matvec": (_int, [_vp, _vp, _vp]),
    "apexgpu_debug_tiles_pcg": (_int, [_vp, _vp, _int, _dbl, _vp, _P(_int), _vp]),
    "apexgpu_debug_tiles_get": (_int, [_vp, _int, _vp, _P(_int)]),
    "apexgpu_debug_tiles_destroy": (None, [_vp]),
    "apexgpu_debug_host_structure": (_int, [_i64, _i64, _i64, _int, _vp, _vp, _int, _int, _vp, _vp, _vp, _vp, _vp]),
    "apexgpu_debug_pair_lists": (_int, [_i64, _i64, _i64, _int] + _pairs),
    "apexgpu_debug_pair_lists_queued": (_int, [_i64, _i64, _i64] + _pairs + [_vp]),
    "apexgpu_debug_pair_lists_queued_dc": (_int, [_i64, _i64, _i64, _int] + _pairs + [_vp]),
    "apexgpu_export_step": (_int, [_vp, _vp, _vp]),
    "apexgpu_shard_range": (_int, [_i64, _i64, _vp, _int, _int, _P(_i64), _P(_i64)]),
    "apexgpu_bal_open": (_int, [_str, _P(_vp)]),
    "apexgpu_bal_close": (None, [_vp]),
    "apexgpu_bal_last_error": (_str, []),
    "apexgpu_bal_sizes": (_int, [_vp, _P(_i64), _P(_i64), _P(_i64)]),
    "apexgpu_bal_raw": (_int, [_vp] * 6),
    "apexgpu_bal_variables": (_int, [_vp, _vp, _vp]),
    "apexgpu_reference_columns": (_int, [_i64, _i64, _vp, _vp, _vp]),
    # pose graphs: SE3, SE2, SO3 on one handle
    "apexgpu_pg_create": (_int, [_i64, _i64, _int, _P(_vp)]),
    "apexgpu_pg_create_se2": (_int, [_i64, _i64, _int, _P(_vp)]),
    "apexgpu_pg_create_so3": (_int, [_i64, _i64, _int, _P(_vp)]),
    "apexgpu_pg_manifold": (_int, [_vp, _P(_int * 3)]),
    "apexgpu_pg_destroy": (None, [_vp]),
    "apexgpu_pg_last_error": (_str, [_vp]),
    "apexgpu_pg_set_structure": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _dbl]),
    "apexgpu_pg_set_priors": (_int, [_vp, _i64, _vp, _vp, _vp]),
    "apexgpu_pg_get_prior_residual": (_int, [_vp, _vp]),
    "apexgpu_pg_set_loss": (_int, [_vp, _int, _dbl, _dbl]),
    "apexgpu_pg_get_loss": (_int, [_vp, _P(_int), _P(_dbl * 2)]),
    "apexgpu_pg_set_information": (_int, [_vp, _vp]),
    "apexgpu_pg_get_information": (_int, [_vp, _P(_int), _vp]),
    "apexgpu_loss_evaluate": (_int, [_int, _dbl, _dbl, _dbl, _P(_dbl * 6)]),
    "apexgpu_pg_set_params": (_int, [_vp, _vp]),
    "apexgpu_pg_get_params": (_int, [_vp, _vp]),
    "apexgpu_pg_cost": (_int, [_vp, _P(_dbl)]),
    "apexgpu_pg_solve_augmented": (_int, [_vp, _dbl, _vp, _vp]),
    "apexgpu_pg_step_stats": (_int, [_vp, _P(_dbl * 3)]),
    "apexgpu_pg_eval_step": (_int, [_vp, _P(_dbl)]),
    "apexgpu_pg_commit_step": (_int, [_vp]),
    "apexgpu_pg_discard_step": (_int, [_vp]),
    "apexgpu_pg_parameter_norm": (_int, [_vp, _P(_dbl)]),
    "apexgpu_pg_column_norms": (_int, [_vp, _vp]),
    "apexgpu_pg_set_column_scaling": (_int, [_vp, _vp]),
    "apexgpu_pg_lm_optimize": (_int, [_vp, _P(LmConfigC)] + _opt),
    "apexgpu_pg_jv_gram": (_int, [_vp, _vp, _vp, _P(_dbl * 3)]),
    "apexgpu_pg_dogleg_step": (_int, [_vp, _dbl, _dbl, _int, _P(_dbl * 8)]),
    "apexgpu_pg_gn_optimize": (_int, [_vp, _P(GnConfigC)] + _opt),
    "apexgpu_pg_dogleg_optimize": (_int, [_vp, _P(DlConfigC)] + _opt),
    "apexgpu_jv_gram": (_int, [_vp, _vp, _vp, _P(_dbl * 3)]),
    "apexgpu_dogleg_step": (_int, [_vp, _dbl, _dbl, _int, _P(_dbl * 8)]),
    "apexgpu_dogleg_optimize": (_int, [_vp, _P(DlConfigC)] + _opt),
    "apexgpu_pg_get_residual": (_int, [_vp, _vp]),
    "apexgpu_pg_get_jacobian_blocks": (_int, [_vp, _vp]),
    "apexgpu_pg_get_hessian": (_int, [_vp, _dbl, _vp, _vp]),
    "apexgpu_pg_covariance": (_int, [_vp, _vp]),
    "apexgpu_pg_covariance_stats": (_int, [_vp, _P(_dbl * 6), _vp, _int]),
    "apexgpu_pg_set_option": (_int, [_vp, _str, _int]),
    "apexgpu_pg_enable_stage_timing": (_int, [_vp, _int]),
    "apexgpu_pg_reset_stage_times": (_int, [_vp]),
    "apexgpu_pg_stage_times": (_int, [_vp, _P(_dbl * PG_NUM_STAGES), _P(_i64 * PG_NUM_STAGES)]),
    "apexgpu_pg_info": (_int, [_vp, _P(_dbl * 9)]),
    "apexgpu_pg_counters": (_int, [_vp, _P(_i64 * 4)]),
    "apexgpu_g2o_open": (_int, [_str, _P(_vp)]),
    "apexgpu_g2o_close": (None, [_vp]),
    "apexgpu_g2o_last_error": (_str, []),
    "apexgpu_g2o_sizes": (_int, [_vp] + [_P(_i64)] * 4),
    "apexgpu_g2o_raw": (_int, [_vp] * 7),
    "apexgpu_g2o_problem": (_int, [_vp] * 8),
    "apexgpu_pose_graph_columns": (_int, [_i64, _vp, _vp]),
    "apexgpu_g2o_raw_se2": (_int, [_vp] * 7),
    "apexgpu_g2o_problem_se2": (_int, [_vp] * 8),
    "apexgpu_pose_graph_columns_se2": (_int, [_i64, _vp, _vp]),
    "apexgpu_g2o_problem_information": (_int, [_vp, _int, _vp]),
}
SYMBOLS = tuple(API)

_lib = None


def load() -> C.CDLL:
    """Load libapexgpu.so (built by __graft_entry__.build() / `make -C apex-solver_amd/csrc`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()')."
            " There is no CPU fallback."
        )
    L = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in API.items():
        f = getattr(L, name)
        f.restype, f.argtypes = restype, argtypes
    _lib = L
    return L


def tile_partition(present: np.ndarray, world: int):
    """Owner rank of every tile column (-1: shared top) for a distributed plan of `world` ranks; host arithmetic in the
    library, no GPU needed.  present: (nt, nt) lower-triangular 0/1 structure."""
    L = load()
    pr = np.ascontiguousarray(present, dtype=np.uint8)
    nt = pr.shape[0]
    owner = np.zeros(nt, dtype=np.int32)
    n_top = L.apexgpu_debug_partition(nt, pr.ctypes.data_as(C.c_void_p), int(world), owner.ctypes.data_as(C.c_void_p))
    if n_top < 0:
        raise LinAlgError(n_top, "apexgpu_debug_partition")
    return owner, n_top


def check_schedule(present: np.ndarray, world: int = 1, rank: int = 0, two_side: int = 1, overlap: int = 1, split_u1: int = 4,
                   flood_gate: int = 256, factor_flow: int = -1, factor_flow_rows: int = 24, old_idle_level_bug: bool = False,
                   drop_wait: int = -1) -> dict:
    """Host-only race check of the factorisation's launch sequence for one tile structure (apexgpu_debug_check_schedule)."""
    L = load()
    pr = np.ascontiguousarray(present, dtype=np.uint8)
    nt = pr.shape[0]
    opts = np.array([two_side, overlap, split_u1, flood_gate, factor_flow, factor_flow_rows, int(old_idle_level_bug), drop_wait], dtype=np.int32)
    out = np.zeros(8, dtype=np.int64)
    msg = C.create_string_buffer(512)
    rc = L.apexgpu_debug_check_schedule(nt, pr.ctypes.data_as(C.c_void_p), int(world), int(rank), opts.ctypes.data_as(C.c_void_p),
                                        out.ctypes.data_as(C.c_void_p), msg, 512)
    if rc < 0:
        raise LinAlgError(rc, "apexgpu_debug_check_schedule: " + msg.value.decode())
    return dict(levels=rc, calls=int(out[0]), launches=int(out[1]), violations=int(out[2]) + int(out[3]), violations_top=int(out[3]),
                flow_units=int(out[4]), flow_groups=int(out[5]), waits=int(out[6]), dropped=bool(out[7]), first=msg.value.decode())


def schedule_ops(present: np.ndarray, phase: int = 0, world: int = 1, rank: int = 0, two_side: int = 1, overlap: int = 1, split_u1: int = 4,
                 flood_gate: int = 256, factor_flow: int = -1, factor_flow_rows: int = 24) -> np.ndarray:
    """Host only: the factorisation's launch sequence of one phase as rows {op, stream, event, list, first, count}
    (apexgpu_debug_schedule_ops; options as check_schedule)."""
    L = load()
    pr = np.ascontiguousarray(present, dtype=np.uint8)
    nt = pr.shape[0]
    opts = np.array([two_side, overlap, split_u1, flood_gate, factor_flow, factor_flow_rows, 0, -1], dtype=np.int32)
    args = (nt, pr.ctypes.data_as(C.c_void_p), int(world), int(rank), opts.ctypes.data_as(C.c_void_p), int(phase))
    n = L.apexgpu_debug_schedule_ops(*args, None, 0)
    if n < 0:
        raise LinAlgError(n, "apexgpu_debug_schedule_ops")
    rows = np.zeros((n, 6), dtype=np.int64)
    if n and L.apexgpu_debug_schedule_ops(*args, rows.ctypes.data_as(C.c_void_p), n) != n:
        raise LinAlgError(-6, "apexgpu_debug_schedule_ops")
    return rows


# the tables of apexgpu_debug_plan_lists (include/apexgpu.h), in its numbering: name, columns of a row
PLAN_TABLES = (("scalars", 23), ("slots", 3), ("columns", 4), ("owner_ranges", 5), ("levels", 9), ("fwd_cut", 2), ("upd_rounds", 2),
               ("bwd_step", 1), ("potrf", 5), ("panel", 7), ("upd", 7), ("fwd", 6), ("bwd", 6), ("flow_fwd", 10), ("flow_bwd", 10),
               ("units", 16), ("sym_row_ptr", 1), ("sym_entries", 3), ("sym_tiles", 3), ("group_cols", 2))


def plan_lists(present: np.ndarray, which: str, world: int = 1, rank: int = 0, two_side: int = 1, overlap: int = 1, split_u1: int = 4,
               flood_gate: int = 256, factor_flow: int = -1, factor_flow_rows: int = 24) -> np.ndarray:
    """Host only: one table of the plan's structure and task lists, tiles by name (apexgpu_debug_plan_lists; `which` a name of
    PLAN_TABLES; options as check_schedule)."""
    L = load()
    pr = np.ascontiguousarray(present, dtype=np.uint8)
    w = [n for n, _ in PLAN_TABLES].index(which)
    opts = np.array([two_side, overlap, split_u1, flood_gate, factor_flow, factor_flow_rows, 0, -1], dtype=np.int32)
    args = (pr.shape[0], pr.ctypes.data_as(C.c_void_p), int(world), int(rank), opts.ctypes.data_as(C.c_void_p), w)
    n = L.apexgpu_debug_plan_lists(*args, None, 0)
    if n < 0:
        raise LinAlgError(n, "apexgpu_debug_plan_lists")
    rows = np.zeros((n, PLAN_TABLES[w][1]), dtype=np.int64)
    if n and L.apexgpu_debug_plan_lists(*args, rows.ctypes.data_as(C.c_void_p), n) != n:
        raise LinAlgError(-6, "apexgpu_debug_plan_lists")
    return rows


def _sinv_rows(call, what, msg=None):
    counts = np.zeros(4, dtype=np.int64)
    n = call(None, 0, ptr(counts))
    if n < 0:
        raise LinAlgError(n, what + (": " + msg.value.decode() if msg is not None else ""))
    rows = np.zeros((n, 6), dtype=np.int64)
    if n and call(ptr(rows), n, ptr(counts)) != n:
        raise LinAlgError(-6, what)
    return rows, counts


def sinv_lists(present: np.ndarray, with_slots: bool = False):
    """Host only: the task lists of the selected inversion of the single-rank plan of one tile structure, tiles by name
    (apexgpu_debug_sinv_lists): (rows, counts) with rows {kind, group, C.array, C.tile, first, count} per task, then
    {3, A.array, A.tile, B.array, B.tile, op} per product; counts = products per kind, Y tiles of the largest group.
    with_slots: (rows, counts, slot), slot the plan's (nt, nt) slot map."""
    L = load()
    pr = np.ascontiguousarray(present, dtype=np.uint8)
    slot = np.zeros(pr.shape, dtype=np.int32)
    out = _sinv_rows(lambda rows, n, counts: L.apexgpu_debug_sinv_lists(pr.shape[0], ptr(pr), rows, n, counts, ptr(slot)), "apexgpu_debug_sinv_lists")
    return out + (slot,) if with_slots else out


def sinv_lists_direct(slot: np.ndarray, groups):
    """The same from a caller-given slot map ((nt, nt), -1 where absent) and level groups (lists of tile columns, leaves
    first), with no plan in between (apexgpu_debug_sinv_lists_direct); a refusal raises InvalidState with the builder's
    message."""
    L = load()
    sl = np.ascontiguousarray(slot, dtype=np.int32)
    gp = np.cumsum([0] + [len(g) for g in groups]).astype(np.int32)
    gc = np.array([c for g in groups for c in g] + [0], dtype=np.int32)   # (never empty: a pointer to pass)
    msg = C.create_string_buffer(512)
    return _sinv_rows(lambda rows, n, counts: L.apexgpu_debug_sinv_lists_direct(sl.shape[0], ptr(sl), len(groups), ptr(gp), ptr(gc), rows, n, counts, msg, 512),
                      "apexgpu_debug_sinv_lists_direct", msg)


HOST_STRUCTURE_STATS = ("tile_rows", "hub_cameras", "border_tiles", "touched_tiles", "tiles", "etree_levels", "top_columns",
                        "tree_sharded", "s_order", "s_lists", "s_plan", "s_schur_lists", "s_uploads", "s_total", "pair_contributions",
                        "pair_blocks")


def host_structure(n_cam: int, n_pt: int, cam_idx: np.ndarray, pt_idx: np.ndarray, mode: int = 1, rank: int = 0, world: int = 1,
                   nested_dissection: int = 1, hubs_last: int = 1, dist_factor: int = 1, tree_sharding: int = 1, schur_form: int = 3):
    """Host only: what apexgpu_set_structure derives from the observation list before it touches the device."""
    ci = np.ascontiguousarray(cam_idx, dtype=np.uint32); pi = np.ascontiguousarray(pt_idx, dtype=np.uint32)
    opts = np.array([nested_dissection, hubs_last, dist_factor, tree_sharding, schur_form], dtype=np.int32)
    stats = np.zeros(16); dc = 9 if mode in (1, 4, 5, 6) else 6
    nt = (n_cam * dc + 143) // 144
    cmap = np.zeros(n_cam, dtype=np.int32); owned = np.zeros(n_pt, dtype=np.uint8); towner = np.zeros(nt, dtype=np.int32)
    rc = load().apexgpu_debug_host_structure(n_cam, n_pt, len(ci), mode, ptr(ci), ptr(pi), rank, world, ptr(opts), ptr(stats),
                                             ptr(cmap), ptr(owned), ptr(towner))
    if rc != 0:
        raise LinAlgError(rc, "apexgpu_debug_host_structure failed")
    out = dict(zip(HOST_STRUCTURE_STATS, stats.tolist()))
    out.update(cmap=cmap, owned=owned.astype(bool), tile_owner=towner)
    return out


def pair_lists(n_cam: int, n_pt: int, dc: int, cam_idx: np.ndarray, pt_idx: np.ndarray):
    """Host only: the sorted camera-pair lists of the default Schur reduction (apexgpu_debug_pair_lists)."""
    ci = np.ascontiguousarray(cam_idx, dtype=np.uint32); pi = np.ascontiguousarray(pt_idx, dtype=np.uint32)
    counts = np.zeros(4, dtype=np.int64)
    L = load()
    rc = L.apexgpu_debug_pair_lists(n_cam, n_pt, len(ci), dc, ptr(ci), ptr(pi), ptr(counts), None, None, None, None, None)
    if rc != 0:
        raise LinAlgError(rc, "apexgpu_debug_pair_lists failed")
    recs = np.zeros((counts[0], 4), dtype=np.uint32); chunks = np.zeros((counts[1], 2), dtype=np.int32)
    blocks = np.zeros((counts[2], 4), dtype=np.int64); tasks = np.zeros((counts[3], 2), dtype=np.int32)
    o_index = np.zeros(len(ci), dtype=np.int32)
    rc = L.apexgpu_debug_pair_lists(n_cam, n_pt, len(ci), dc, ptr(ci), ptr(pi), ptr(counts), ptr(recs), ptr(chunks), ptr(blocks),
                                    ptr(tasks), ptr(o_index))
    if rc != 0:
        raise LinAlgError(rc, "apexgpu_debug_pair_lists failed")
    return dict(recs=recs, chunks=chunks, blocks=blocks, tasks=tasks, o_index=o_index)


def pair_lists_queued(n_cam: int, n_pt: int, cam_idx: np.ndarray, pt_idx: np.ndarray, dc: int = 9):
    """Host only: the same pairs in the queued layout ("schur_form" 4; apexgpu_debug_pair_lists_queued_dc): nine columns per
    camera = seven queues of nine pairs per chunk, six columns = sixteen queues of four."""
    ci = np.ascontiguousarray(cam_idx, dtype=np.uint32); pi = np.ascontiguousarray(pt_idx, dtype=np.uint32)
    counts = np.zeros(4, dtype=np.int64)
    L = load()
    nd = 8 if dc == 9 else 17
    rc = L.apexgpu_debug_pair_lists_queued_dc(n_cam, n_pt, len(ci), dc, ptr(ci), ptr(pi), ptr(counts), None, None, None, None, None, None)
    if rc != 0:
        raise LinAlgError(rc, "apexgpu_debug_pair_lists_queued_dc failed")
    recs = np.zeros((counts[0], 4), dtype=np.uint32); chunks = np.zeros((counts[1], 2), dtype=np.int32)
    blocks = np.zeros((counts[2], 4), dtype=np.int64); tasks = np.zeros((counts[3], 2), dtype=np.int32)
    o_index = np.zeros(len(ci), dtype=np.int32); qdesc = np.zeros((counts[1] * nd, 3), dtype=np.int64)
    rc = L.apexgpu_debug_pair_lists_queued_dc(n_cam, n_pt, len(ci), dc, ptr(ci), ptr(pi), ptr(counts), ptr(recs), ptr(chunks), ptr(blocks),
                                              ptr(tasks), ptr(o_index), ptr(qdesc))
    if rc != 0:
        raise LinAlgError(rc, "apexgpu_debug_pair_lists_queued_dc failed")
    return dict(recs=recs, chunks=chunks, blocks=blocks, tasks=tasks, o_index=o_index, qdesc=qdesc.reshape(-1, nd, 3), dc=dc)


def invert_blocks_on_device(blocks: np.ndarray, device: int = 0):
    """The device's eigenvalue-gated 3x3 inverse (row A9) on caller-supplied blocks [n,3,3] -> (inverses, ok)."""
    b = np.ascontiguousarray(blocks, dtype=np.float64).reshape(-1, 9)
    out = np.empty_like(b)
    ok = np.zeros(len(b), dtype=np.int32)
    rc = load().apexgpu_debug_invert_blocks(int(device), len(b), ptr(b), ptr(out), ptr(ok))
    if rc != 0:
        raise LinAlgError(rc, "apexgpu_debug_invert_blocks failed")
    return out.reshape(-1, 3, 3), ok.astype(bool)


def shard_range(pt_idx: np.ndarray, n_pt: int, rank: int, world: int) -> tuple[int, int]:
    """Landmark range owned by `rank` (host arithmetic in the library, no GPU needed)."""
    L = load()
    a = np.ascontiguousarray(pt_idx, dtype=np.uint32)
    lo, hi = C.c_int64(), C.c_int64()
    rc = L.apexgpu_shard_range(n_pt, a.shape[0], a.ctypes.data_as(C.c_void_p), rank, world, C.byref(lo), C.byref(hi))
    if rc != 0:
        raise LinAlgError(rc, "apexgpu_shard_range")
    return lo.value, hi.value


def ptr(a):
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.c_void_p)


class _HandleBase:
    """Owner of one library handle of the kind whose calls start with _PREFIX: L the library, h the handle."""

    _PREFIX = ""

    def __init__(self):
        self.L = load()
        self.h = C.c_void_p()

    def _fn(self, name: str):
        """The call of this handle's kind by its unprefixed name: apexgpu_cost / apexgpu_pg_cost for "cost"."""
        return getattr(self.L, self._PREFIX + name)

    def _call(self, name: str, *args):
        """That call on this handle; raises what it refuses."""
        rc = getattr(self.L, self._PREFIX + name)(self.h, *args)
        if rc != 0:
            self.check(rc)

    def check(self, rc: int):
        if rc != 0:
            raise LinAlgError(rc, self._fn("last_error")(self.h).decode())

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self._fn("destroy")(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Handle(_HandleBase):
    """RAII wrapper of an apexgpu_solver*."""

    _PREFIX = "apexgpu_"

    def __init__(self, n_cam: int, n_pt: int, n_obs: int, mode: int, device: int = 0):
        super().__init__()
        rc = self.L.apexgpu_create(n_cam, n_pt, n_obs, mode, device, C.byref(self.h))
        if rc != 0:
            raise LinAlgError(rc, "apexgpu_create failed (no MI355X visible to HIP?)")
        self.n_cam, self.n_pt, self.n_obs, self.mode = n_cam, n_pt, n_obs, mode


class PgHandle(_HandleBase):
    """RAII wrapper of an apexgpu_pg_solver*."""

    _PREFIX = "apexgpu_pg_"

    def __init__(self, n_vertices: int, n_edges: int, device: int = 0, manifold: int = MANIFOLD_SE3):
        super().__init__()
        if manifold not in MANIFOLD_SIZES:
            raise ValueError(f"unknown manifold {manifold!r}")
        create = {MANIFOLD_SE3: self.L.apexgpu_pg_create, MANIFOLD_SE2: self.L.apexgpu_pg_create_se2,
                  MANIFOLD_SO3: self.L.apexgpu_pg_create_so3}[manifold]
        rc = create(n_vertices, n_edges, device, C.byref(self.h))
        if rc != 0:
            raise LinAlgError(rc, "apexgpu_pg_create failed (no MI355X visible to HIP?)")
        self.n_vertices, self.n_edges = n_vertices, n_edges
        self.manifold = manifold
        self.ambient, self.dof = MANIFOLD_SIZES[manifold]   # SO3: 4-wide poses / measurements / priors, 3-wide steps and masks


class TileCholesky:
    """Tests only: the single-GPU tile Cholesky (TilePlan) on a matrix the caller chooses (apexgpu_debug_tiles_*).

    present: (nt, nt) lower-triangular 0/1 tile structure in the final order (nothing is reordered).  Tiles are 144 x 144
    row-major; the arrays below are indexed by slot (`slot[I, J]`, -1 outside the filled pattern)."""

    OPTS = ("graphs", "factor_flow", "factor_flow_rows", "tri_dataflow", "update_overlap", "split_u1", "two_side", "flood_gate")
    DEFAULTS = dict(graphs=1, factor_flow=-1, factor_flow_rows=24, tri_dataflow=1, update_overlap=1, split_u1=4, two_side=1, flood_gate=256)

    def __init__(self, present: np.ndarray, device: int = 0, diag_update_lower: int = 1, **opts):
        """diag_update_lower 0: the updates of diagonal tiles compute all nine 48 x 48 blocks (bit 1 of opts[0])."""
        unknown = set(opts) - set(self.OPTS)
        if unknown:
            raise ValueError(f"unknown options {sorted(unknown)}")
        self.L = load()
        self.h = C.c_void_p()
        pr = np.ascontiguousarray(present, dtype=np.uint8)
        self.nt = int(pr.shape[0])
        o = dict(self.DEFAULTS, **opts)
        ov = np.array([o[k] for k in self.OPTS], dtype=np.int32)
        ov[0] = (1 if o["graphs"] else 0) | (0 if diag_update_lower else 2)
        rc = self.L.apexgpu_debug_tiles_create(int(device), self.nt, ptr(pr), ptr(ov), C.byref(self.h))
        if rc != 0:
            raise LinAlgError(rc, "apexgpu_debug_tiles_create failed")
        self.slot = np.zeros((self.nt, self.nt), dtype=np.int32)
        info = np.zeros(8, dtype=np.int64)
        self._check(self.L.apexgpu_debug_tiles_pattern(self.h, ptr(self.slot), ptr(info)), "pattern")
        self.n_slots, self.n_touched, self.levels, self.first_writers_flagged = int(info[0]), int(info[1]), int(info[2]), bool(info[3])
        self.flow_units, self.flow_groups, self.n_pad, self.nb = int(info[4]), int(info[5]), int(info[6]), int(info[7])

    def _check(self, rc: int, what: str):
        if rc != 0:
            raise LinAlgError(rc, f"apexgpu_debug_tiles_{what} failed")

    def set(self, touched: np.ndarray, n_valid: int | None = None, add_diag: float = 0.0, fill_mode: int = 0):
        """touched: (n_touched, 144, 144) tiles in slot order, diagonal tiles in full (symmetric)."""
        t = np.ascontiguousarray(touched, dtype=np.float64)
        assert t.shape == (self.n_touched, self.nb, self.nb), t.shape
        nv = self.n_pad if n_valid is None else int(n_valid)
        self._check(self.L.apexgpu_debug_tiles_set(self.h, ptr(t), nv, float(add_diag), int(fill_mode)), "set")

    def factor(self) -> int:
        """0, or (a failed tile column + 1)."""
        f = C.c_int(0)
        self._check(self.L.apexgpu_debug_tiles_factor(self.h, C.byref(f)), "factor")
        return f.value

    def solve(self, rhs: np.ndarray) -> np.ndarray:
        b = np.ascontiguousarray(np.atleast_2d(rhs), dtype=np.float64)
        assert b.shape[1] == self.n_pad
        x = np.empty_like(b)
        self._check(self.L.apexgpu_debug_tiles_solve(self.h, b.shape[0], ptr(b), ptr(x)), "solve")
        return x.reshape(np.shape(rhs))

    def matvec(self, x: np.ndarray) -> np.ndarray:
        xv = np.ascontiguousarray(x, dtype=np.float64)
        y = np.empty_like(xv)
        self._check(self.L.apexgpu_debug_tiles_matvec(self.h, ptr(xv), ptr(y)), "matvec")
        return y

    def pcg(self, rhs: np.ndarray, max_iter: int, tol: float):
        """Jacobi-PCG on the unfactored tiles (TilePlan::pcg): (x, iterations, scal) with scal = the loop's device scalars
        [rz_old, p.Ap, r.r, r.z, frozen] after the call.  Voids the factor: solve() raises InvalidState until factor()."""
        b = np.ascontiguousarray(rhs, dtype=np.float64)
        assert b.shape == (self.n_pad,), b.shape
        x, scal, it = np.empty_like(b), np.empty(5), C.c_int(0)
        self._check(self.L.apexgpu_debug_tiles_pcg(self.h, ptr(b), int(max_iter), float(tol), ptr(x), C.byref(it), ptr(scal)), "pcg")
        return x, it.value, scal

    def get(self, which: str) -> np.ndarray:
        """"tiles" (raw), "L" (the tiles with the diagonal tiles masked to their lower triangle), "Linv" ((nt, 144, 144)),
        "Z" (the selected inverse on the pattern of L; self.z_recomputed then says whether this call computed it or found
        it current)."""
        k = {"tiles": 0, "L": 0, "Linv": 1, "Z": 2}[which]
        out = np.empty(((self.nt if k == 1 else self.n_slots), self.nb, self.nb))
        rec = C.c_int(0)
        self._check(self.L.apexgpu_debug_tiles_get(self.h, k, ptr(out), C.byref(rec)), "get")
        if k == 2:
            self.z_recomputed = bool(rec.value)
        if which == "L":   # a factorised diagonal tile keeps the assembled matrix in its 16 x 16 blocks right of the diagonal
            low = np.tril(np.ones((self.nb, self.nb), dtype=bool))
            for K in range(self.nt):
                out[self.slot[K, K]] = np.where(low, out[self.slot[K, K]], 0.0)
        return out

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.L.apexgpu_debug_tiles_destroy(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
