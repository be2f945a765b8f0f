"""The Python front end's surface and the condition its shared solver base rests on (no GPU).

tests/golden/frontend_surface.json was recorded by tools/record_frontend_surface.py from the commit BEFORE the two solver
classes got a common base (handle_solver.HandleSolver over capi._HandleBase): the names GpuSchurComplementSolver,
GpuSparseCholeskySolver, capi.Handle, capi.PgHandle, LevenbergMarquardt and DogLeg show and the signature of every callable.
Never re-record with the code under test."""
import ctypes as C
import importlib.util
import inspect
import json
import os
import re

import pytest

from apex_solver_amd import capi, handle_solver, pose_graph, solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_frontend_surface", os.path.join(ROOT, "tools", "record_frontend_surface.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

# instance attributes that exist from construction on where they used to appear with initialize_structure
SINCE_CONSTRUCTION = {"GpuSchurComplementSolver": ["setup_wall"]}


def test_surface_is_the_recorded_one():
    with open(rec.GOLDEN) as f:
        want = json.load(f)
    got = rec.surface()
    assert sorted(got) == sorted(want)
    for cls in want:
        assert got[cls]["class"] == want[cls]["class"], cls
        assert got[cls]["instance"] == sorted(want[cls]["instance"] + SINCE_CONSTRUCTION.get(cls, [])), cls
    assert want["GpuSchurComplementSolver"]["class"]["_need"] and "_h" in want["GpuSparseCholeskySolver"]["instance"]


def shared_calls():
    """Every unprefixed name handle_solver.py and capi._HandleBase resolve through a handle's prefix, read from their source."""
    src = inspect.getsource(handle_solver) + inspect.getsource(capi._HandleBase)
    return sorted(set(re.findall(r"\b_(?:call|fn|optimize)\(\"(\w+)\"", src)))


def test_shared_calls_have_one_signature_under_both_prefixes():
    """What lets one body serve both solvers: apexgpu_<name> and apexgpu_pg_<name> both exist and take the same arguments.
    Not in that table: stage_times, whose two arrays have the solver's own number of stages (HandleSolver sizes them by
    _STAGE_NAMES, so the one body still fits both), and solve_augmented, which takes a variant for bundle adjustment only and
    stays with the two solver classes."""
    names = shared_calls()
    assert len(names) >= 20 and {"cost", "lm_optimize", "dogleg_step", "destroy", "last_error", "stage_times"} <= set(names), names
    assert "solve_augmented" not in names
    for n in names:
        ba, pg = capi.API["apexgpu_" + n], capi.API["apexgpu_pg_" + n]
        if n == "stage_times":
            assert ba != pg and len(capi.STAGE_NAMES) == capi.NUM_STAGES and len(capi.PG_STAGE_NAMES) == capi.PG_NUM_STAGES
            assert ba[1][1:] == [C.POINTER(C.c_double * capi.NUM_STAGES), C.POINTER(C.c_int64 * capi.NUM_STAGES)]
            assert pg[1][1:] == [C.POINTER(C.c_double * capi.PG_NUM_STAGES), C.POINTER(C.c_int64 * capi.PG_NUM_STAGES)]
        else:
            assert ba == pg, n
    assert capi.API["apexgpu_solve_augmented"] != capi.API["apexgpu_pg_solve_augmented"]
    assert solver.GpuSchurComplementSolver._STAGE_NAMES == capi.STAGE_NAMES
    assert pose_graph.GpuSparseCholeskySolver._STAGE_NAMES == capi.PG_STAGE_NAMES


# every method of the shared base that reaches the handle, with arguments that would be valid on a built solver
SHARED_METHODS = [
    ("set_loss", (None,)), ("get_loss", ()), ("compute_cost", ()), ("solve_normal_equation", ()), ("compute_column_norms", ()),
    ("apply_column_scaling", (None,)), ("step_stats", ()), ("eval_step", ()), ("commit_step", ()), ("discard_step", ()),
    ("parameter_norm", ()), ("covariance_stats", ()), ("counters", ()), ("set_option", ("graphs", 1)), ("enable_stage_timing", ()),
    ("reset_stage_times", ()), ("stage_times", ()), ("lm_optimize", (solver.LevenbergMarquardtConfig(),)),
    ("dogleg_optimize", (pose_graph.DogLegConfig(),)), ("dogleg_step", (1e-4, 1.0)), ("jv_gram", ([0.0], [0.0])), ("_need", ()),
]


@pytest.mark.parametrize("cls,code", [(solver.GpuSchurComplementSolver, -5), (pose_graph.GpuSparseCholeskySolver, -6)])
def test_before_initialize_structure_every_shared_method_raises_the_class_own_error(cls, code):
    s = cls().with_option("graphs", 1)
    listed = {m for m, _ in SHARED_METHODS}
    for m, f in inspect.getmembers(handle_solver.HandleSolver, inspect.isfunction):   # none that reaches the handle is left out
        reaches = re.search(r"_need\(\)|_optimize\(|solve_augmented_equation\(", inspect.getsource(f))
        assert m in listed or m.startswith("_") or not reaches, m
    for m, args in SHARED_METHODS:
        with pytest.raises(capi.LinAlgError) as e:
            getattr(s, m)(*args)
        assert e.value.code == code and e.value.kind == capi.ERROR_NAMES[code], m
        assert str(e.value) == f"{capi.ERROR_NAMES[code]}: Block structure not built. Call initialize_structure() first.", m
    # what needs no handle: nothing kept, nothing to undo, nothing to close
    assert s.get_gradient() is None and s.apply_inverse_scaling(3.0) == 3.0 and s._h is None
    s.close()
