"""Records the surface of the Python front end as tests/golden/frontend_surface.json.  Per class: "class", the names dir() of
the class shows without a leading underscore, plus _need and __init__, each with its signature as a string where it is callable;
"instance", the further names a freshly constructed object carries (public ones and _h).  No GPU and no library: the two
handle classes are constructed over a stand-in library whose every call answers 0.
tests/test_frontend_surface_host.py holds the front end to the file; re-record only from a commit whose surface is the wanted one.
Usage: python tools/record_frontend_surface.py"""
import inspect
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "frontend_surface.json")
KEPT_PRIVATE = ("_need", "_h", "__init__")


class _AnswersZero:
    def __getattr__(self, name):
        return lambda *args: 0


def instances() -> dict:
    """One freshly constructed object per recorded class, by the class's recorded name."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from apex_solver_amd import capi, pose_graph, solver
    real, capi.load = capi.load, _AnswersZero
    try:
        handles = {"capi.Handle": capi.Handle(4, 10, 30, 1), "capi.PgHandle": capi.PgHandle(4, 3)}
    finally:
        capi.load = real
    return dict(handles, GpuSchurComplementSolver=solver.GpuSchurComplementSolver(), GpuSparseCholeskySolver=pose_graph.GpuSparseCholeskySolver(),
                LevenbergMarquardt=solver.LevenbergMarquardt(), DogLeg=solver.DogLeg())


def _kept(names):
    return sorted(n for n in names if not n.startswith("_") or n in KEPT_PRIVATE)


def surface() -> dict:
    out = {}
    for name, obj in instances().items():
        cls = type(obj)
        members = {n: getattr(cls, n) for n in _kept(dir(cls))}
        out[name] = {"class": {n: str(inspect.signature(m)) if callable(m) else None for n, m in members.items()},
                     "instance": _kept(set(dir(obj)) - set(dir(cls)))}
    return out


if __name__ == "__main__":
    with open(GOLDEN, "w") as f:
        json.dump(surface(), f, indent=1, sort_keys=True)
        f.write("\n")
