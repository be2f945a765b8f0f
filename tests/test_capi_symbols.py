"""The C-ABI library loads and exports every symbol include/apexgpu.h declares (no GPU needed;
no compute call is made)."""
import ctypes as C
import os
import re

import pytest

import apex_solver_amd as pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    src = open(os.path.join(ROOT, "include", "apexgpu.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(apexgpu_[a-z_0-9]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    if not os.path.exists(pkg.capi.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    L = pkg.capi.load()
    names = header_symbols()
    assert len(names) >= 25
    for n in names:
        assert hasattr(L, n), f"libapexgpu.so does not export {n}"
    assert sorted(pkg.capi.SYMBOLS) == names  # the Python binding covers the whole header
    assert b"gfx950" in L.apexgpu_version()


def test_every_symbol_has_its_signature_from_the_one_table():
    """load() is a loop over capi.API: every name of SYMBOLS has explicit argtypes (a missing one lets ctypes pass a Python int
    as a C int, whatever the parameter is) and the table's restype, and SYMBOLS is the table's key set."""
    capi = pkg.capi
    L = capi.load()
    assert tuple(capi.SYMBOLS) == tuple(capi.API) and len(set(capi.SYMBOLS)) == len(capi.SYMBOLS)
    for n in capi.SYMBOLS:
        restype, argtypes = capi.API[n]
        f = getattr(L, n)
        assert f.argtypes is not None and list(f.argtypes) == list(argtypes), n
        assert f.restype is restype and restype in (None, C.c_int, C.c_int64, C.c_char_p), n
    # three int64, an int, then nine pointers (include/apexgpu.h)
    assert list(L.apexgpu_debug_pair_lists_queued_dc.argtypes) == [C.c_int64] * 3 + [C.c_int] + [C.c_void_p] * 9
    for n in ("apexgpu_version", "apexgpu_bal_last_error", "apexgpu_g2o_last_error", "apexgpu_host_cache_bytes"):
        assert list(getattr(L, n).argtypes) == [], n


def header_handle_entries():
    """{name: 'handle' | 'array'} for every declaration of include/apexgpu.h whose first parameter is a solver, pose-graph or
    tiles handle, or an array of such handles."""
    src = open(os.path.join(ROOT, "include", "apexgpu.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    found = re.findall(r"\b(apexgpu_[a-z_0-9]+)\s*\(\s*(?:const\s+)?apexgpu_(?:solver|pg_solver|tiles)\s*(\*+)\s*\w+\s*[,)]", src)
    return {name: ("handle" if stars == "*" else "array") for name, stars in found}


def null_handle_answers(entries):
    """{name: what the loaded library answers} for the call list of test_null_handle_on_every_entry."""
    capi = pkg.capi
    L = capi.load()
    got = {}
    for n in sorted(entries):
        args = [None if issubclass(t, (C.c_void_p, C.c_char_p, C._Pointer)) else 0 for t in capi.API[n][1]]
        assert args[0] is None, n
        r = getattr(L, n)(*args)
        got[n] = r.decode() if isinstance(r, bytes) else r
    return got


def test_null_handle_on_every_entry():
    """Every entry that takes a handle, called with a NULL handle, NULL for every pointer and 0 for every scalar, answers what
    the library answered before the entries went through one helper (tests/golden/capi_null_handle.json, recorded from that
    build with this call list): APEXGPU_ERR_INVALID_STATE from the solver and pose-graph entries, APEXGPU_ERR_INVALID_INPUT
    from the apexgpu_debug_tiles_* entries and from the lockstep solve's NULL array, "invalid handle" from the two
    *_last_error calls, nothing from the destroy calls.  No device is needed: the handle is looked at first."""
    import json

    entries = header_handle_entries()
    assert len(entries) >= 90 and entries["apexgpu_debug_lockstep_solve"] == "array" and "apexgpu_debug_tiles_get" in entries
    assert not [n for n in entries if n.endswith("_create") or "_create_" in n]   # (their handle is an output, never the first parameter)
    got = null_handle_answers(entries)
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "capi_null_handle.json")))
    assert sorted(want) == sorted(got)
    assert got == want, {n: (got[n], want[n]) for n in got if got[n] != want[n]}
    # ... and what the golden file holds is what reading the earlier code gives
    for n, v in want.items():
        if n.endswith("destroy"):
            assert v is None, n
        elif n.endswith("last_error"):
            assert v == "invalid handle", n
        else:
            assert v == (-5 if n.startswith("apexgpu_debug_tiles_") or entries[n] == "array" else -6), (n, v)


def test_struct_layouts_match_header():
    # apexgpu_lm_config: int + 11 doubles + int (with padding) ; apexgpu_lm_iter: 8 doubles
    assert C.sizeof(pkg.capi.LmIterC) == 64
    assert C.sizeof(pkg.capi.LmConfigC) == 8 + 11 * 8 + 8
    assert C.sizeof(pkg.capi.LmResultC) == 8 + 5 * 8 + 16


def test_product_fails_loudly_without_gpu():
    """No CPU fallback: without a visible MI355X the handle cannot even be created."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    with pytest.raises(pkg.capi.LinAlgError) as e:
        pkg.capi.Handle(4, 10, 30, 1, 0)
    assert e.value.kind == "DeviceError"


def test_product_does_not_import_the_oracle():
    """oracle/ is test infrastructure: nothing under apex-solver_amd/ may reference it."""
    pk = os.path.join(ROOT, "apex-solver_amd")
    for dp, _, files in os.walk(pk):
        for f in files:
            if f.endswith((".py", ".hip", ".cpp", ".h", ".hpp")):
                txt = open(os.path.join(dp, f), errors="ignore").read()
                assert "oracle" not in txt.lower() or f == "ba_device.hpp", os.path.join(dp, f)


def test_host_block_cache_trims():
    """apexgpu_trim_host_cache answers without a GPU (nothing kept in a fresh process: 0 bytes) -- the set-up's host blocks
    are kept by the process for the next handle and this call hands them back."""
    import ctypes as C

    from apex_solver_amd import capi

    L = capi.load()
    n = C.c_int64(-1)
    assert L.apexgpu_trim_host_cache(C.byref(n)) == 0 and n.value >= 0
    assert L.apexgpu_trim_host_cache(None) == 0
