"""CPU: the time-surface entry is declared in include/xmaps.h, bound in _native.py with the header's arity, and the ctypes
struct has the header's fields (no compute calls)."""
import ctypes
import os
import re

from x_maps_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    src = open(os.path.join(ROOT, "include", "xmaps.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def _params(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", _header())
    assert m, f"{name} is not declared in include/xmaps.h"
    return [p.strip() for p in m.group(1).split(",")]


def test_header_declares_the_entry_and_the_binding_has_its_arity():
    for name in ("xm_surface_set_cloud_tables", "xm_process_time_surfaces"):
        params = _params(name)
        assert name in N.SYMBOLS, f"{name} is not bound in _native.py"
        res, args = N.SYMBOLS[name]
        assert res is ctypes.c_int and len(args) == len(params)
        for p, a in zip(params, args):  # pointers are pointers, ints are ints
            assert ("*" in p) == (a is ctypes.c_void_p), (name, p, a)
    assert [p.split()[-1].lstrip("*") for p in _params("xm_process_time_surfaces")] == \
        ["h", "surfaces", "dtype", "n_surfaces", "mem", "depth_out", "cloud_out", "stats_out"]


def test_surface_stats_struct_matches_the_header():
    m = re.search(r"typedef\s+struct\s+xm_surface_stats\s*\{(.*?)\}\s*xm_surface_stats\s*;", _header(), flags=re.S)
    assert m, "xm_surface_stats is not declared in include/xmaps.h"
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    want = {"uint64_t": ctypes.c_uint64, "double": ctypes.c_double}
    assert [(n, want[t]) for n, t in fields] == list(N.xm_surface_stats._fields_)
    assert [n for n, _ in fields] == ["n_nonzero", "n_events", "n_inliers", "n_index_errors", "lo", "hi", "t_min", "t_max"]
    assert ctypes.sizeof(N.xm_surface_stats) == 8 * len(fields) == 64


def test_api_version_is_unchanged():
    assert int(re.search(r"#define\s+XM_API_VERSION\s+(\d+)", _header()).group(1)) == 5
