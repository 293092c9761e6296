"""CPU: what the group objects' Python classes share (x_maps_amd/_group.py) and what the timing tools share (tools/_timing.py).
No library is loaded: surface_group / map_group on every form a caller may hand over, stats_dtype against the two dtypes
tools/run_esl_on_arrival.py used to spell out by hand (written here as literals), and no tool importing another *_time.py."""
import ast
import glob
import os

import numpy as np
import pytest

from x_maps_amd import _group as G
from x_maps_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 3, 5


def _maps(n, dtype, seed=1):
    return (np.random.default_rng(seed).random((n, H, W)) * 100).astype(dtype)


@pytest.mark.parametrize("stack", [lambda s: G.surface_group(s, H, W), lambda s: G.map_group(s, H, W, np.float32)], ids=["surface", "map"])
def test_every_form_of_a_group(stack):
    m = _maps(4, np.float32)
    for given, want in ((list(m), m), (m, m), (m[2], m[2:3]), (tuple(m[:1]), m[:1])):  # a list of 2-D arrays, one 3-D array, one 2-D array
        got = stack(given)
        assert got.dtype == np.float32 and got.shape == want.shape and got.flags.c_contiguous and np.array_equal(got, want)
    strided = np.asfortranarray(m)
    assert stack(strided).flags.c_contiguous and np.array_equal(stack(strided), m)
    for bad in ([], np.zeros((0, H, W), np.float32), np.zeros((2, H, W + 1), np.float32), [np.zeros((H + 1, W), np.float32)],
                np.zeros((W,), np.float32), np.zeros((1, 2, H, W), np.float32)):
        with pytest.raises(ValueError):
            stack(bad)


def test_surface_group_dtypes():
    f32, f64 = _maps(2, np.float32), _maps(2, np.float64, 2)
    assert G.surface_group(f64, H, W).dtype == np.float64 and G.surface_group(f64, H, W) is f64  # (nothing to copy)
    mixed = G.surface_group([f32[0], f64[1]], H, W)  # mixed float32 / float64: float64, the float32 values exact
    assert mixed.dtype == np.float64 and np.array_equal(mixed[0], f32[0].astype(np.float64)) and np.array_equal(mixed[1], f64[1])
    ints = (np.arange(2 * H * W).reshape(2, H, W) * 1000).astype(np.int32)
    for given in (ints, list(ints), ints[0]):  # an integer dtype: float64
        got = G.surface_group(given, H, W)
        assert got.dtype == np.float64 and np.array_equal(got.reshape(-1, H, W)[0], ints[0])
    assert G.surface_group(f32.astype(np.float16), H, W).dtype == np.float64
    assert set(G.T_DTYPES) == {np.dtype(np.float32), np.dtype(np.float64)}
    assert G.T_DTYPES[np.dtype(np.float32)] == N.XM_T_FLOAT32 and G.T_DTYPES[np.dtype(np.float64)] == N.XM_T_FLOAT64
    with pytest.raises(ValueError, match=r"time surfaces must be \(n, 3, 5\), got \(2, 3, 6\)"):
        G.surface_group(np.zeros((2, H, W + 1)), H, W)
    with pytest.raises(ValueError, match="no surfaces"):
        G.surface_group([], H, W)


def test_map_group_takes_the_dtype_it_is_given():
    f64 = _maps(2, np.float64)
    for given in (f64, list(f64), [f64[0], f64[1].astype(np.float32)], (f64 * 10).astype(np.int64)):
        got = G.map_group(given, H, W, np.float32)
        assert got.dtype == np.float32 and got.shape == (2, H, W)
    assert np.array_equal(G.map_group(f64, H, W, np.float32), f64.astype(np.float32))
    with pytest.raises(ValueError, match=r"depth_init must be \(n, 3, 5\), got \(1, 5, 3\)"):
        G.map_group(np.zeros((W, H)), H, W, np.float32, "depth_init")


def test_ptr():
    a = np.zeros(3, np.float32)
    assert G.ptr(None) is None and G.ptr(a).value == a.ctypes.data


def test_stats_dtype_is_the_struct():
    optim = np.dtype([("n_optimised", "<u8"), ("n_evals", "<u8"), ("n_hit_limit", "<u8"), ("n_bad_bounds", "<u8"), ("lo", "<f8"),
                      ("hi", "<f8")])
    flt = np.dtype([("lo", "<f8"), ("hi", "<f8"), ("final_norm", "<f8"), ("n_outer", "<u4"), ("n_lsqr", "<u4"), ("sum_itn", "<u4"),
                    ("reserved", "<u4"), ("istop_count", "<u4", (8,))])
    for struct, want in ((N.xm_esl_optim_stats, optim), (N.xm_esl_filter_stats, flt)):
        got = G.stats_dtype(struct)
        assert got.names == want.names and got.itemsize == want.itemsize == __import__("ctypes").sizeof(struct)
        for name in want.names:
            assert got.fields[name][1] == want.fields[name][1], name          # offset
            assert got.fields[name][0] == want.fields[name][0], name          # element type and shape
        assert got == want
    # a buffer of structs read through the dtype gives the fields' values
    arr = (N.xm_esl_filter_stats * 2)()
    arr[1].n_outer, arr[1].final_norm = 7, 2.5
    arr[1].istop_count[3] = 9
    view = np.frombuffer(bytes(arr), np.uint8).view(G.stats_dtype(N.xm_esl_filter_stats))
    assert view.shape == (2,) and view[1]["n_outer"] == 7 and view[1]["final_norm"] == 2.5 and view[1]["istop_count"][3] == 9


def test_group_object_closes_once_and_tolerates_a_failed_create():
    calls = []

    class Lib:
        def destroy(self, h):
            calls.append(h)

    class Obj(G.GroupObject):
        _destroy = "destroy"

    o = Obj()
    o.close()  # (a create that raised before there was a handle)
    o._lib, o._h = Lib(), 5
    with o as same:
        assert same is o
    o.close()
    del o
    assert calls == [5]


def test_no_tool_imports_another_time_tool():
    tools = sorted(glob.glob(os.path.join(ROOT, "tools", "*.py")))
    timers = {os.path.basename(p)[:-3] for p in tools if p.endswith("_time.py")}
    assert {"esl_init_time", "mc3d_time", "esl_optim_time", "esl_filter_time"} <= timers
    for path in tools:
        for node in ast.walk(ast.parse(open(path).read())):
            names = [a.name for a in node.names] if isinstance(node, ast.Import) else [node.module or ""] if isinstance(node, ast.ImportFrom) else []
            hit = [n for n in names if n.split(".")[-1] in timers]
            assert not hit, (os.path.basename(path), hit)
