"""CPU: the restatement of the ESL depth optimisation (tests/esl_optim_ref.py) against the reference's own outputs (golden G13: the
reference's depth_optimization on the installed scipy; tests/golden/make_golden_esl_optim.py) and against a live scipy; the table
builder and the binding's layout."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import esl_optim_cases as K
import esl_optim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rigs(golden_dir):
    return K.load_g13(golden_dir)


@pytest.mark.parametrize("name", K.G13_RIGS)
def test_restatement_equals_the_reference_bit_for_bit(rigs, name):
    rig = rigs[name]
    depth, nfev, st = R.depth_optim(K.ref_rig(rig), rig["surface"], rig["depth_init"])
    assert np.array_equal(depth.view(np.uint32), rig["depth_optim"].view(np.uint32))
    assert np.array_equal(nfev, rig["nfev"])
    assert 200 <= st["n_optimised"] == np.count_nonzero(nfev) <= 300 and st["n_evals"] == int(nfev.sum()) and st["n_hit_limit"] == 0


def test_fixture_is_the_cases_construction(rigs):
    """the fixture's inputs are what make_rig builds from the stored seeds: the seeded rigs of the GPU tests share its construction"""
    for name in K.G13_RIGS:
        made = K.make_rig(*K.G13_SPECS[name])
        for k in K.RIG_KEYS:
            assert np.allclose(np.asarray(made[k]), rigs[name][k], rtol=1e-9, atol=0), (name, k)  # (cos / sin may differ in a last bit)
    assert rigs["a"]["surface"][0, 0] == 0 and rigs["b"]["surface"][0, 0] != 0  # (+inf fill, finite fill)


def _closures(rng, n):
    """(func, a, b, xatol, maxfun): step-shaped costs like the optimisation's (piecewise constant, plateaus of 100000, +inf
    levels), smooth ones, and both at tolerances where a parabolic step is moved to tol1"""
    out = []
    for i in range(n):
        a = float(rng.uniform(-50, 80))
        b = a + float(rng.uniform(1e-3, 40))
        kind = i % 4
        levels = rng.random(64) * 10
        if kind == 1:
            levels[rng.random(64) < 0.3] = 100000.0
        if kind == 2:
            levels[rng.random(64) < 0.2] = math.inf
        cells = float(rng.uniform(3, 60))
        c0, curv, tilt = float(rng.uniform(a, b)), float(rng.uniform(0.1, 5)), float(rng.uniform(-1, 1))
        if kind == 3:
            func = lambda x, c0=c0, curv=curv, tilt=tilt: curv * (x - c0) ** 2 + tilt * math.sin(3 * x)
        else:
            func = lambda x, a=a, b=b, levels=levels, cells=cells, c0=c0: \
                float(levels[int((x - a) / (b - a) * cells) % 64]) + 0.5 * abs(int((x - c0) * cells / (b - a)))
        xatol = (1e-5, 1e-5, 0.05 * (b - a), 1e-3)[i % 4] if i % 8 < 4 else 1e-5
        out.append((func, a, b, xatol, (500, 500, 500, 7)[(i // 4) % 4]))
    return out


def test_solver_equals_a_live_scipy():
    so = pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(13)
    steps, hits = set(), 0
    for func, a, b, xatol, maxfun in _closures(rng, 400):
        with np.errstate(all="ignore"):
            res = so.minimize_scalar(func, bounds=(np.float64(a), np.float64(b)), method="bounded", options={"xatol": xatol, "maxiter": maxfun})
        xf, nfev, hit, trace = R.minimize_bounded(func, a, b, xatol, maxfun)
        assert float(res.x) == xf and res.nfev == nfev and (res.status == 1) == hit, (a, b, xatol, maxfun)
        steps |= {s for s, _ in trace} | {br for _, br in trace}
        hits += hit
    assert {"golden", "golden+rejected", "parabolic", "parabolic_tol1", "le:a", "le:b", "gt:a:nfc", "gt:b:nfc", "gt:a:fulc", "gt:b:fulc"} <= steps
    assert {"gt:a:none", "gt:b:none"} & steps and hits > 20


def test_fma_is_one_rounding():
    rng = np.random.default_rng(3)
    for _ in range(2000):
        d, s = float(rng.standard_normal()), float(abs(rng.standard_normal()) * 3)
        exact = R.Fraction(d) * R.Fraction(d) + R.Fraction(s)
        got = R.fma(d, d, s)
        assert abs(R.Fraction(got) - exact) <= abs(R.Fraction(np.nextafter(got, math.inf)) - exact)
        assert abs(R.Fraction(got) - exact) <= abs(R.Fraction(np.nextafter(got, -math.inf)) - exact)
    assert R.fma(math.inf, math.inf, 1.0) == math.inf and R.fma(1e200, 1e200, 0.0) == math.inf and math.isnan(R.fma(math.nan, 1.0, 0.0))
    assert R.fma(1.0 + 2.0 ** -30, 1.0 + 2.0 ** -30, -1.0) == 2.0 ** -29 + 2.0 ** -60  # (a plain product loses the last term)


def test_table_builder_follows_esl_init_and_the_restatements_rt(rigs):
    from x_maps_amd.calibration import CamProjCalibrationParams
    from x_maps_amd.esl_init import build_esl_init_tables
    from x_maps_amd.esl_optim import build_esl_optim_tables, make_rt
    rig = rigs["a"]
    cp = CamProjCalibrationParams(rig["cam_w"], rig["cam_h"], rig["proj_w"], rig["proj_h"], 3 * rig["proj_w"], 3 * rig["proj_h"], rig["cam_K"],
                                  rig["cam_D"], rig["proj_K"], rig["proj_D"], rig["R"], rig["T"].reshape(3, 1))
    tb = build_esl_optim_tables(cp)
    assert tb["p1_03"] == build_esl_init_tables(cp)["p1_03"] != 0 and tb["window_size"] == 3
    assert np.array_equal(tb["proj_surface"], rig["proj"]) and tb["proj_surface"].dtype == np.float32
    assert np.array_equal(tb["cam_K"], rig["cam_K"]) and np.array_equal(tb["proj_D"], rig["proj_D"])
    # the product's Rt takes its orthogonal factor from an SVD, the restatement's from Newton rounds: equal to rounding
    rt = make_rt(rig["R"], rig["T"])
    assert rt.shape == (12,) and np.abs(rt - rig["Rt"]).max() < 1e-14 and np.array_equal(rt, tb["Rt"])
    assert np.array_equal(rt[9:], rig["T"].astype(np.float32).astype(np.float64))
    assert np.abs(rt[:9] - rig["R"].ravel()).max() < 1e-7 and not np.array_equal(rt[:9], rig["R"].ravel())  # (the float32 rounding shows)


def test_binding_layout_matches_the_header(tmp_path):
    from x_maps_amd import _native as N
    assert ctypes.sizeof(N.xm_esl_optim_config) == 8 * 4 + 2 * 8 + (9 + 5 + 9 + 5 + 12) * 8 + 8
    assert ctypes.sizeof(N.xm_esl_optim_stats) == 6 * 8
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "xmaps.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %d\\n", sizeof(xm_esl_optim_config), offsetof(xm_esl_optim_config, xatol),\n'
                   '         offsetof(xm_esl_optim_config, Rt), offsetof(xm_esl_optim_config, proj_surface), sizeof(xm_esl_optim_stats),\n'
                   '         XM_API_VERSION);\n  return 0;\n}\n')
    exe = tmp_path / "t"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [ctypes.sizeof(N.xm_esl_optim_config), N.xm_esl_optim_config.xatol.offset, N.xm_esl_optim_config.Rt.offset,
                   N.xm_esl_optim_config.proj_surface.offset, ctypes.sizeof(N.xm_esl_optim_stats), 5]
