"""CPU: the restatement of ESL's two filters (tests/esl_filter_ref.py) against the installed scipy's lsqr, against the reference's
own denoise_tv (golden G14: tests/golden/make_golden_esl_filter.py) and against a brute-force bilateral filter; the dims quirk, the
early exits, the bilateral filter's border / copy / table reach; the ctypes structs against the header."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import esl_filter_cases as K
import esl_filter_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g14(golden_dir):
    return K.load_g14(golden_dir)


@pytest.fixture(scope="module")
def runs(g14):
    """per fixture scene: the restatement's run and the same loop around scipy's own lsqr, on the fixture's bilateral map"""
    out = {}
    for n, s in g14.items():
        mine, theirs = R.Record(), R.Record()
        x, info = R.denoise_tv(s["bilateral"], rec=mine)
        x2, _ = R.denoise_tv(s["bilateral"], lsqr=R.lsqr_scipy, rec=theirs)
        out[n] = (x, info, mine, x2, theirs)
    return out


def test_restated_lsqr_equals_scipys_on_every_inner_call(runs):
    trips, istops = set(), set()
    for n, (x, info, mine, x2, theirs) in runs.items():
        assert len(mine.calls) == len(theirs.calls) == info["n_lsqr"] >= 180
        for (rhs_a, dx_a), (rhs_b, dx_b) in zip(mine.calls, theirs.calls):
            assert np.array_equal(rhs_a.view(np.uint64), rhs_b.view(np.uint64)) and np.array_equal(dx_a.view(np.uint64), dx_b.view(np.uint64))
        assert mine.trips == theirs.trips and mine.istops == theirs.istops and np.array_equal(x.view(np.uint64), x2.view(np.uint64))
        trips |= set(mine.trips)
        istops |= set(mine.istops)
        print(n, "decision margin", info["margin"])
        assert info["margin"] >= 1e-6
    assert trips == {1, 2, 3, 4, 5} and istops == {2, 7}


@pytest.fixture(scope="module")
def fsum_runs(g14):
    """the restatement with exactly rounded norms: how far a summation order moves the values of each scene"""
    return {n: R.denoise_tv(s["bilateral"], norm=R.norm_fsum) for n, s in g14.items()}


def test_restatement_equals_the_references_denoise_tv(g14, runs, fsum_runs):
    """trip counts exactly; values to the order in which np.linalg.norm sums -- the BLAS kernel of the machine that runs this, which
    need not be the one that wrote the fixture -- bounded like the device's: 1000 x the numpy-vs-fsum difference here, floor 1e-12"""
    for n, s in g14.items():
        x, info = runs[n][:2]
        bound = max(1000.0 * float(np.abs(x - fsum_runs[n][0]).max()), 1e-12)
        d = float(np.abs(x - s["filtered"]).max())
        print(n, "restatement vs G14:", d, "bound", bound)
        assert s["filtered"].dtype == np.float64 and d <= bound
        assert np.array_equal(info["trips"], s["trips"])
        assert np.array_equal(R.bilateral(s["input"]).view(np.uint32), s["bilateral"].view(np.uint32))
        assert np.array_equal(s["input"], K.scene(*K.G14_SCENES[n]))
    a = g14["a"]
    x, info = R.denoise_tv(a["input"])
    bound = max(1000.0 * float(np.abs(x - R.denoise_tv(a["input"], norm=R.norm_fsum)[0]).max()), 1e-12)
    assert np.abs(x - a["tv_only"]).max() <= bound and np.array_equal(info["trips"], a["tv_only_trips"])


def test_fsum_norms_move_values_but_no_trip_count(g14, runs, fsum_runs):
    for n in g14:
        x, info = runs[n][:2]
        x2, info2 = fsum_runs[n]
        d = np.abs(x - x2).max()
        print(n, "numpy vs fsum norms:", d)
        assert np.array_equal(info["trips"], info2["trips"]) and d < 1e-12


def test_the_dims_swap_is_live(g14):
    img = g14["a"]["bilateral"]  # 20 x 24
    swapped, _ = R.denoise_tv(img)
    plain, _ = R.denoise_tv(img, swapped=False)
    assert np.abs(swapped - plain).max() > 1e-3
    # on a square image the two agree: only the stride differs
    sq = img[:, :20]
    assert np.array_equal(R.denoise_tv(sq)[0], R.denoise_tv(sq, swapped=False)[0])


def test_operators_are_adjoint_and_match_a_dense_matrix():
    rng = np.random.default_rng(5)
    H, W = 4, 6
    N = H * W
    for axis in (0, 1):
        M = np.stack([R.D(e, H, axis) for e in np.eye(N)], 1)
        for k in range(N):
            row = np.zeros(N)
            if (axis == 0 and k >= H) or (axis == 1 and k % H != 0):
                row[k], row[k - (H if axis == 0 else 1)] = 1, -1
            assert np.array_equal(M[k], row)
        y = rng.standard_normal(N)
        assert np.array_equal(R.Dt(y, H, axis), M.T @ y) or np.allclose(R.Dt(y, H, axis), M.T @ y, rtol=0, atol=1e-15)
    assert np.array_equal(R.soft_threshold(np.array([-0.3, -0.05, 0.0, 0.1, 0.25]), 0.1), np.array([-0.3 + 0.1, -0.0, 0.0, 0.0, 0.25 - 0.1]))


def test_early_exits():
    for H, W in ((20, 24), (48, 40)):
        x, info = R.denoise_tv(K.zero_map(H, W))
        assert info["n_outer"] == 1 and info["n_lsqr"] == 10 and info["istop_count"][0] == 10 and info["sum_itn"] == 0 and not x.any()
        assert (info["trips"][:10] == 0).all() and (info["trips"][10:] == 0xFF).all() and info["final_norm"] == 0.0
        x, info = R.denoise_tv(K.constant_map(H, W))
        assert info["n_outer"] == 2 and info["n_lsqr"] == 20 and np.abs(x - 58.25).max() < 1e-6
        x, info = R.esl_filter(K.ramp(H, W))[::2]
        assert 2 < info["n_outer"] < 10 and info["final_norm"] <= R.TOL and info["margin"] >= 1e-6
        assert (info["trips"][info["n_lsqr"]:] == 0xFF).all()


def test_bilateral_border_copy_and_table_reach():
    assert [R.reflect101(i, 5) for i in (-2, -1, 0, 4, 5, 6)] == [2, 1, 0, 4, 3, 2]
    assert [R.reflect101(i, 2) for i in (-2, -1, 2, 3)] == [0, 1, 0, 1] and R.reflect101(-2, 1) == 0
    taps = R.bilateral_taps()
    assert len(taps) == 13 and taps[0][:2] == (-2, 0) and taps[6][:2] == (0, 0) and taps[6][2] == 1.0
    c = K.constant_map(6, 7)
    assert np.array_equal(R.bilateral(c), c)
    almost = c.copy()
    almost[2, 3] = np.nextafter(np.float32(58.25), np.float32(60))  # max - min = 3.8e-6 >= FLT_EPSILON: filtered, not copied
    assert not np.array_equal(R.bilateral(almost), almost)
    # |v - v0| = len: a = 4096 exactly, idx + 1 = 4097, the table's last entry
    two = np.full((5, 5), 20.0, np.float32)
    two[2, 2] = 120.0
    scale, lut = R.bilateral_table(two.min(), two.max())
    assert lut.shape == (4098,) and np.float32(100.0) * scale == 4096.0 and lut[0] == 1.0
    out = R.bilateral(two)
    assert out[2, 2] == 120.0 and out[0, 0] == 20.0  # the far weight exp(-100^2 / 18) is 0 in float32
    # a 1 x 1 and a 1 x N map
    assert R.bilateral(np.array([[3.0]], np.float32))[0, 0] == 3.0
    row = np.array([[1.0, 2.0, 4.0, 8.0]], np.float32)
    assert np.abs(R.bilateral(row) - R.bilateral_bruteforce(row)).max() < 1e-5


def test_bilateral_against_the_float64_formula(g14):
    """the table is a linear interpolation of exp(-t^2 / 18) over bins of len / 4096 in float32 arithmetic: the error is measured
    here and printed; its bound is the interpolation's h^2 / 8 max|f''| (f'' <= 1 / 9) plus a few float32 roundings of sums of 13
    terms of magnitude hi"""
    for n, s in g14.items():
        img = s["input"]
        err = float(np.abs(s["bilateral"].astype(np.float64) - R.bilateral_bruteforce(img)).max())
        h = (float(img.max()) - float(img.min())) / 4096
        bound = float(img.max()) * (h * h / 8 / 9 + 16 * 2.0 ** -24)
        print(n, "bilateral: table vs float64 formula, max abs error", err, "bound", bound)
        assert err <= bound


def test_thirdparty_pin_once_it_exists(g14, golden_dir):
    """pin-on-arrival (tools/pin_thirdparty.py): cv2's and pylops' own outputs on G14's inputs, where a maintainer recorded them"""
    path = os.path.join(golden_dir, "g14_esl_filter_thirdparty.npz")
    if not os.path.exists(path):
        pytest.skip("g14_esl_filter_thirdparty.npz is absent: cv2 / pylops are not in this image (DESIGN.md section 5)")
    t = np.load(path)
    for n, s in g14.items():
        if f"{n}_cv2_bilateral" in t.files:  # last bits may move: the centre tap's place in the sum and fused multiply-adds
            d = np.abs(t[f"{n}_cv2_bilateral"].astype(np.float64) - s["bilateral"]).max()
            print(n, "cv2 bilateral vs restatement", d)
            assert d <= 8 * 2.0 ** -24 * float(s["input"].max())
        if f"{n}_pylops_tv" in t.files:  # the table prints two decimals: 1e-5 is fit for purpose (float32 operator dtype)
            d = np.abs(t[f"{n}_pylops_tv"] - s["filtered"]).max()
            print(n, "pylops TV vs restatement", d, "outer", int(t[f"{n}_pylops_niter"]))
            assert d <= 1e-5


def test_ctypes_structs_match_the_header():
    from x_maps_amd import _native as N
    assert ctypes.sizeof(N.xm_esl_filter_config) == 8 * 4 + 8 * 8 and ctypes.sizeof(N.xm_esl_filter_stats) == 3 * 8 + 4 * 4 + 8 * 4
    assert N.XM_ESL_FILTER_NO_BILATERAL == 1 and N.XM_ESL_FILTER_NO_TV == 2
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no C compiler")
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "xmaps.h"\nint main(void) {\n'
           '  printf("%zu %zu %zu %zu %zu %d\\n", sizeof(xm_esl_filter_config), offsetof(xm_esl_filter_config, sigma_color),\n'
           '         offsetof(xm_esl_filter_config, damp), sizeof(xm_esl_filter_stats), offsetof(xm_esl_filter_stats, istop_count),\n'
           '         XM_API_VERSION);\n  return 0;\n}\n')
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "t.c"), "w") as f:
            f.write(src)
        subprocess.run([cc, "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")], check=True)
        out = [int(v) for v in subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [ctypes.sizeof(N.xm_esl_filter_config), N.xm_esl_filter_config.sigma_color.offset, N.xm_esl_filter_config.damp.offset,
                   ctypes.sizeof(N.xm_esl_filter_stats), N.xm_esl_filter_stats.istop_count.offset, 5]
