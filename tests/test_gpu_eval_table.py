"""-m gpu: the evaluation table's scorer on the device (xm_eval_table_*, csrc/xmaps_evaltable.hpp, x_maps_amd.eval_table.EvalTable)
against golden G15 -- the reference's own combine_mc3d / load_and_filter / evaluation_stats -- and, at small shapes, against the
NumPy yardstick of tests/eval_table_cases.py, which tests/test_eval_table_golden_cpu.py holds to the same golden.

Inputs of the shape tests are multiples of 1/8 (eval_table_cases.make_case): every float32 difference and square of a per-scan row
is exact and every float64 sum too, in any order, so the xm_eval_sums of those rows are EQUAL to the yardstick's, sums included
(tests/test_gpu_eval_edges.py derives this).  A "1 sec" row's estimate is a mean over the scans, no multiple of 1/8: its counts are
equal -- the float32 maps are bit-identical and the margin comes from the exact ground-truth sum -- and margin / RMSE agree to rtol
1e-9, that file's bound for a float64 sum of up to 2^22 non-negative terms.  Each case asserts on its INPUTS that no pixel's error
lies within 1e-3 * margin of the margin.  Against G15 the tolerance is the golden's: counts and quotients equal, margin / RMSE /
avg_depth to rtol 1e-6 (the reference sums in float32).

The shapes: one pixel, single rows and columns, sizes below a quad, odd sizes (scalar loads), multiples of four (16-byte loads),
and two shapes of three flat tiles with a partial last one, one per load path, derived from the constants of
csrc/xmaps_geometry.hpp (the unmarked test at the end checks that on the CPU)."""
import ctypes as C
import importlib.util
import math
import os
import re

import numpy as np
import pytest

import eval_ref as E
import eval_table_cases as K

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _constants():
    geo = open(os.path.join(ROOT, "x_maps_amd", "csrc", "xmaps_geometry.hpp")).read()
    block = int(re.search(r"constexpr\s+int\s+BLOCK\s*=\s*(\d+)", geo).group(1))
    m = re.search(r"constexpr\s+int\s+EVT_UN\s*=\s*(\d+)\s*,\s*EVT_TILE\s*=\s*BLOCK\s*\*\s*4\s*\*\s*EVT_UN\s*;", geo)
    mw = re.search(r"constexpr\s+int\s+EVT_MW\s*=\s*(\d+)\s*,\s*EVT_MH\s*=\s*BLOCK\s*/\s*EVT_MW\s*;", geo)
    return block, block * 4 * int(m.group(1)), int(mw.group(1)), block // int(mw.group(1))


BLOCK, TILE, MW, MH = _constants()
TILES_SCALAR = (3, TILE - 5)        # 3 * TILE - 15 pixels, odd: scalar loads, three flat tiles, the last 15 pixels short
TILES_VEC = (4, TILE // 2 + 33)     # 2 * TILE + 132 pixels, a multiple of four: 16-byte loads, three flat tiles, the last 132 pixels wide
# (shape, scans, methods, the methods with a 1-sec row): every shape, n_scans in {1, 2, 5, 61}, n_methods in {1, 3, 8}, no / one / every 1-sec row
CASES = [((1, 1), 1, 1, ()), ((1, 7), 2, 3, (1,)), ((7, 1), 5, 1, (0,)), ((2, 2), 61, 3, (0, 1, 2)), ((3, 3), 2, 8, ()),
         ((37, 29), 5, 8, tuple(range(8))), ((131, 97), 2, 3, (2,)), (TILES_SCALAR, 5, 3, (0, 1, 2)), (TILES_VEC, 2, 8, (5,)),
         ((37, 29), 61, 1, ()), (TILES_VEC, 61, 1, ())]


def _score(table, gt, est, one_sec):
    names = [f"m{i}" for i in range(len(est))]
    return table.score(gt, dict(zip(names, est)), one_sec=[names[i] for i in one_sec])


def _same(a, b):
    return np.array_equal(np.float64(a), np.float64(b), equal_nan=True)  # (NaN and +-inf as NumPy's)


def _compare(score, tab, n_methods, exact_sums=True):
    """the device's cells against the yardstick's"""
    assert score.results.shape == score.sums.shape == (len(tab["cells"]), len(tab["cells"][0]))
    for r, cells in enumerate(tab["cells"]):
        for s, c in enumerate(cells):
            got, res = score.sums[r, s], score.results[r, s]
            print(r, s, {k: got[k] for k in got.dtype.names}, {k: res[k] for k in res.dtype.names}, c)
            for k in E.COUNTS:
                assert int(got[k]) == c[k], (r, s, k, int(got[k]), c[k])
            assert (int(res["n_valid"]), int(res["n_gt_zero"])) == (c["n_valid"], c["n_gt_zero"])
            if exact_sums and r < n_methods:
                assert float(got["sum_gt"]) == c["sum_gt"] and float(got["sum_sq"]) == c["sum_sq"], (r, s, got, c["sum_gt"], c["sum_sq"])
            else:
                np.testing.assert_allclose([got["sum_gt"], got["sum_sq"]], [c["sum_gt"], c["sum_sq"]], rtol=1e-9, atol=0)
            for f in ("fillrate", "perc_1", "perc_5", "perc_10"):
                assert _same(res[f], c[f]), (r, s, f, res[f], c[f])  # quotients of the same integers: equal as doubles
            for f in ("margin", "rmse"):
                if math.isfinite(c[f]):
                    np.testing.assert_allclose(res[f], c[f], rtol=1e-9, atol=0, err_msg=f"{r} {s} {f}")
                else:
                    assert _same(res[f], c[f]), (r, s, f, res[f], c[f])


def _compare_maps(score, tab):
    assert np.array_equal(score.mask.view(np.uint32), tab["mask"].view(np.uint32))  # bit for bit
    np.testing.assert_allclose(score.avg_depth, tab["avg_depth"], rtol=1e-9, atol=0)


# ---- 1. golden G15 -----------------------------------------------------------------------------------------------------------

@gpu
def test_g15_on_the_device(golden_dir):
    from x_maps_amd.eval_table import EvalTable
    g15 = np.load(os.path.join(golden_dir, "g15_eval_table.npz"))
    gt, est, _ = K.g15_inputs()
    assert K.inputs_sha256(gt, est) == str(g15["inputs_sha256"])
    tab = K.table(gt, est, one_sec=(K.G15_METHODS.index("mc3d"),))
    h, w = K.G15_SHAPE
    with EvalTable(h, w, K.MIN_D, K.MAX_D) as t:
        score = t.score(gt, est, one_sec=K.G15_ONE_SEC)
        one_sec, one_sec_avg = t.combine(est["mc3d"])
    assert tuple(score.rows) == K.G15_ROWS
    # the mask and the 1-sec map: the NumPy restatement bit for bit, the golden by hash and sample
    _compare_maps(score, tab)
    assert np.array_equal(one_sec.view(np.uint32), tab["one_sec_maps"][2].view(np.uint32))
    K.check_maps_against_golden(g15, score.mask, one_sec)
    print("avg_depth", score.avg_depth, float(g15["avg_depth"]), "1-sec map's", one_sec_avg)
    np.testing.assert_allclose(score.avg_depth, float(g15["avg_depth"]), rtol=1e-6, atol=0)

    def get(r, s):
        d = {k: score.results[r, s][k] for k in E.FLOATS}
        d.update({k: score.sums[r, s][k] for k in E.COUNTS})
        print(r, s, d)
        return d
    K.check_cells_against_golden(g15, get)
    _compare(score, tab, len(K.G15_METHODS))  # and the yardstick, to its own tighter bounds


# ---- 2. shapes ----------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("shape,n_scans,n_methods,one_sec", CASES, ids=[f"{h}x{w}-s{s}-m{m}-o{len(o)}" for (h, w), s, m, o in CASES])
def test_shapes_equal_the_yardstick(shape, n_scans, n_methods, one_sec):
    from x_maps_amd.eval_table import EvalTable
    gt, est, _ = K.make_case(shape, n_scans, n_methods, seed=shape[0] * 10007 + shape[1] + 31 * n_scans)
    if shape == (1, 1):
        gt[0, 0, 0], est[0, 0, 0, 0] = 43.0, 44.0  # one pixel with ground truth and an error that counts once
    tab = K.table(gt, est, one_sec)
    K.assert_clear_of_the_margin(tab)
    if shape[0] * shape[1] > 1000:  # the case holds what it is for
        c = tab["cells"][0][0]
        assert 0 < c["n10"] < c["n5"] < c["n1"] and c["n_valid"] > 0 and 0 < c["n_gt_zero"] < gt[0].size and c["rmse"] > 0
        assert shape[0] * shape[1] < 10000 or all(row[0]["n10"] > 0 for row in tab["cells"][n_methods:])
    with EvalTable(shape[0], shape[1], K.MIN_D, K.MAX_D) as t:
        score = _score(t, gt, est, one_sec)
        maps = {m: t.combine(est[m])[0] for m in one_sec[:2]}
    _compare_maps(score, tab)
    for m, got in maps.items():
        assert np.array_equal(got.view(np.uint32), tab["one_sec_maps"][m].view(np.uint32))
    _compare(score, tab, n_methods)


# ---- 3. value edges -----------------------------------------------------------------------------------------------------------

def _edge_case():
    """16 x 12, 3 scans, 2 methods: a quiet background and one pixel per edge, in the ground truth and in the estimates"""
    f32 = np.float32
    lo, hi = f32(K.MIN_D), f32(K.MAX_D)
    gt = np.full((3, 16, 12), 50.0, f32)
    est = np.full((2, 3, 16, 12), 50.125, f32)
    gt[:, :, ::5] = 0
    est[:, :, ::4, :] = 0
    values = [lo, np.nextafter(lo, f32(0)), np.nextafter(lo, f32(999)), hi, np.nextafter(hi, f32(0)), np.nextafter(hi, f32(999)),
              f32(-3), f32(-np.inf), f32(np.inf), f32(-0.0)]
    at = iter(range(13, 192, 5))
    for v in values:  # every value once in a ground-truth scan and once in each method's estimate, all at different pixels
        for target in (gt[1], est[0][2], est[1][0]):
            target.ravel()[next(at)] = v
    return gt, est


@gpu
def test_value_edges_equal_the_yardstick():
    from x_maps_amd.eval_table import EvalTable
    gt, est = _edge_case()
    tab = K.table(gt, est, (0, 1))
    lo, hi = np.float32(K.MIN_D), np.float32(K.MAX_D)
    g1 = E.load_and_filter(gt[1], tab["mask"], K.MIN_D, K.MAX_D)
    kept = {float(v) for v in g1.ravel()}  # one float32 step inside either bound is kept, the bounds themselves are not
    assert float(np.nextafter(lo, np.float32(999))) in kept and float(np.nextafter(hi, np.float32(0))) in kept
    assert float(lo) not in kept and float(hi) not in kept and float(np.nextafter(hi, np.float32(999))) not in kept
    K.assert_clear_of_the_margin(tab)
    with EvalTable(16, 12, K.MIN_D, K.MAX_D) as t:
        score = _score(t, gt, est, (0, 1))
    _compare_maps(score, tab)
    _compare(score, tab, 2, exact_sums=False)  # (the values beside the bounds are no multiples of 1/8)


@gpu
def test_no_ground_truth_and_no_estimate():
    from x_maps_amd.eval_table import EvalTable
    gt, est, _ = K.make_case((37, 29), 3, 2, seed=77)
    with EvalTable(37, 29, K.MIN_D, K.MAX_D) as t:
        # a ground-truth stack that is zero everywhere: NaN margins (NumPy's 0 / 0), fill rates of -inf (-H W / 0)
        zero = np.zeros_like(gt)
        tab = K.table(zero, est, (1,))
        assert math.isnan(tab["cells"][0][0]["margin"]) and not (tab["mask"] != 0).any() and tab["avg_depth"] == 0
        assert all(c["fillrate"] == -math.inf and c["rmse"] == 0 and c["n_close"] == 0 for row in tab["cells"] for c in row)
        score = _score(t, zero, est, (1,))
        _compare_maps(score, tab)
        _compare(score, tab, 2)
        assert np.isnan(score.results["margin"]).all() and (score.results["fillrate"] == -np.inf).all()
        # one scan without ground truth among scans with
        part = gt.copy()
        part[1] = 0
        tab = K.table(part, est, (1,))
        assert math.isnan(tab["cells"][0][1]["margin"]) and math.isfinite(tab["cells"][0][0]["margin"]) and (tab["mask"] != 0).any()
        K.assert_clear_of_the_margin(tab)
        score = _score(t, part, est, (1,))
        _compare_maps(score, tab)
        _compare(score, tab, 2)
        # estimates all zero: RMSE 0, n_valid 0 -- in the method's rows and in its 1-sec row
        none = np.zeros_like(est)
        tab = K.table(gt, none, (0,))
        assert all(c["rmse"] == 0 and c["n_valid"] == 0 and c["n1"] > 0 for row in tab["cells"] for c in row)
        score = _score(t, gt, none, (0,))
        _compare(score, tab, 2)
        assert (score.results["rmse"] == 0).all() and (score.sums["n_valid"] == 0).all()


# ---- 4. median ------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("shape", [(1, 9), (9, 1), (2, 2), (3, 3), (1, 1), (MH + 1, MW + 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_median_of_distinct_values(shape):
    from x_maps_amd.eval_table import EvalTable, median_blur3
    n = shape[0] * shape[1]
    img = (np.random.default_rng(n).permutation(n).astype(np.float32) + 1).reshape(shape)  # 1 .. n, each once
    with EvalTable(shape[0], shape[1], 0, 10 * n + 10) as t:
        comb, avg, mean = t.combine([img], want_mean=True)
        comb2, _ = t.combine(np.stack([img, np.zeros_like(img), img * 3]))  # a second map out of range: mean of img and 3 img
    want = median_blur3(img)
    assert np.array_equal(mean, img) and np.array_equal(comb, want), (img, comb, want)
    assert avg == float(want.astype(np.float64).sum()) / n
    assert np.array_equal(comb2, median_blur3((img + img * 3) / np.float32(2)))
    if shape == (3, 3):
        assert comb[1, 1] == 5 and len(set(img.ravel())) == 9


# ---- 5. independence ---------------------------------------------------------------------------------------------------------------

@gpu
def test_bits_do_not_depend_on_the_run_the_company_or_the_memory():
    import torch
    from x_maps_amd.eval_table import EvalTable
    shape, S, M = (24, TILE // 8 + 5), 5, 8  # 3 * TILE + 120 pixels, a multiple of four: four flat tiles
    assert shape[0] * shape[1] % 4 == 0 and shape[0] * shape[1] > 3 * TILE
    gt, est, _ = K.make_case(shape, S, M, seed=5)
    rng = np.random.default_rng(6)  # arbitrary float32 values: now the order of a sum shows in its last bits
    gt = np.where(gt > 0, gt + rng.random(gt.shape, np.float32), 0).astype(np.float32)
    est = np.where(est > 0, est + rng.random(est.shape, np.float32), 0).astype(np.float32)
    names = [f"m{i}" for i in range(M)]
    with EvalTable(shape[0], shape[1], K.MIN_D, K.MAX_D) as t:
        a = t.score(gt, dict(zip(names, est)), one_sec=("m3", "m6"))
        b = t.score(gt, dict(zip(names, est)), one_sec=("m3", "m6"))
        alone = t.score(gt, {"m3": est[3]}, one_sec=("m3",))
        d_gt = torch.from_numpy(gt).cuda()
        d_est = [torch.from_numpy(e).cuda() for e in est]
        # the same stacks one float off a 16-byte boundary: the scalar loads
        off = [torch.empty(x.numel() + 1, dtype=torch.float32, device="cuda") for x in [d_gt] + d_est]
        for o, x in zip(off, [d_gt] + d_est):
            o[1:].copy_(x.reshape(-1))
        d_mask = torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        dev = t.score_device(d_gt.data_ptr(), {n: x.data_ptr() for n, x in zip(names, d_est)}, S, one_sec=("m3", "m6"), mask_ptr=d_mask.data_ptr())
        odd = t.score_device(off[0].data_ptr() + 4, {n: o.data_ptr() + 4 for n, o in zip(names, off[1:])}, S, one_sec=("m3", "m6"))
        mask = d_mask.cpu().numpy()
    assert a.rows == names + ["m3_1s", "m6_1s"] and alone.rows == ["m3", "m3_1s"]
    assert np.isfinite(a.results["rmse"]).all() and (a.results["rmse"] > 0).all() and (a.sums["n10"] > 0).all()
    for other, what in ((b, "a second run"), (dev, "device memory"), (odd, "device memory off a 16-byte boundary")):
        assert a.results.tobytes() == other.results.tobytes() and a.sums.tobytes() == other.sums.tobytes(), what
        assert a.avg_depth == other.avg_depth, what
    assert np.array_equal(mask.view(np.uint32), a.mask.view(np.uint32))
    for r_alone, r_all in ((0, 3), (1, M)):
        assert alone.results[r_alone].tobytes() == a.results[r_all].tobytes() and alone.sums[r_alone].tobytes() == a.sums[r_all].tobytes()


# ---- 6. a sequence directory ----------------------------------------------------------------------------------------------------

def _write_sequence(root, gt, est):
    for sub, stack in ((("esl", "depth_optim_filtered"), gt), (("x_maps", "depth_init"), est[0]), (("esl", "depth_init"), est[1]),
                       (("mc3d", "depth"), est[2])):
        if stack is None:
            continue
        os.makedirs(os.path.join(root, *sub))
        for i, a in enumerate(stack):
            np.save(os.path.join(root, *sub, f"scans{i:03d}.npy"), a)


def _tool():
    spec = importlib.util.spec_from_file_location("run_esl_on_arrival", os.path.join(ROOT, "tools", "run_esl_on_arrival.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@gpu
def test_sequence_table_equals_the_per_pair_rows(tmp_path, monkeypatch):
    from x_maps_amd import eval_table as T
    gt, est, _ = K.make_case((48, 40), 3, 3, seed=21)
    K.assert_clear_of_the_margin(K.table(gt, est, (2,)))
    seq = str(tmp_path / "seq")
    _write_sequence(seq, gt, est)
    got = T.sequence_table(seq, K.MIN_D, K.MAX_D)
    want = {"x_maps": T.x_maps_table_row(seq, K.MIN_D, K.MAX_D), "esl_init": T.esl_init_table_row(seq, K.MIN_D, K.MAX_D),
            **T.mc3d_table_rows(seq, K.MIN_D, K.MAX_D)}
    assert list(got) == ["x_maps", "esl_init", "mc3d", "mc3d_1s"]
    for name, row in want.items():
        print(name, got[name], row)
        assert set(got[name]) == set(row) and got[name]["scans"] == row["scans"] == 3
        assert got[name]["fill_rate"] == row["fill_rate"]  # means of equal quotients (the inputs are clear of the margin)
        np.testing.assert_allclose(got[name]["rmse"], row["rmse"], rtol=1e-9, atol=0)
        np.testing.assert_allclose(got[name]["mean_depth"], row["mean_depth"], rtol=1e-6, atol=0)
        assert got[name]["table_cell"] == f"{round(got[name]['fill_rate'], 2)} & {round(got[name]['rmse'], 2)}"
    assert got["mc3d"]["rmse"] > got["mc3d_1s"]["rmse"] > 0 and 0 < got["x_maps"]["fill_rate"] < 1
    # --table-on-device through the tool's main: one more key, the others as they were (the depth maps are the files already there)
    tool = _tool()
    monkeypatch.setattr(tool, "depth_from_scans", lambda *a, **k: {"scans_found": 3, "scans_processed": 3})
    args = ["--scans", seq, "--eval-calib", "unused.yaml", "--min-depth", str(K.MIN_D), "--max-depth", str(K.MAX_D), "--mc3d"]
    monkeypatch.setattr(tool, "mc3d_from_scans", lambda *a, **k: {"scans_found": 3})
    plain, with_table = tool.main(args), tool.main(args + ["--table-on-device"])
    assert "table_1_on_device" not in plain and with_table["table_1_on_device"] == got
    assert {k: v for k, v in with_table.items() if k != "table_1_on_device"} == plain
    assert plain["table_1_row_mc3d_1s"] == want["mc3d_1s"]
    # the two error rows, as depth_table_row words them
    os.remove(os.path.join(seq, "mc3d", "depth", "scans002.npy"))
    short = T.sequence_table(seq, K.MIN_D, K.MAX_D)
    assert short["mc3d"] == short["mc3d_1s"] == T.mc3d_table_rows(seq, K.MIN_D, K.MAX_D)["mc3d"] == \
        {"error": "frames are missing", "gt_files": 3, "mc3d_files": 2}
    assert short["x_maps"] == got["x_maps"] and short["esl_init"] == got["esl_init"]  # (and no bit moves when a method leaves)
    bare = str(tmp_path / "bare")
    _write_sequence(bare, None, est)
    none = T.sequence_table(bare, K.MIN_D, K.MAX_D)
    assert none["x_maps"] == T.x_maps_table_row(bare, K.MIN_D, K.MAX_D) and none["x_maps"]["error"].startswith("no ground truth under")
    assert none["esl_init"] == T.esl_init_table_row(bare, K.MIN_D, K.MAX_D) and none["mc3d"]["mc3d_files"] == 3
    assert none["mc3d_1s"] == none["mc3d"] == T.mc3d_table_rows(bare, K.MIN_D, K.MAX_D)["mc3d_1s"]
    assert "table_1_on_device" not in tool.main(["--scans", bare, "--eval-calib", "unused.yaml", "--table-on-device"])


# ---- 7. argument errors ------------------------------------------------------------------------------------------------------------

@gpu
def test_argument_errors_leave_the_object_usable():
    from x_maps_amd import _native as N
    from x_maps_amd.eval_table import RESULT_DTYPE, SUMS_DTYPE, EvalTable
    lib = N.load_library()
    h = C.c_void_p()
    good = N.xm_eval_table_config(C.sizeof(N.xm_eval_table_config), 5, 7, 20.0, 120.0, 0)
    for cfg in (N.xm_eval_table_config(C.sizeof(N.xm_eval_table_config) - 4, 5, 7, 20.0, 120.0, 0),
                N.xm_eval_table_config(C.sizeof(N.xm_eval_table_config), 0, 7, 20.0, 120.0, 0),
                N.xm_eval_table_config(C.sizeof(N.xm_eval_table_config), 5, -1, 20.0, 120.0, 0)):
        assert lib.xm_eval_table_create(0, C.byref(cfg), C.byref(h)) == N.XM_ERR_INVALID and not h.value
    assert lib.xm_eval_table_create(0, None, C.byref(h)) == N.XM_ERR_INVALID
    assert lib.xm_eval_table_create(0, C.byref(good), None) == N.XM_ERR_INVALID
    assert lib.xm_eval_table_create(99, C.byref(good), C.byref(h)) == N.XM_ERR_INVALID and not h.value
    gt, est, _ = K.make_case((5, 7), 2, 2, seed=3)
    tab = K.table(gt, est, (1,))
    with EvalTable(5, 7, K.MIN_D, K.MAX_D) as t:
        res, sums, avg = np.zeros((3, 2), RESULT_DTYPE), np.zeros((3, 2), SUMS_DTYPE), C.c_double()
        ptrs = (C.c_void_p * 2)(est[0].ctypes.data, est[1].ctypes.data)
        holed = (C.c_void_p * 2)(est[0].ctypes.data, None)
        g = gt.ctypes.data_as(C.c_void_p)

        def call(gt_p=g, est_p=ptrs, n_methods=2, bits=2, n_scans=2, mem=N.XM_MEM_HOST, obj=t._h):
            return lib.xm_eval_table_score(obj, gt_p, est_p, n_methods, bits, n_scans, mem, res.ctypes.data_as(C.c_void_p),
                                           sums.ctypes.data_as(C.c_void_p), None, C.byref(avg))
        for kw in (dict(n_methods=0), dict(n_methods=9), dict(bits=4), dict(bits=1 << 31), dict(n_scans=0), dict(n_scans=-2), dict(gt_p=None),
                   dict(est_p=None), dict(est_p=holed), dict(mem=7), dict(obj=None)):
            assert call(**kw) == N.XM_ERR_INVALID, kw
            assert N.last_error()
        assert call(n_scans=65536) == N.XM_ERR_TOO_MANY
        assert lib.xm_eval_table_combine(t._h, None, 2, N.XM_MEM_HOST, None, None, None) == N.XM_ERR_INVALID
        assert lib.xm_eval_table_combine(t._h, g, 0, N.XM_MEM_HOST, None, None, None) == N.XM_ERR_INVALID
        assert not res.view(np.uint8).any() and not sums.view(np.uint8).any()  # nothing was written
        with pytest.raises(ValueError):
            t.score(gt, {"a": est[0]}, one_sec=("b",))
        with pytest.raises(ValueError):
            t.score(gt, {"a": est[0][:1]})
        with pytest.raises(ValueError):
            t.score(gt[:, :4], {"a": est[0]})
        # ... and the object still scores: every output optional but one
        assert call() == N.XM_OK
        score = _score(t, gt, est, (1,))
        assert score.results.tobytes() == res.tobytes() and score.sums.tobytes() == sums.tobytes() and score.avg_depth == avg.value
        _compare(score, tab, 2)
        assert lib.xm_eval_table_combine(t._h, g, 2, N.XM_MEM_HOST, None, None, C.byref(avg)) == N.XM_OK and avg.value == score.avg_depth
    lib.xm_eval_table_destroy(None)  # (tolerated)


# ---- CPU: what the shapes are for -----------------------------------------------------------------------------------------------

def test_shapes_cross_the_tile_and_the_load_paths():
    """CPU: the constants of the flat tiles, read from the sources, and what each shape is for"""
    host = open(os.path.join(ROOT, "x_maps_amd", "csrc", "host", "xm_api_evaltable.hpp")).read()
    assert "grid_for(e->px, EVT_TILE)" in host and "e->px % 4" in host  # one block per tile; 16-byte loads need px % 4 == 0
    assert (BLOCK, TILE, MW * MH) == (256, BLOCK * 16, BLOCK)

    def tiles(shape):
        return -(-shape[0] * shape[1] // TILE)
    shapes = [c[0] for c in CASES]
    for sh in ((1, 1), (1, 7), (7, 1), (2, 2), (3, 3), (37, 29), (131, 97), TILES_SCALAR, TILES_VEC):
        assert sh in shapes
    px = lambda sh: sh[0] * sh[1]  # noqa: E731
    assert tiles(TILES_SCALAR) == 3 and px(TILES_SCALAR) % 4 != 0 and 0 < px(TILES_SCALAR) % TILE < TILE
    assert tiles(TILES_VEC) == 3 and px(TILES_VEC) % 4 == 0 and 0 < px(TILES_VEC) % TILE < TILE
    assert tiles((131, 97)) == 4 and px((131, 97)) % 4 != 0 and px((2, 2)) % 4 == 0 and tiles((37, 29)) == 1
    assert 131 > MH and 97 > 2 * MW  # more than one block of the median in either direction, the last ones partial
    assert {c[1] for c in CASES} == {1, 2, 5, 61} and {c[2] for c in CASES} == {1, 3, 8}
    assert {len(c[3]) == 0 for c in CASES} == {True, False} and any(len(c[3]) == 1 for c in CASES) and any(len(c[3]) == c[2] > 1 for c in CASES)
