#!/usr/bin/env python3
"""Generate tests/golden/g13_esl_optim.npz by RUNNING THE REFERENCE'S OWN depth_optimization (python/eval/compute_depth_esl.py:
104-129, with cost_calculator :45-69 and project_and_backproject_punkt :27-42) through the installed scipy's minimize_scalar.

Run only in the build container (needs /root/reference, which does not exist on the GPU box):
    python tests/golden/make_golden_esl_optim.py
The module imports cv2 and esl_utilities at its top; neither is installed.  esl_utilities becomes an empty stub; cv2 becomes a stub
of the three calls the optimisation makes -- undistortPoints, Rodrigues, projectPoints -- which are the three geometry functions of
tests/esl_optim_ref.py with cv2's shapes and depths around them.  So the geometry is UNPINNED against a real cv2 (DESIGN.md section
5); PINNED are the solver (scipy's own code runs), the cost with its truncation and its patch norm (the reference's own code and
NumPy run), the +inf / finite fill and the bounds.  minimize_scalar is wrapped only to record nfev; cost_calculator is wrapped only
to compare each value it returns with the restatement's at the same rho -- which ASSERTS, on every patch evaluated, that this
machine's np.linalg.norm equals the sequential fused sum -- and the script stops otherwise.  Nothing from /root/reference is copied:
the .npz holds inputs (calibration, surface, depth_init) and the outputs the reference produced for them.

The normalisation and the fill (:207-212) stand in the reference's main(), not in a function; they are restated here in NumPy on
the float64 surface (the G7 / G11 convention), line for line.

The script ASSERTS that the three rigs hold every case the fixture exists for -- see check_cases().

One case of the issue's list cannot be constructed at the reference's xatol: "a parabolic step moved to tol1 from a bound".  It needs
the vertex of an ACCEPTED parabola within tol2 = 2 (sqrt(2.2e-16) |xf| + 1e-5 / 3), about 8e-6, of an end of the current bracket.
The cost is piecewise constant in rho (rho enters only through the truncated projector pixel), so a parabola is accepted only while
the three points still straddle steps -- brackets of 0.1 .. 10 -- and lands that close to an end by chance alone: none did in about
10 000 optimised pixels of 48 seeded rigs like these.  The branch is pinned where it can be reached: against a live scipy on smooth
and step-shaped closures (tests/test_esl_optim_ref_cpu.py), and on the device against the restatement with xatol = 0.25, where the
traces hold it (tests/test_gpu_esl_optim.py)."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import esl_optim_cases as K  # noqa: E402
import esl_optim_ref as R  # noqa: E402

REF_EVAL = "/root/reference/python/eval"


def cv2_stub():
    m = types.ModuleType("cv2")

    def undistortPoints(pts, K_, D_, P=None):
        assert pts.dtype == np.float32 and pts.shape == (1, 2) and P is K_
        return np.array([[R.undistort_points(pts[0, 0], pts[0, 1], K_, np.ravel(D_))]], np.float32)  # (the input's depth)

    def Rodrigues(M):
        assert M.shape == (3, 3)
        return np.array(R.rodrigues_vector(M), np.float64).reshape(3, 1), None

    def projectPoints(obj, rvec, tvec, K_, D_):
        assert obj.shape == (3, 1) and obj.dtype == np.float64 and tvec.dtype == np.float32
        Rr = R.rodrigues_matrix(tuple(float(v) for v in rvec.ravel()))
        Rt = [Rr[i][j] for i in range(3) for j in range(3)] + [float(t) for t in tvec]
        u, v = R.project_points(float(obj[0, 0]), float(obj[1, 0]), float(obj[2, 0]), Rt, K_, np.ravel(D_))
        return np.array([[[u, v]]], np.float64), None

    m.undistortPoints, m.Rodrigues, m.projectPoints = undistortPoints, Rodrigues, projectPoints
    return m


def import_reference():
    sys.modules["cv2"] = cv2_stub()
    eu = types.ModuleType("esl_utilities")
    eu.utils = object
    sys.modules["esl_utilities"] = eu
    sys.path.insert(0, REF_EVAL)
    import compute_depth_esl
    return compute_depth_esl


def run_reference(ref, rig):
    """-> (depth_optim f32, nfev u16): the reference on one rig"""
    cam = rig["surface"].copy()
    with np.errstate(all="ignore"):  # :207-212
        cam = (cam - np.min(cam[cam != 0])) / (np.max(cam[cam != 0]) - np.min(cam[cam != 0]))
        cam[cam < 0] = 0
        cam[cam == 0] = 1 / cam[0, 0]
    mine, _ = R.normalise_and_fill(rig["surface"])
    assert cam.dtype == np.float64 and np.array_equal(cam, mine)
    T = np.zeros((4, 4), np.float32)  # esl_utilities.py:144-146
    T[:3, :3] = rig["R"]
    T[:3, 3] = rig["T"]
    assert np.array_equal(R.make_rt(rig["R"], rig["T"]), rig["Rt"])
    P1 = np.zeros((3, 4))
    P1[0, 3] = rig["p1_03"]
    calib = types.SimpleNamespace(P1=P1, cam_int=rig["cam_K"], cam_dist=rig["cam_D"].reshape(1, 5), proj_int=rig["proj_K"],
                                  proj_dist=rig["proj_D"].reshape(1, 5), T=T)
    d0 = rig["depth_init"]
    assert ((d0 ** 2) / P1[0, 3]).dtype == np.float64 and (d0 ** 2).dtype == np.float32  # (float32 product, float64 quotient)
    proj = ref.get_projector_time_surface((rig["proj_w"], rig["proj_h"]))
    assert np.array_equal(proj, rig["proj"]) and proj.dtype == np.float32
    rr = K.ref_rig(rig)
    nfevs, n_cost = [], [0]
    real_min, real_cost = ref.minimize_scalar, ref.cost_calculator

    def minimize_scalar(*a, **kw):
        res = real_min(*a, **kw)
        nfevs.append(int(res.nfev))
        return res

    def cost_calculator(rho, point, t_event, *rest):
        c = real_cost(rho, point, t_event, *rest)
        mine_c = R.make_cost(rr, t_event, int(point[0, 0]), int(point[0, 1]))(float(rho))
        assert float(c) == mine_c, (point, rho, c, mine_c)  # (np.linalg.norm == the sequential fused sum, among the rest)
        n_cost[0] += 1
        return c

    ref.minimize_scalar, ref.cost_calculator = minimize_scalar, cost_calculator
    try:
        out = ref.depth_optimization(d0, cam, proj, rig["window_size"], calib)
    finally:
        ref.minimize_scalar, ref.cost_calculator = real_min, real_cost
    ws = rig["window_size"]
    live = np.zeros(d0.shape, bool)
    live[ws:-ws, ws:-ws] = d0[ws:-ws, ws:-ws] > 0
    assert out.dtype == np.float32 and live.sum() == len(nfevs) and sum(nfevs) == n_cost[0]
    nfev = np.zeros(d0.shape, np.uint16)
    nfev[live] = nfevs  # (boolean indexing and the reference's loops both run in raster order)
    return out, nfev


def check_cases(rigs, outs):
    """every case the fixture exists for, found in the inputs, the reference's outputs and the restatement's traces"""
    seen = set()
    for name in K.G13_RIGS:
        rig, (out, nfev) = rigs[name], outs[name]
        rr = K.ref_rig(rig)
        cam, _ = R.normalise_and_fill(rig["surface"])
        d0, ws = rig["depth_init"], rig["window_size"]
        w = ws // 2
        h, w_ = d0.shape
        norm00 = (rig["surface"][0, 0] - rig["surface"][rig["surface"] != 0].min())
        seen.add("fill_inf" if np.isinf(cam).any() else "fill_finite")
        assert np.isinf(cam).any() == (norm00 <= 0) and (cam != 0).all()
        border = np.ones(d0.shape, bool)
        border[ws:-ws, ws:-ws] = False
        if (d0[border] > 0).any():
            assert not out[border].any()
            seen.add("d0_in_border")
        if (d0[~border] == 0).any():
            assert not out[~border][d0[~border] == 0].any()
            seen.add("d0_zero")
        got, got_n, st, traces = R.depth_optim(rr, rig["surface"], d0, want_trace=True)
        assert np.array_equal(got.view(np.uint32), out.view(np.uint32)) and np.array_equal(got_n, nfev), name
        assert 200 <= st["n_optimised"] <= 300 and st["n_hit_limit"] == 0 and st["n_bad_bounds"] == 0, st
        for (y, x), tr in traces.items():
            ev = []
            diff = float(np.float64(d0[y, x] * d0[y, x]) / np.float64(rig["p1_03"]))
            R.minimize_bounded(R.make_cost(rr, cam, x, y, ev), float(d0[y, x]) - diff, float(d0[y, x]) + diff)
            assert len(ev) == nfev[y, x] == len(tr) + 1
            inside = [e[4] for e in ev]
            seen.add("always_outside" if not any(inside) else "always_inside" if all(inside) else "sometimes_outside")
            if any(-1 < c < 0 for e in ev for c in e[2:4]):
                seen.add("trunc_neg")
                assert any(e[0] == 0 and -1 < e[2] < 0 or e[1] == 0 and -1 < e[3] < 0 for e in ev)
            patch_inf = np.isinf(cam[y - w:y + w + 1, x - w:x + w + 1]).any()
            if patch_inf and any(inside):
                seen.add("inf_cost")
                if inside.count(True) >= 2 and any(s != "golden" for s, _ in tr):
                    seen.add("nan_parabola")  # (inf - inf in the fit: NaN p, q -> refused)
            for step, branch in tr:
                seen.add(step)
                seen.add(branch[:4])
                if branch.startswith("gt"):
                    seen.add("gt:" + branch.split(":")[2])
    need = {"fill_inf", "fill_finite", "d0_in_border", "d0_zero", "always_outside", "always_inside", "sometimes_outside", "trunc_neg",
            "inf_cost", "nan_parabola", "golden", "golden+rejected", "parabolic", "le:a", "le:b", "gt:a", "gt:b",
            "gt:nfc", "gt:fulc", "gt:none"}
    assert need <= seen, sorted(need - seen)
    return sorted(seen)


def main():
    assert os.path.isdir(REF_EVAL), "needs /root/reference (build container only)"
    ref = import_reference()
    rigs = {n: K.make_rig(*K.G13_SPECS[n]) for n in K.G13_RIGS}
    outs = {n: run_reference(ref, rigs[n]) for n in K.G13_RIGS}
    print("cases:", check_cases(rigs, outs))
    out = {}
    for n in K.G13_RIGS:
        rig = rigs[n]
        for k in K.RIG_KEYS:
            out[f"{n}_{k}"] = np.asarray(rig[k])
        out[f"{n}_proj_shape"] = np.array([rig["proj_w"], rig["proj_h"]], np.int32)
        out[f"{n}_window_size"] = np.int32(rig["window_size"])
        out[f"{n}_depth_optim"], out[f"{n}_nfev"] = outs[n]
        print(n, "optimised", int((outs[n][1] > 0).sum()), "nfev", int(outs[n][1][outs[n][1] > 0].min()), "..", int(outs[n][1].max()))
    path = os.path.join(HERE, K.G13)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(path, size, "bytes")
    assert size <= 117 * 1024


if __name__ == "__main__":
    main()
