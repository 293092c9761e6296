#!/usr/bin/env python3
"""Generate tests/golden/g14_esl_filter.npz by RUNNING THE REFERENCE'S OWN utils.denoise_tv (python/eval/esl_utilities.py:194-224)
on the installed scipy's lsqr.

Run only in the build container (needs /root/reference, which does not exist on the GPU box):
    python tests/golden/make_golden_esl_filter.py
esl_utilities imports cv2 and pylops at its top; neither is installed.  cv2 becomes a stub of the one call made here; pylops becomes
a stub module of the three names denoise_tv uses -- Identity, FirstDerivative and optimization.sparsity.SplitBregman -- which are
the operators and the loop of tests/esl_filter_ref.py with scipy's REAL lsqr inside (lsqr_scipy), and which ASSERT the arguments the
reference hands them: dims, dir, kind, edge, niter, niterinner, mu, epsRL1s, tol, tau, iter_lim, damp.  Nothing from /root/reference
is copied: the .npz holds inputs and the outputs the reference's function produced for them.

PINNED: the reference's call and its dims swap (dims = (ny, nx) with nx, ny = y.shape: the stub differences with the strides the
dims it is GIVEN imply, so an H x W image is differenced as if it were W x H); every parameter; scipy's solver.
UNPINNED: pylops' roughly 30 lines of outer loop, the stacking of [Op; eps R], the backward stencil and the soft threshold (the
restatement's max(|x| - lam, 0) * sign(x); pylops may spell it x / (|x| + tiny) * max(.)); its float32 operator dtype, which may
round D x to float32 there; cv2's bilateral filter (the stub is the restatement's).  tools/pin_thirdparty.py records both filters'
outputs on this fixture's inputs where cv2 / pylops exist.

compute_depth_esl.py:243-244 sit in the reference's main(), not in a function; they are restated here (the G7 / G11 convention).

The script REFUSES to write a fixture (a) whose decision margin -- the least relative distance of any `test <= threshold` decision
of lsqr or of the outer loop from its threshold, taken by the line-for-line restatement, which this script first shows equal to
scipy's lsqr on every inner call -- is below 1e-6: the trip counts would not be a robust pin; (b) one of whose colour-table entries
lies, in float64, within 1e-8 of a float32 SPACING of a float32 rounding boundary: another exp could round it the other way.  (The
distance is measured in spacings, not relative to the value: with some 2000 non-zero entries per table and spacings of 6e-8 .. 1.2e-7
of the value, a distance below 1e-9 of the VALUE occurs in every table -- 3.6e-11 on scene a -- so that reading would refuse every
fixture.  1e-8 of a spacing is 3 to 10 float64 spacings of the value, beyond what two correctly working exp routines differ by.)"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import esl_filter_cases as K  # noqa: E402
import esl_filter_ref as R  # noqa: E402

REF_EVAL = "/root/reference/python/eval"
RECORDS = []


def pylops_stub():
    m = types.ModuleType("pylops")

    class Identity:
        def __init__(self, n):
            self.n = n

    class FirstDerivative:
        def __init__(self, N, dims=None, dir=0, edge=False, kind="centered", dtype="float64"):
            assert kind == "backward" and edge is False and dtype is np.float32 and len(dims) == 2 and N == dims[0] * dims[1]
            self.N, self.dims, self.dir = N, tuple(dims), dir

    def SplitBregman(Op, RegsL1, data, niter_outer=3, niter_inner=5, mu=1.0, epsRL1s=None, tol=1e-10, tau=1.0, show=False, **kw):
        assert isinstance(Op, Identity) and Op.n == data.size and data.ndim == 1
        assert [r.dir for r in RegsL1] == [0, 1] and RegsL1[0].dims == RegsL1[1].dims and RegsL1[0].N == data.size
        assert (niter_outer, niter_inner, mu, list(epsRL1s), tol, tau, show) == (R.NITER_OUTER, R.NITER_INNER, R.MU, list(R.LAMBDAS), R.TOL,
                                                                                  R.TAU, False)
        assert kw == {"iter_lim": R.ITER_LIM, "damp": R.DAMP}
        # axis 0 of a C-ordered dims array has stride dims[1], axis 1 stride 1 and period dims[1]
        rec = R.Record()
        x, info = R.split_bregman(np.asarray(data, np.float64), RegsL1[0].dims[1], mu=mu, lambdas=tuple(epsRL1s), niter_outer=niter_outer,
                                  niter_inner=niter_inner, tol=tol, tau=tau, lsqr=R.lsqr_scipy, rec=rec, **kw)
        RECORDS.append((RegsL1[0].dims, info, rec))
        return x, info["n_outer"]

    m.Identity, m.FirstDerivative = Identity, FirstDerivative
    m.optimization = types.ModuleType("pylops.optimization")
    m.optimization.sparsity = types.ModuleType("pylops.optimization.sparsity")
    m.optimization.sparsity.SplitBregman = SplitBregman
    return m


def cv2_stub():
    m = types.ModuleType("cv2")

    def bilateralFilter(src, d, sigmaColor, sigmaSpace):
        assert src.dtype == np.float32 and (d, sigmaColor, sigmaSpace) == (5, 3, 3)
        return R.bilateral(src, d, float(sigmaColor), float(sigmaSpace))

    m.bilateralFilter = bilateralFilter
    return m


def import_reference():
    sys.modules["cv2"] = cv2_stub()
    pl = pylops_stub()
    sys.modules["pylops"], sys.modules["pylops.optimization"] = pl, pl.optimization
    sys.modules["pylops.optimization.sparsity"] = pl.optimization.sparsity
    sys.path.insert(0, REF_EVAL)
    import esl_utilities
    assert esl_utilities.pylops is pl
    return esl_utilities.utils, sys.modules["cv2"]


def table_margin(img):
    """the least distance of a colour-table entry's float64 value from a float32 rounding boundary, in float32 spacings there"""
    lo, hi = img.min(), img.max()
    if abs(float(lo) - float(hi)) < R.FLT_EPSILON:
        return np.inf
    _, f32, f64 = R.bilateral_table(lo, hi, want_f64=True)
    worst = np.inf
    for a, v in zip(f32, f64):
        if v == 0.0:
            continue
        for nb in (np.nextafter(a, np.float32(np.inf)), np.nextafter(a, np.float32(-np.inf))):
            mid = (float(a) + float(nb)) / 2
            worst = min(worst, abs(v - mid) / abs(float(a) - float(nb)))
    return worst


def run_reference(ut, cv2, img):
    """-> (bilateral, filtered, info): compute_depth_esl.py:243-244 on one depth_optim map"""
    depth_optim = img.copy()
    depth_optim = cv2.bilateralFilter(depth_optim, 5, 3, 3)  # :243
    bil = depth_optim
    depth_optim = ut.denoise_tv(depth_optim, mu=0.5)          # :244
    dims, info, rec = RECORDS[-1]
    assert dims == (img.shape[1], img.shape[0]), "the reference's dims swap"
    assert depth_optim.dtype == np.float64 and depth_optim.shape == img.shape
    # the restatement, line for line, equals scipy's lsqr on every inner call -- x, istop, itn -- and gives the margin
    mine = R.Record()
    x, my_info = R.denoise_tv(bil, rec=mine)
    assert np.array_equal(x, depth_optim) and mine.trips == rec.trips and mine.istops == rec.istops
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(mine.calls, rec.calls))
    return bil, depth_optim, my_info


def main():
    assert os.path.isdir(REF_EVAL), "needs /root/reference (build container only)"
    ut, cv2 = import_reference()
    out, seen_trips, seen_istop = {}, set(), set()
    for name, (H, W, seed) in K.G14_SCENES.items():
        img = K.scene(H, W, seed)
        bil, filt, info = run_reference(ut, cv2, img)
        tm = table_margin(img)
        print(name, (H, W), "outer", info["n_outer"], "lsqr", info["n_lsqr"], "itn", info["sum_itn"], "istop", list(info["istop_count"]),
              "decision margin %.3e" % info["margin"], "table margin %.3e" % tm)
        assert info["margin"] >= 1e-6, "REFUSED: a stopping decision sits within 1e-6 of its threshold"
        assert tm >= 1e-8, "REFUSED: a colour-table entry sits within 1e-8 of a spacing of a float32 rounding boundary"
        seen_trips |= set(int(t) for t in info["trips"] if t != 0xFF)
        seen_istop |= set(int(i) for i in np.nonzero(info["istop_count"])[0])
        out[f"{name}_input"], out[f"{name}_bilateral"], out[f"{name}_filtered"], out[f"{name}_trips"] = img, bil, filt, info["trips"]
    assert seen_trips == {1, 2, 3, 4, 5} and seen_istop == {2, 7}, (seen_trips, seen_istop)
    # stage 2 alone on the smallest scene: what XM_ESL_FILTER_NO_BILATERAL computes
    img = out["a_input"]
    out["a_tv_only"] = ut.denoise_tv(img, mu=0.5)
    out["a_tv_only_trips"] = RECORDS[-1][1]["trips"]
    assert R.denoise_tv(img)[1]["margin"] >= 1e-6  # (the restatement's: scipy's own lsqr records no margins)
    path = os.path.join(HERE, K.G14)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(path, size, "bytes")
    assert size <= 400 * 1024


if __name__ == "__main__":
    main()
