"""The ESL depth optimisation in explicit scalar float64 steps: what xm_esl_optim_* computes (csrc/xmaps_esloptim.hpp) and what the
reference's depth_optimization (python/eval/compute_depth_esl.py:104-129) computes through scipy's minimize_scalar(method="bounded").

Three parts, none of which touches BLAS or LAPACK (no @, no np.dot, no linalg):
  * minimize_bounded: scipy 1.15's _minimize_scalar_bounded, operation for operation, with a trace of the step kinds;
  * the geometry the reference takes from cv2 -- undistort_points (five fixed-point rounds, the result rounded to float32 as
    OpenCV returns the input's depth), rodrigues_vector / rodrigues_matrix, project_points -- each spelt out element by element.
    The generator of golden G13 hands exactly these to the reference as its cv2; a real cv2 has not been compared (UNPINNED);
  * cost and depth_optim: the reference's cost_calculator and its caller, with the patch norm as sequential fused steps
    s = fma(d, d, s) -- what np.linalg.norm's nine-element dot gives (the generator asserts that on every patch it evaluates).
Python floats are IEEE float64 and every expression below is written in the order it is evaluated."""
import math
from fractions import Fraction

import numpy as np

XATOL, MAX_ITER, WINDOW = 1e-5, 500, 3
OUTSIDE = 100000.0
SQRT_EPS = math.sqrt(2.2e-16)
GOLDEN_MEAN = 0.5 * (3.0 - math.sqrt(5.0))
STAT_KEYS = ("n_optimised", "n_evals", "n_hit_limit", "n_bad_bounds", "lo", "hi")


def fma(a, b, c):
    """a * b + c rounded once (math.fma arrives with Python 3.13): exact rationals, rounded to nearest even by float()"""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c  # (inf / NaN: no rounding is involved)
    try:
        return float(Fraction(a) * Fraction(b) + Fraction(c))
    except OverflowError:
        return math.inf if (a > 0) == (b > 0) else -math.inf


def _sign(v):
    """np.sign: NaN stays NaN"""
    return 1.0 if v > 0 else -1.0 if v < 0 else 0.0 if v == 0 else math.nan


def _maximum(a, b):
    """np.maximum: NaN if either is"""
    return math.nan if (a != a or b != b) else (a if a >= b else b)


def minimize_bounded(func, x1, x2, xatol=XATOL, maxfun=MAX_ITER):
    """-> (xf, nfev, hit_limit, trace); trace: one (step, branch) per evaluation behind the first.  step: "golden", "parabolic"
    or "parabolic_tol1" (a parabolic step within tol2 of a bound, replaced by tol1 towards the middle), with "+rejected" appended to
    golden when a parabola was fitted and refused.  branch: which way the three-point bookkeeping went."""
    a, b = x1, x2
    fulc = a + GOLDEN_MEAN * (b - a)
    nfc, xf = fulc, fulc
    rat = e = 0.0
    x = xf
    fx = func(x)
    num = 1
    ffulc = fnfc = fx
    xm = 0.5 * (a + b)
    tol1 = SQRT_EPS * abs(xf) + xatol / 3.0
    tol2 = 2.0 * tol1
    trace, hit = [], False
    while abs(xf - xm) > (tol2 - 0.5 * (b - a)):
        golden = True
        step = "golden"
        if abs(e) > tol1:
            golden = False
            r = (xf - nfc) * (fx - ffulc)
            q = (xf - fulc) * (fx - fnfc)
            p = (xf - fulc) * q - (xf - nfc) * r
            q = 2.0 * (q - r)
            if q > 0.0:
                p = -p
            q = abs(q)
            r = e
            e = rat
            if (abs(p) < abs(0.5 * q * r)) and (p > q * (a - xf)) and (p < q * (b - xf)):
                rat = (p + 0.0) / q
                x = xf + rat
                step = "parabolic"
                if ((x - a) < tol2) or ((b - x) < tol2):
                    si = _sign(xm - xf) + (1.0 if (xm - xf) == 0 else 0.0)
                    rat = tol1 * si
                    step = "parabolic_tol1"
            else:
                golden = True
                step = "golden+rejected"
        if golden:
            if xf >= xm:
                e = a - xf
            else:
                e = b - xf
            rat = GOLDEN_MEAN * e
        si = _sign(rat) + (1.0 if rat == 0 else 0.0)
        x = xf + si * _maximum(abs(rat), tol1)
        fu = func(x)
        num += 1
        if fu <= fx:
            if x >= xf:
                a = xf
                branch = "le:a"
            else:
                b = xf
                branch = "le:b"
            fulc, ffulc = nfc, fnfc
            nfc, fnfc = xf, fx
            xf, fx = x, fu
        else:
            if x < xf:
                a = x
                branch = "gt:a"
            else:
                b = x
                branch = "gt:b"
            if (fu <= fnfc) or (nfc == xf):
                fulc, ffulc = nfc, fnfc
                nfc, fnfc = x, fu
                branch += ":nfc"
            elif (fu <= ffulc) or (fulc == xf) or (fulc == nfc):
                fulc, ffulc = x, fu
                branch += ":fulc"
            else:
                branch += ":none"
        trace.append((step, branch))
        xm = 0.5 * (a + b)
        tol1 = SQRT_EPS * abs(xf) + xatol / 3.0
        tol2 = 2.0 * tol1
        if num >= maxfun:
            hit = True
            break
    return xf, num, hit, trace


# ---- the geometry (the reference's cv2 calls) ------------------------------------------------------------------------------------
def undistort_points(px, py, K, D):
    """cv2.undistortPoints((px, py) float32, K, D, P = K): five fixed-point rounds in float64, the result rounded to float32"""
    fx, fy, cx, cy = float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2])
    k1, k2, p1, p2, k3 = (float(v) for v in D)
    x0 = (float(px) - cx) / fx
    y0 = (float(py) - cy) / fy
    x, y = x0, y0
    for _ in range(5):
        r2 = x * x + y * y
        icdist = 1.0 / (1.0 + r2 * (k1 + r2 * (k2 + r2 * k3)))
        dx = ((2.0 * p1) * x) * y + p2 * (r2 + (2.0 * x) * x)
        dy = p1 * (r2 + (2.0 * y) * y) + ((2.0 * p2) * x) * y
        x = (x0 - dx) * icdist
        y = (y0 - dy) * icdist
    return np.float32(fx * x + cx), np.float32(fy * y + cy)


def _orthogonal_factor(R):
    """the rotation next to a nearly orthogonal 3 x 3 matrix (its polar factor, what cv2.Rodrigues takes from an SVD): four Newton
    rounds X <- (X + X^-T) / 2, the inverse transpose by cofactors"""
    X = [[float(R[i][j]) for j in range(3)] for i in range(3)]
    for _ in range(4):
        c = [[X[(i + 1) % 3][(j + 1) % 3] * X[(i + 2) % 3][(j + 2) % 3] - X[(i + 1) % 3][(j + 2) % 3] * X[(i + 2) % 3][(j + 1) % 3]
              for j in range(3)] for i in range(3)]
        det = (X[0][0] * c[0][0] + X[0][1] * c[0][1]) + X[0][2] * c[0][2]
        X = [[0.5 * (X[i][j] + c[i][j] / det) for j in range(3)] for i in range(3)]
    return X


def rodrigues_vector(R):
    """cv2.Rodrigues(matrix) -> rotation vector (the half-turn case is not needed by any rig and not spelt out)"""
    r = _orthogonal_factor(R)
    v = (r[2][1] - r[1][2], r[0][2] - r[2][0], r[1][0] - r[0][1])
    s = math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) * 0.5
    c = (((r[0][0] + r[1][1]) + r[2][2]) - 1.0) * 0.5
    c = 1.0 if c > 1.0 else -1.0 if c < -1.0 else c
    theta = math.acos(c)
    if s < 1e-12:
        if c > 0:
            return (0.0, 0.0, 0.0)
        raise NotImplementedError("a rotation by pi")
    f = (0.5 / s) * theta
    return (v[0] * f, v[1] * f, v[2] * f)


def rodrigues_matrix(v):
    """cv2.Rodrigues(vector) -> matrix: cos I + (1 - cos) k k^T + sin [k]x, element by element"""
    theta = math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    if theta < 1e-15:
        return [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    k = (v[0] / theta, v[1] / theta, v[2] / theta)
    c, s = math.cos(theta), math.sin(theta)
    kx = [[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]]
    return [[(c * (1.0 if i == j else 0.0) + (1.0 - c) * (k[i] * k[j])) + s * kx[i][j] for j in range(3)] for i in range(3)]


def make_rt(R, T):
    """Rt[12] as the device takes it: the Rodrigues round trip of the float32-rounded rotation, rows first, then the float32-rounded
    translation (esl_utilities.py:144-146 keeps both in a float32 matrix; cost_calculator sends the rotation through cv2.Rodrigues
    and cv2.projectPoints turns it back)"""
    R32 = np.asarray(R, np.float64).astype(np.float32)
    t32 = np.asarray(T, np.float64).reshape(3).astype(np.float32)
    Rr = rodrigues_matrix(rodrigues_vector(R32))
    return np.array([Rr[i][j] for i in range(3) for j in range(3)] + [float(t) for t in t32], np.float64)


def project_points(X, Y, Z, Rt, K, D):
    """cv2.projectPoints of one point: R' (X, Y, Z) + t, perspective divide, Brown distortion, K"""
    fx, fy, cx, cy = float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2])
    k1, k2, p1, p2, k3 = (float(v) for v in D)
    xc = ((Rt[0] * X + Rt[1] * Y) + Rt[2] * Z) + Rt[9]
    yc = ((Rt[3] * X + Rt[4] * Y) + Rt[5] * Z) + Rt[10]
    zc = ((Rt[6] * X + Rt[7] * Y) + Rt[8] * Z) + Rt[11]
    with np.errstate(all="ignore"):
        xc, yc, zc = np.float64(xc), np.float64(yc), np.float64(zc)  # (division by zero gives inf / NaN as in NumPy, no exception)
        x, y = float(xc / zc), float(yc / zc)
    r2 = x * x + y * y
    radial = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
    xd = (x * radial + ((2.0 * p1) * x) * y) + p2 * (r2 + (2.0 * x) * x)
    yd = (y * radial + p1 * (r2 + (2.0 * y) * y)) + ((2.0 * p2) * x) * y
    return fx * xd + cx, fy * yd + cy


def trunc_i32(v):
    """float64 -> int32 by truncation toward zero; None for a value that is not finite or not representable"""
    if not math.isfinite(v) or not (-2147483649.0 < v < 2147483648.0):
        return None
    return int(v)


class Rig:
    """the constants of one camera / projector pair as the cost needs them"""

    def __init__(self, cam_K, cam_D, proj_K, proj_D, Rt, proj, p1_03, window_size=WINDOW):
        self.cam_K, self.proj_K = np.asarray(cam_K, np.float64), np.asarray(proj_K, np.float64)
        self.cam_D, self.proj_D = np.asarray(cam_D, np.float64).ravel(), np.asarray(proj_D, np.float64).ravel()
        self.Rt = [float(v) for v in np.asarray(Rt, np.float64).ravel()]
        self.proj = np.asarray(proj, np.float32)
        self.p1_03, self.ws = float(p1_03), int(window_size)


def make_cost(rig, cam, x, y, seen=None):
    """cost_calculator for camera pixel (x, y) of the filled image cam (float64) as a function of rho.  seen (a list) collects
    (xp, yp, u, v, inside) per evaluation."""
    w = int(rig.ws / 2)
    pu_x, pu_y = undistort_points(np.float32(x), np.float32(y), rig.cam_K, rig.cam_D)
    cx, cy, fx, fy = float(rig.cam_K[0][2]), float(rig.cam_K[1][2]), float(rig.cam_K[0][0]), float(rig.cam_K[1][1])
    ph, pw = rig.proj.shape
    patch = [[float(cam[y + i][x + j]) for j in range(-w, w + 1)] for i in range(-w, w + 1)]

    def cost(rho):
        X = ((float(pu_x) - cx) / fx) * rho
        Y = ((float(pu_y) - cy) / fy) * rho
        u, v = project_points(X, Y, rho, rig.Rt, rig.proj_K, rig.proj_D)
        xp, yp = trunc_i32(u), trunc_i32(v)
        inside = xp is not None and yp is not None and yp - w > 0 and yp + w < ph and xp - w > 0 and xp + w < pw
        if seen is not None:
            seen.append((xp, yp, u, v, inside))
        if not inside:
            return OUTSIDE
        s = 0.0
        for i in range(2 * w + 1):
            for j in range(2 * w + 1):
                d = patch[i][j] - float(rig.proj[yp - w + i][xp - w + j])
                s = fma(d, d, s)
        return math.sqrt(s)
    return cost


def normalise_and_fill(surface):
    """compute_depth_esl.py:207-212 on the surface widened to float64 -> the filled image, or None for a surface that cannot be
    normalised (all zero, or a single non-zero value: defined as a zero map)"""
    s = np.asarray(surface).astype(np.float64)
    nz = s[s != 0]
    if nz.size == 0 or not nz.max() > nz.min():
        return None, (float(nz.min()) if nz.size else 0.0, float(nz.max()) if nz.size else 0.0)
    lo, hi = float(nz.min()), float(nz.max())
    with np.errstate(all="ignore"):
        v = (s - lo) / (hi - lo)
        v[v < 0] = 0
        f = np.float64(1.0) / v[0, 0]
        v[v == 0] = f
    return v, (lo, hi)


def depth_optim(rig, surface, depth_init, xatol=XATOL, max_iter=MAX_ITER, want_trace=False):
    """-> (depth_optim f32, nfev u16, stats dict[, traces {(y, x): trace}])"""
    d0 = np.asarray(depth_init)
    assert d0.dtype == np.float32
    h, w_ = d0.shape
    out, nfev = np.zeros((h, w_), np.float32), np.zeros((h, w_), np.uint16)
    cam, (lo, hi) = normalise_and_fill(surface)
    st = dict(n_optimised=0, n_evals=0, n_hit_limit=0, n_bad_bounds=0, lo=lo, hi=hi)
    traces = {}
    if cam is not None:
        ws = rig.ws
        for y in range(ws, h - ws):
            for x in range(ws, w_ - ws):
                if not d0[y, x] > 0:
                    continue
                with np.errstate(all="ignore"):
                    diff = float(np.float64(d0[y, x] * d0[y, x]) / np.float64(rig.p1_03))  # (float32 product, float64 quotient)
                a, b = float(d0[y, x]) - diff, float(d0[y, x]) + diff
                if not (math.isfinite(a) and math.isfinite(b)) or a > b:
                    st["n_bad_bounds"] += 1
                    continue
                xf, n, hit, tr = minimize_bounded(make_cost(rig, cam, x, y), a, b, xatol, max_iter)
                with np.errstate(all="ignore"):
                    out[y, x] = np.float32(xf)
                nfev[y, x] = n
                st["n_optimised"] += 1
                st["n_evals"] += n
                st["n_hit_limit"] += int(hit)
                traces[y, x] = tr
    return (out, nfev, st, traces) if want_trace else (out, nfev, st)
