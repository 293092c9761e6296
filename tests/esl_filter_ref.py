"""CPU restatement of the two filters behind ESL's depth optimisation (python/eval/compute_depth_esl.py:243-244: cv2.bilateralFilter
(depth_optim, 5, 3, 3), then esl_utilities.py:194-224 denoise_tv(mu=0.5)) -- TEST INFRASTRUCTURE ONLY; the product path is
x_maps_amd.esl_filter on the GPU (csrc/xmaps_eslfilter.hpp), whose arithmetic this file states in NumPy.

bilateral        the 32F bilateral filter as include/xmaps.h specifies it (float32 throughout, taps in raster order)
D, Dt            the reference's two backward differences WITH ITS SWAPPED dims: the H x W image is differenced as if it were W x H,
                 so "axis 0" has stride H in the flat row-major index and "axis 1" restarts every H elements
soft_threshold   max(|x| - lam, 0) * sign(x)
lsqr_restated    scipy 1.15's lsqr line for line (it keeps scipy's names, NumPy scalar types and ** 2 spellings, which is what makes
                 it bit-identical); `norm` is the vector norm it uses: np.linalg.norm, or norm_fsum (exactly rounded sums)
lsqr_scipy       the installed scipy's own lsqr on a LinearOperator of the same two products
split_bregman    pylops 1.18's SplitBregman + RegularizedInversion for Op = Identity, two L1 regularisers, x0 = xinv
Both lsqr forms record into `rec` (a Record) the trip count and istop of every inner call; the restated one also the DECISION MARGIN:
the least relative distance |test - threshold| / threshold over every `test <= threshold` decision taken (1 + t <= 1 is t <= 2^-53).
"""
import math

import numpy as np

EPS = np.finfo(np.float64).eps
MU, LAMBDAS, NITER_OUTER, NITER_INNER, TOL, TAU, ITER_LIM, DAMP = 0.5, (0.1, 0.1), 20, 10, 1e-4, 1.0, 5, 1e-4
ATOL = BTOL = 1e-6
CONLIM = 1e8
BIL_D, BIL_SIGMA_COLOR, BIL_SIGMA_SPACE, BIL_BINS = 5, 3.0, 3.0, 4096
FLT_EPSILON = float(np.finfo(np.float32).eps)


# ---- stage 1 -------------------------------------------------------------------------------------------------------------------
def bilateral_taps(d=BIL_D, sigma_space=BIL_SIGMA_SPACE):
    """[(i, j, float32 weight)] in raster order: the taps with sqrt(i*i + j*j) <= d // 2"""
    radius, coeff = d // 2, -0.5 / (sigma_space * sigma_space)
    taps = []
    for i in range(-radius, radius + 1):
        for j in range(-radius, radius + 1):
            r = math.sqrt(float(i * i + j * j))
            if r <= radius:
                taps.append((i, j, np.float32(math.exp(r * r * coeff))))
    return taps


def bilateral_table(lo, hi, sigma_color=BIL_SIGMA_COLOR, want_f64=False):
    """-> (float32 scale, float32 lut[BIL_BINS + 2]) of a surface with extrema lo < hi (float32 values)"""
    length = np.float32(float(hi) - float(lo))
    scale = np.float32(BIL_BINS) / length
    coeff = -0.5 / (sigma_color * sigma_color)
    val = (np.arange(BIL_BINS + 2, dtype=np.float32) / scale).astype(np.float64)  # (a float32 quotient, widened)
    f64 = np.array([math.exp(v * v * coeff) for v in val])
    return (scale, f64.astype(np.float32), f64) if want_f64 else (scale, f64.astype(np.float32))


def reflect101(i, n):
    """BORDER_REFLECT_101 of an index at most n - 1 outside (a dimension of 1 maps everything to 0)"""
    if n == 1:
        return 0
    while i < 0 or i >= n:
        i = -i if i < 0 else 2 * (n - 1) - i
    return i


def bilateral(img, d=BIL_D, sigma_color=BIL_SIGMA_COLOR, sigma_space=BIL_SIGMA_SPACE):
    img = np.ascontiguousarray(img, np.float32)
    H, W = img.shape
    lo, hi = img.min(), img.max()
    if abs(float(lo) - float(hi)) < FLT_EPSILON:
        return img.copy()
    scale, lut = bilateral_table(lo, hi, sigma_color)
    ri = np.array([[reflect101(r + o, H) for r in range(H)] for o in range(-(d // 2), d // 2 + 1)])
    ci = np.array([[reflect101(c + o, W) for c in range(W)] for o in range(-(d // 2), d // 2 + 1)])
    s = np.zeros((H, W), np.float32)
    ws = np.zeros((H, W), np.float32)
    with np.errstate(all="ignore"):
        for i, j, wsp in bilateral_taps(d, sigma_space):
            v = img[ri[i + d // 2]][:, ci[j + d // 2]]
            a = np.abs(v - img) * scale
            idx = np.minimum(np.maximum(a, np.float32(0)), np.float32(BIL_BINS)).astype(np.int32)  # (NaN -> 0: never outside)
            al = a - idx.astype(np.float32)
            w = wsp * (lut[idx] + al * (lut[idx + 1] - lut[idx]))
            s = s + v * w
            ws = ws + w
        return s / ws


def bilateral_bruteforce(img, d=BIL_D, sigma_color=BIL_SIGMA_COLOR, sigma_space=BIL_SIGMA_SPACE):
    """the formula the table approximates, in float64: sum v exp(-r^2 / 2 ss^2) exp(-(v - v0)^2 / 2 sc^2) / sum of the weights"""
    img = np.asarray(img, np.float64)
    H, W = img.shape
    s, ws = np.zeros((H, W)), np.zeros((H, W))
    for i, j, _ in bilateral_taps(d, sigma_space):
        ri = [reflect101(r + i, H) for r in range(H)]
        ci = [reflect101(c + j, W) for c in range(W)]
        v = img[ri][:, ci]
        w = np.exp(-(i * i + j * j) / (2 * sigma_space ** 2)) * np.exp(-((v - img) ** 2) / (2 * sigma_color ** 2))
        s += v * w
        ws += w
    return s / ws


# ---- stage 2 -------------------------------------------------------------------------------------------------------------------
def D(x, H, axis):
    """D0 x[k] = x[k] - x[k-H] (k >= H), D1 x[k] = x[k] - x[k-1] (k % H != 0), else 0"""
    y = np.zeros_like(x)
    if axis == 0:
        y[H:] = x[H:] - x[:-H]
    else:
        y[1:] = x[1:] - x[:-1]
        y[::H] = 0
    return y


def Dt(y, H, axis):
    """the adjoint: (y[k] where D has a row k) - (y[k'] where row k' reads x[k])"""
    a = y.copy()
    b = np.zeros_like(y)
    if axis == 0:
        a[:H] = 0
        b[:-H] = y[H:]
    else:
        a[::H] = 0
        b[:-1] = y[1:]
        b[H - 1::H] = 0
    return a - b


def soft_threshold(x, lam):
    return np.maximum(np.abs(x) - lam, 0) * np.sign(x)


def norm_fsum(x):
    return np.float64(math.sqrt(math.fsum((x * x).tolist())))


class Record:
    def __init__(self):
        self.trips, self.istops, self.margin, self.calls = [], [], math.inf, []

    def decide(self, test, thr):
        if thr > 0 and math.isfinite(test):
            self.margin = min(self.margin, abs(float(test) - thr) / thr)
        return test <= thr


class StackedOp:
    """A = [I; e0 D0; e1 D1] on a flat image of N pixels whose differences run with stride H and 1"""

    def __init__(self, N, H, eps):
        self.N, self.H, self.eps, self.shape = N, H, eps, (3 * N, N)

    def matvec(self, v):
        return np.concatenate((v, self.eps[0] * D(v, self.H, 0), self.eps[1] * D(v, self.H, 1)))

    def rmatvec(self, u):
        N = self.N
        y = np.zeros(N) + u[:N]
        y = y + self.eps[0] * Dt(u[N:2 * N], self.H, 0)
        return y + self.eps[1] * Dt(u[2 * N:], self.H, 1)


def _sym_ortho(a, b):
    if b == 0:
        return np.sign(a), 0, abs(a)
    elif a == 0:
        return 0, np.sign(b), abs(b)
    elif abs(b) > abs(a):
        tau = a / b
        s = np.sign(b) / math.sqrt(1 + tau * tau)
        c = s * tau
        r = b / s
    else:
        tau = b / a
        c = np.sign(a) / math.sqrt(1 + tau * tau)
        s = c * tau
        r = a / c
    return c, s, r


def lsqr_restated(A, b, damp=0.0, atol=1e-6, btol=1e-6, conlim=1e8, iter_lim=None, norm=np.linalg.norm, rec=None):
    """-> (x, istop, itn); scipy/sparse/linalg/_isolve/lsqr.py (1.15) without show, calc_var and x0"""
    sqrt = math.sqrt
    rec = rec if rec is not None else Record()
    m, n = A.shape
    if iter_lim is None:
        iter_lim = 2 * n
    itn = 0
    istop = 0
    ctol = 0
    if conlim > 0:
        ctol = 1 / conlim
    anorm = 0
    acond = 0
    dampsq = damp ** 2
    ddnorm = 0
    res2 = 0
    xnorm = 0
    xxnorm = 0
    z = 0
    cs2 = -1
    sn2 = 0
    u = b
    bnorm = norm(b)
    x = np.zeros(n)
    beta = bnorm.copy()
    if beta > 0:
        u = (1 / beta) * u
        v = A.rmatvec(u)
        alfa = norm(v)
    else:
        v = x.copy()
        alfa = 0
    if alfa > 0:
        v = (1 / alfa) * v
    w = v.copy()
    rhobar = alfa
    phibar = beta
    arnorm = alfa * beta
    if arnorm == 0:
        return x, istop, itn
    while itn < iter_lim:
        itn = itn + 1
        u = A.matvec(v) - alfa * u
        beta = norm(u)
        if beta > 0:
            u = (1 / beta) * u
            anorm = sqrt(anorm ** 2 + alfa ** 2 + beta ** 2 + dampsq)
            v = A.rmatvec(u) - beta * v
            alfa = norm(v)
            if alfa > 0:
                v = (1 / alfa) * v
        if damp > 0:
            rhobar1 = sqrt(rhobar ** 2 + dampsq)
            cs1 = rhobar / rhobar1
            sn1 = damp / rhobar1
            psi = sn1 * phibar
            phibar = cs1 * phibar
        else:
            rhobar1 = rhobar
            psi = 0.
        cs, sn, rho = _sym_ortho(rhobar1, beta)
        theta = sn * alfa
        rhobar = -cs * alfa
        phi = cs * phibar
        phibar = sn * phibar
        tau = sn * phi
        t1 = phi / rho
        t2 = -theta / rho
        dk = (1 / rho) * w
        x = x + t1 * w
        w = v + t2 * w
        ddnorm = ddnorm + norm(dk) ** 2
        delta = sn2 * rho
        gambar = -cs2 * rho
        rhs = phi - delta * z
        zbar = rhs / gambar
        xnorm = sqrt(xxnorm + zbar ** 2)
        gamma = sqrt(gambar ** 2 + theta ** 2)
        cs2 = gambar / gamma
        sn2 = theta / gamma
        z = rhs / gamma
        xxnorm = xxnorm + z ** 2
        acond = anorm * sqrt(ddnorm)
        res1 = phibar ** 2
        res2 = res2 + psi ** 2
        rnorm = sqrt(res1 + res2)
        arnorm = alfa * abs(tau)
        test1 = rnorm / bnorm
        test2 = arnorm / (anorm * rnorm + EPS)
        test3 = 1 / (acond + EPS)
        t1 = test1 / (1 + anorm * xnorm / bnorm)
        rtol = btol + atol * anorm * xnorm / bnorm
        if itn >= iter_lim:
            istop = 7
        if 1 + test3 <= 1:
            istop = 6
        if 1 + test2 <= 1:
            istop = 5
        if 1 + t1 <= 1:
            istop = 4
        for t in (test3, test2, t1):
            rec.decide(t, EPS / 2)
        if rec.decide(test3, ctol):
            istop = 3
        if rec.decide(test2, atol):
            istop = 2
        if rec.decide(test1, rtol):
            istop = 1
        if istop != 0:
            break
    return x, istop, itn


def lsqr_scipy(A, b, damp=0.0, atol=1e-6, btol=1e-6, conlim=1e8, iter_lim=None, rec=None):
    from scipy.sparse.linalg import LinearOperator, lsqr
    op = LinearOperator(A.shape, matvec=A.matvec, rmatvec=A.rmatvec, dtype=np.float64)
    r = lsqr(op, b, damp=damp, atol=atol, btol=btol, conlim=conlim, iter_lim=iter_lim)
    return r[0], r[1], r[2]


def split_bregman(y, H, mu=MU, lambdas=LAMBDAS, niter_outer=NITER_OUTER, niter_inner=NITER_INNER, tol=TOL, tau=TAU, iter_lim=ITER_LIM,
                  damp=DAMP, lsqr=lsqr_restated, rec=None, **kw):
    """y: flat float64 image; H: the stride of difference 0 (the image's HEIGHT under the reference's swap, its width without).
    -> (x, info) with info = {n_outer, n_lsqr, sum_itn, istop_count[8], final_norm, trips u8 [niter_outer * niter_inner], margin}"""
    rec = rec if rec is not None else Record()
    N = y.size
    eps = [np.sqrt(lam / 2) / np.sqrt(mu / 2) for lam in lambdas]
    A = StackedOp(N, H, eps)
    b = [np.zeros(N), np.zeros(N)]
    d = [np.zeros(N), np.zeros(N)]
    x = np.zeros(N)
    xold = np.inf * np.ones(N)
    it, nrm = 0, math.inf
    first = len(rec.trips)
    while True:
        nrm = np.linalg.norm(x - xold) if "norm" not in kw else kw["norm"](x - xold)
        if it > 0:
            rec.decide(nrm, tol)
        if not (nrm > tol and it < niter_outer):
            break
        xold = x
        for _ in range(niter_inner):
            rhs = np.concatenate([y] + [eps[i] * (d[i] - b[i]) for i in range(2)]) - A.matvec(x)
            dx, istop, itn = lsqr(A, rhs, damp=damp, atol=ATOL, btol=BTOL, conlim=CONLIM, iter_lim=iter_lim, rec=rec, **kw)
            rec.trips.append(itn)
            rec.istops.append(istop)
            rec.calls.append((rhs, dx))
            x = x + dx
            d = [soft_threshold(D(x, H, i) + b[i], lambdas[i]) for i in range(2)]
        b = [b[i] + tau * (D(x, H, i) - d[i]) for i in range(2)]
        it += 1
    trips = np.full(niter_outer * niter_inner, 0xFF, np.uint8)
    mine = rec.trips[first:]
    trips[:len(mine)] = mine
    info = {"n_outer": it, "n_lsqr": len(mine), "sum_itn": int(sum(mine)), "istop_count": np.bincount(rec.istops[first:], minlength=8),
            "final_norm": float(nrm), "trips": trips, "margin": rec.margin}
    return x, info


def denoise_tv(img, swapped=True, **kw):
    """esl_utilities.py:194-224 on an H x W map -> (float64 H x W, info); swapped=False differences the image as it lies"""
    img = np.asarray(img)
    H, W = img.shape
    x, info = split_bregman(img.astype(np.float64).ravel(), H if swapped else W, **kw)
    return x.reshape(H, W), info


def esl_filter(img, no_bilateral=False, no_tv=False, **kw):
    """both stages -> (float64 H x W, float32 bilateral | None, info | None)"""
    img = np.ascontiguousarray(img, np.float32)
    bil = None if no_bilateral else bilateral(img)
    mid = img if no_bilateral else bil
    if no_tv:
        return mid.astype(np.float64), bil, None
    out, info = denoise_tv(mid, **kw)
    return out, bil, info
