"""Seeded scenes for the ESL filters' CPU and GPU tests: depth_optim maps as the solver leaves them -- a slanted plane with a depth
step, noise, and about 15 % pixels at 0 (no initial depth, hence not optimised) -- plus the three maps that end the TV loop early.
The generator of golden G14 stores the three G14 scenes with the reference's outputs; load_g14 reads them back."""
import os

import numpy as np

G14 = "g14_esl_filter.npz"
G14_SCENES = {"a": (20, 24, 141), "b": (48, 40, 142), "c": (96, 80, 143)}  # name -> (H, W, seed)


def scene(H, W, seed, zeros=0.15):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    z = 60.0 + 0.3 * (xx - W / 2) - 0.2 * (yy - H / 2)
    z = z + np.where(xx + 0.5 * yy > 0.6 * W, 7.5, 0.0)  # the step
    z = z * (1.0 + 0.01 * rng.standard_normal((H, W)))
    z[rng.random((H, W)) < zeros] = 0
    return z.astype(np.float32)


def zero_map(H, W):
    return np.zeros((H, W), np.float32)


def constant_map(H, W, value=58.25):
    return np.full((H, W), value, np.float32)


def ramp(H, W):
    """a ramp steeper than the thresholds flatten: the TV loop ends through tol well before niter_outer"""
    yy, xx = np.mgrid[0:H, 0:W]
    return (3.0 + 0.2 * xx + 0.3 * yy).astype(np.float32)


def group(H, W, n, seed=150):
    """n maps: a zero map, a constant map and the ramp between full-length scenes, so stopped surfaces sit beside running ones"""
    maps = [scene(H, W, seed), zero_map(H, W), constant_map(H, W), ramp(H, W), scene(H, W, seed + 1)]
    return np.ascontiguousarray(np.stack(maps[:n]))


def load_g14(golden_dir):
    """name -> {input, bilateral, filtered, trips}; scene a also holds tv_only and tv_only_trips (stage 2 alone on the input)"""
    g = np.load(os.path.join(golden_dir, G14))
    return {n: {k[len(n) + 1:]: g[k] for k in g.files if k.startswith(n + "_")} for n in G14_SCENES}
