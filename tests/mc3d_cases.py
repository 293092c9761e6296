"""MC3D rigs for the CPU and GPU tests: the three rigs of golden G12 (float maps, surfaces and the reference's own disparities and
depths; see tests/golden/make_golden_mc3d.py for what each holds) with their int32 maps, surfaces for the median (dense enough
that medians survive, every border and corner lit) and groups holding the degenerate surfaces."""
import os

import numpy as np

G12 = "g12_mc3d.npz"
RIGS = ("a", "b", "c")
P1_03 = (5821.0837, -5821.0837)  # (the fixture's two signs: "pos", "neg")


def load_rigs(golden_dir, int_maps):
    """name -> dict of one rig; int_maps: the float -> int32 pair conversion under test or its restatement"""
    g = np.load(os.path.join(golden_dir, G12))
    rigs = {}
    for r in RIGS:
        W, H = (int(v) for v in g[f"{r}_proj_shape"])
        cam_h, cam_w = g[f"{r}_cam_mapx"].shape
        rigs[r] = {"name": r, "proj_w": W, "proj_h": H, "cam_w": cam_w, "cam_h": cam_h,
                   "cam_map": int_maps(g[f"{r}_cam_mapx"], g[f"{r}_cam_mapy"]), "proj_map": int_maps(g[f"{r}_proj_mapx"], g[f"{r}_proj_mapy"]),
                   "cam_map_f": (g[f"{r}_cam_mapx"], g[f"{r}_cam_mapy"]), "proj_map_f": (g[f"{r}_proj_mapx"], g[f"{r}_proj_mapy"]),
                   "surf_f32": g[f"{r}_surf_f32"], "surf_f64": g[f"{r}_surf_f64"], "disp_f32": g[f"{r}_disp_f32"],
                   "disp_f64": g[f"{r}_disp_f64"], "depth_pos": g[f"{r}_depth_pos"], "depth_neg": g[f"{r}_depth_neg"]}
    rigs["a"]["tags"] = {t.split(":")[0]: (int(t.split(":")[1]), int(t.split(":")[2])) for t in g["a_tags"]}
    return rigs


def tables(rig, p1_03, **kw):
    return dict({k: rig[k] for k in ("cam_w", "cam_h", "proj_w", "proj_h", "cam_map", "proj_map")}, p1_03=p1_03, **kw)


def dense_surface(rig, dtype, seed):
    """a surface for the median: two pixels of three lit with values that name projector pixels all over the table, every pixel
    of the outer ring lit, a few values >= 1 and negative ones among them"""
    rng = np.random.default_rng(seed)
    h, w, wh = rig["cam_h"], rig["cam_w"], rig["proj_w"] * rig["proj_h"]
    s = (rng.integers(0, wh, (h, w)) + rng.random((h, w))) / wh
    s[rng.random((h, w)) < 0.35] = 0
    ring = np.ones((h, w), bool)
    ring[1:-1, 1:-1] = False
    s[ring & (s == 0)] = (17 + 0.5) / wh
    s[rng.random((h, w)) < 0.03] = 1.25
    s[rng.random((h, w)) < 0.03] = -0.5
    for i, j in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):  # (the corners stay lit whatever the sprinkling did)
        s[i, j] = (29 + 0.5) / wh
    return np.ascontiguousarray(s.astype(dtype))


def group(rig, dtype, n=5):
    """n surfaces: the fixture's, an all-zero one, one of values >= 1 (1, 2.5, +inf), two dense ones"""
    h, w = rig["cam_h"], rig["cam_w"]
    ge1 = np.full((h, w), 1.0)
    ge1[::2, ::3], ge1[1::2, 1::3] = 2.5, np.inf
    out = [rig["surf_f32" if dtype == np.float32 else "surf_f64"], np.zeros((h, w)), ge1, dense_surface(rig, dtype, 1), dense_surface(rig, dtype, 2)]
    return np.ascontiguousarray(np.stack([np.asarray(a).astype(dtype) for a in out[:n]]))
