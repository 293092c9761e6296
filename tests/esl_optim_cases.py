"""Rigs for the ESL depth optimisation's CPU and GPU tests: small camera / projector pairs whose camera pixels, at the depths of
their depth_init map, project into, across the rim of and beside the projector's time surface.  make_rig builds one from a seed
(the generator of golden G13 stores three of them with the reference's outputs; load_g13 reads those back), so the seeded rigs of the
GPU tests and the fixture's share one construction."""
import os

import numpy as np

import esl_optim_ref as R

G13 = "g13_esl_optim.npz"
G13_RIGS = ("a", "b", "c")
# name -> (camera w, h, projector w, h, seed, is pixel (0, 0) lit, distortion on).  The camera sees more than the projector covers.
G13_SPECS = {"a": (28, 20, 40, 64, 131, False, True), "b": (28, 20, 40, 64, 132, True, True), "c": (26, 21, 40, 64, 133, False, False)}
RIG_KEYS = ("cam_K", "cam_D", "proj_K", "proj_D", "R", "T", "Rt", "p1_03", "surface", "depth_init")


def projector_time_surface(proj_w, proj_h):
    """compute_depth_esl.py:94-101 (x_maps_amd.esl_init.get_projector_time_surface restates the same)"""
    x, y = np.meshgrid(np.arange(proj_w, dtype=np.int64), np.arange(proj_h, dtype=np.int64))
    return ((x * proj_h + y) / float(proj_w * proj_h)).astype(np.float32)


def make_rig(cam_w, cam_h, proj_w, proj_h, seed, lit00=False, distortion=True, window_size=3):
    rng = np.random.default_rng(seed)
    jit = lambda s: 1.0 + s * (rng.random() - 0.5)
    cam_K = np.array([[1.2 * cam_w * jit(0.05), 0, 0.49 * cam_w], [0, 1.2 * cam_w * jit(0.05), 0.48 * cam_h], [0, 0, 1]])
    proj_K = np.array([[1.75 * proj_w * jit(0.05), 0, 0.49 * proj_w], [0, 1.8 * proj_w * jit(0.05), 0.49 * proj_h], [0, 0, 1]])
    cam_D = np.array([-0.08, 0.02, 0.001, -0.0015, 0.0]) * (jit(0.2) if distortion else 0.0)
    proj_D = np.array([0.03, -0.01, 0.0008, 0.0005, 0.0]) * (jit(0.2) if distortion else 0.0)
    rv = (0.02 * jit(1), -0.12 * jit(0.3), 0.01 * jit(1))
    Rm = np.array(R.rodrigues_matrix(rv))
    T = np.array([10.0 * jit(0.1), 0.5 * jit(1), 1.0 * jit(1)])
    Rt = R.make_rt(Rm, T)
    p1_03 = 300.0 * jit(0.2)
    proj = projector_time_surface(proj_w, proj_h)
    rig = R.Rig(cam_K, cam_D, proj_K, proj_D, Rt, proj, p1_03, window_size)
    # the scene: a tilted plane; the camera's time surface is the projector's time where the plane's point is lit
    yy, xx = np.mgrid[0:cam_h, 0:cam_w]
    true_z = 60.0 + 0.3 * (xx - cam_w / 2) - 0.2 * (yy - cam_h / 2)
    surface = np.zeros((cam_h, cam_w), np.float64)
    for y in range(cam_h):
        for x in range(cam_w):
            pu = R.undistort_points(np.float32(x), np.float32(y), cam_K, cam_D)
            z = float(true_z[y, x])
            u, v = R.project_points((float(pu[0]) - cam_K[0, 2]) / cam_K[0, 0] * z, (float(pu[1]) - cam_K[1, 2]) / cam_K[1, 1] * z, z,
                                    rig.Rt, proj_K, proj_D)
            if 0 <= u < proj_w and 0 <= v < proj_h:
                surface[y, x] = (int(u) * proj_h + v) / (proj_w * proj_h) + 0.002 * rng.standard_normal()
            else:
                surface[y, x] = rng.random()
    surface = np.abs(surface) + 1e-3
    surface[rng.random(surface.shape) < 0.2] = 0  # pixels without an event: the fill
    surface[0, 0] = 0.4321 if lit00 else 0.0
    depth_init = (true_z * (1.0 + 0.04 * rng.standard_normal(true_z.shape))).astype(np.float32)
    depth_init[rng.random(depth_init.shape) < 0.25] = 0  # no initial depth: not optimised
    ws = window_size
    depth_init[0, :], depth_init[:, -1] = 55.5, 61.25  # > 0 inside the border: ignored
    depth_init[ws, ws], depth_init[ws + 1, ws] = 58.0, 0.0
    return {"cam_w": cam_w, "cam_h": cam_h, "proj_w": proj_w, "proj_h": proj_h, "window_size": window_size, "cam_K": cam_K, "cam_D": cam_D,
            "proj_K": proj_K, "proj_D": proj_D, "R": Rm, "T": T, "Rt": Rt, "p1_03": p1_03, "proj": proj, "surface": surface,
            "depth_init": depth_init}


def ref_rig(rig, **kw):
    """the restatement's view of a rig dict"""
    return R.Rig(rig["cam_K"], rig["cam_D"], rig["proj_K"], rig["proj_D"], rig["Rt"], rig["proj"], kw.get("p1_03", rig["p1_03"]),
                 kw.get("window_size", rig["window_size"]))


def tables(rig, **kw):
    """the dict x_maps_amd.esl_optim.EslOptim takes"""
    t = {k: rig[k] for k in ("cam_w", "cam_h", "proj_w", "proj_h", "window_size", "cam_K", "cam_D", "proj_K", "proj_D", "Rt", "p1_03")}
    t["proj_surface"] = rig["proj"]
    t.update(kw)
    return t


def load_g13(golden_dir):
    """name -> rig dict with the reference's depth_optim and nfev"""
    g = np.load(os.path.join(golden_dir, G13))
    rigs = {}
    for r in G13_RIGS:
        cam_h, cam_w = g[f"{r}_surface"].shape
        proj_w, proj_h = (int(v) for v in g[f"{r}_proj_shape"])
        rig = {k: g[f"{r}_{k}"] for k in RIG_KEYS}
        rig.update(cam_w=cam_w, cam_h=cam_h, proj_w=proj_w, proj_h=proj_h, window_size=int(g[f"{r}_window_size"]),
                   p1_03=float(g[f"{r}_p1_03"]), proj=projector_time_surface(proj_w, proj_h), depth_optim=g[f"{r}_depth_optim"],
                   nfev=g[f"{r}_nfev"])
        rigs[r] = rig
    return rigs


def group(rig, dtype, n):
    """n surfaces of a rig: its own, an all-zero one, one with a single non-zero value (hi == lo), then reseeded ones"""
    h, w = rig["cam_h"], rig["cam_w"]
    rng = np.random.default_rng(7)
    out = [rig["surface"], np.zeros((h, w)), np.where(rig["surface"] != 0, 0.375, 0.0)]
    for _ in range(max(0, n - 3)):
        s = rig["surface"] * (1.0 + 0.05 * rng.standard_normal((h, w)))
        s[rng.random((h, w)) < 0.1] = 0
        out.append(np.abs(s))
    return np.ascontiguousarray(np.stack(out[:n]).astype(dtype))
