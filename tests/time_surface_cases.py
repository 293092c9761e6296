"""Cameras and surfaces of the time-surface tests (helpers, no tests): the shapes at which the strided loops of
csrc/xmaps_surface.hpp take a second trip, and the value edges of the normalisation.  Everything is seeded."""
import numpy as np

from x_maps_amd.synthetic import RigConfig, make_tables

Q_G7 = np.array([[1, 0, 0, -80.5], [0, 1, 0, -60.25], [0, 0, 0, 540.0], [0, 0, -7.75, 0]], dtype=np.float64)

# the launch geometry of xm_process_time_surfaces (csrc/host/xm_api_surface.hpp); tests/test_oracle_time_surface.py checks these
# against the constants in csrc/xmaps_surface.hpp
RED_CHUNK, TILE_W, TILE_ROWS, WAVES_PER_BLOCK, SCAN_BLOCK = 2048, 64, 16, 4, 1024

# name -> (cam_w, cam_h): what each crosses is in the table of tests/test_gpu_time_surfaces_oracle.py
CAMERAS = {"tall": (65, 2049), "wide": (2049, 33), "on_bound": (64, 1024), "past_bound": (64, 1025)}


def geometry(cam_w, cam_h):
    """(nb_red, tiles_x, tiles_y, n_seg, ipt, n_wo) of a camera"""
    tiles_x, tiles_y = -(-cam_w // TILE_W), -(-cam_h // TILE_ROWS)
    n_seg = cam_h * tiles_x
    return -(-cam_w * cam_h // RED_CHUNK), tiles_x, tiles_y, n_seg, -(-n_seg // SCAN_BLOCK), tiles_x * tiles_y * WAVES_PER_BLOCK


def with_cloud_tables(tb, seed):
    """float rectify maps as tests/golden/make_golden.py builds them (the i16 LUT + uniform(-0.45, 0.45)) and a Q like G7's"""
    rng = np.random.default_rng(seed)
    tb = dict(tb)
    tb["cam_mapx_f32"] = (tb["cam_mapx_i16"] + rng.uniform(-0.45, 0.45, tb["cam_mapx_i16"].shape)).astype(np.float32)
    tb["cam_mapy_f32"] = (tb["cam_mapy_i16"] + rng.uniform(-0.45, 0.45, tb["cam_mapy_i16"].shape)).astype(np.float32)
    tb["Q"] = Q_G7.copy()
    return tb


def camera_tables(name, column0_defined=False):
    """The synthetic rig at one of CAMERAS (projector 64 x 48: camera view ignores its map), the rectified rows clipped into the
    X-map's defined band so that the first and the last camera row have inliers.  column0_defined: X-map column 0 -- where
    every event of a surface with t_min == t_max lands -- is a copy of column 1 instead of undefined."""
    w, h = CAMERAS[name]
    cfg = RigConfig("C-" + name, w, h, 64, 48, 0)
    tb = make_tables(cfg)
    tb["cam_mapy_i16"] = np.clip(tb["cam_mapy_i16"], 8, cfg.rect_h - 8).astype(np.int16)
    if column0_defined:
        tb["proj_x_map"] = tb["proj_x_map"].copy()
        tb["proj_x_map"][:, 0] = tb["proj_x_map"][:, 1]
    return with_cloud_tables(tb, 11)


def _filled(rng, values, fill):
    values[rng.random(values.shape) >= fill] = 0
    return values


def unit(shape, seed=1):
    rng = np.random.default_rng(seed)
    return _filled(rng, rng.random(shape) * 0.8 + 0.1, 0.7)


def us_f32(shape, seed=1):
    """raw microsecond stamps in a float32 file: the f32 ulp is 1/16 at 1e6, the integers are exact"""
    rng = np.random.default_rng(seed)
    return _filled(rng, (1e6 + rng.integers(0, 13000, shape)).astype(np.float32), 0.7)


def neg(shape, seed=1):
    """lo < 0: the zeros that are kept normalise above 0 and are events"""
    rng = np.random.default_rng(seed)
    return _filled(rng, rng.random(shape) * 0.8 - 0.4, 0.7)


def two_values(shape):
    """2.0 on a lattice, 1.0 in one pixel: normalisable, every event has t == 1"""
    ys, xs = np.mgrid[0:shape[0], 0:shape[1]]
    s = np.where((xs + ys) % 3 == 0, 2.0, 0.0)
    s[shape[0] // 2, shape[1] // 2] = 1.0
    return s


def sparse(shape, seed=1):
    rng = np.random.default_rng(seed)
    return _filled(rng, rng.random(shape) * 0.8 + 0.1, 0.002)


def one_pixel(shape):
    s = np.zeros(shape)
    s[shape[0] // 3, shape[1] // 2] = 0.3
    return s


LO, HI = 0.05, 0.95  # outside unit()'s [0.1, 0.9)


def extrema_at_ends(shape, swapped=False, seed=1):
    """unit() with lo only in the last pixel (the tail of the last reduction block) and hi only in the first, or swapped"""
    s = unit(shape, seed)
    s.flat[-1], s.flat[0] = (HI, LO) if swapped else (LO, HI)
    return s


def ties(shape, seed=1):
    """extrema_at_ends() with five pixels equal to lo (all dropped) and five equal to hi, in the first, a middle and the last
    reduction block, and a few -0.0 entries (no event)"""
    s = extrema_at_ends(shape, False, seed)
    px = s.size
    s.flat[[5, 1000, px // 2, px - 300]] = LO
    s.flat[[7, px // 2 + 1, px - 500, px - 2]] = HI
    s.flat[[2, px // 3, px // 2 + 9, px - 3]] = -0.0
    return s
