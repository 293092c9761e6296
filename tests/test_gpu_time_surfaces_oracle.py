"""-m gpu: the time-surface entry (xm_process_time_surfaces) against its CPU oracle, O.process_time_surface, past the bounds of
the strided loops of csrc/xmaps_surface.hpp and at the value edges of the normalisation.

    camera (w x h)        nb_red  tiles_x x tiles_y  n_seg (per thread of the scan)    n_wo   crosses
    tall       65 x 2049    66       2 x 129         4098 (5; thread 819 partial)      1032   all three bounds (64 partials, 1024
                                                                                              segments, 1024 wave counters); 1-pixel
                                                                                              last tile column, 1-row last tile
    wide     2049 x 33      34      33 x 3           1089 (2; thread 544 partial)       396   the scan's bound with an odd tiles_x;
                                                                                              seg / tiles_x in the cloud kernel
    on_bound   64 x 1024    32       1 x 64          1024 (1)                           256   exactly on the scan's bound, no padding
    past_bound 64 x 1025    33       1 x 65          1025 (2)                           260   one past it
(tests/test_oracle_time_surface.py checks this table against the kernels' constants.)

One rule for every case (_check): depth has the oracle's bits; all eight statistics are equal (the doubles with ==: the same
IEEE operations, -ffp-contract=off); the cloud has the bits of the device's own point_from_disparity applied to the ORACLE's
rows -- so gather, order and compaction are the CPU's -- and agrees with the CPU's float32 transform.  Before the GPU is
touched every case asserts from the oracle alone that its surface has what the case is for."""
import ctypes as C

import numpy as np
import pytest

import time_surface_cases as K
import xmaps_oracle as O

pytestmark = pytest.mark.gpu


class Rig:
    def __init__(self, name, column0_defined=False):
        from x_maps_amd.engine import XMapsEngine
        self.name, (self.w, self.h) = name, K.CAMERAS[name]
        self.shape = (self.h, self.w)
        self.tables = K.camera_tables(name, column0_defined)
        self.engine = XMapsEngine(self.tables, camera_perspective=True)  # (a refusal of the shape by xm_create is a finding)
        self._ref = {}

    def oracle(self, key, surf):
        """the oracle's result for a named surface: computed once, shared by the tests of the module, never written to"""
        if key not in self._ref:
            self._ref[key] = O.process_time_surface(self.tables, surf)
        return self._ref[key]


@pytest.fixture(scope="module")
def rigs():
    """one engine per camera (and per X-map variant) for the module"""
    made = {}

    def get(name, column0_defined=False):
        if (name, column0_defined) not in made:
            made[name, column0_defined] = Rig(name, column0_defined)
        return made[name, column0_defined]
    yield get
    for rig in made.values():
        rig.engine.close()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


STAT_FIELDS = ("n_nonzero", "n_events", "n_inliers", "n_index_errors", "lo", "hi", "t_min", "t_max")


def _check_depth(rig, ref, depth):
    assert _same_bits(depth, ref["depth"]), f"{int((depth.view(np.uint32) != ref['depth'].view(np.uint32)).sum())} depth pixels differ"


def _check(rig, ref, got, want_cloud=True):
    depth, cloud, st = got
    _check_depth(rig, ref, depth)
    assert {f: getattr(st, f) for f in STAT_FIELDS} == ref["stats"]
    assert st.n_index_errors == 0
    if not want_cloud:
        assert cloud is None
        return
    n = int(ref["mask"].sum())
    assert cloud.shape == (n, 3) and cloud.dtype == np.float32
    Q, disp = rig.tables["Q"], ref["disp"].astype(np.float32)
    # the same device function on the oracle's rows: exact
    assert _same_bits(cloud, rig.engine.construct_point_cloud(Q, ref["xr_f32"], ref["yr_f32"], disp))
    cpu = O.construct_point_cloud(Q, ref["xr_f32"], ref["yr_f32"], disp)
    fin = np.isfinite(cpu)
    assert np.array_equal(np.isfinite(cloud), fin)
    np.testing.assert_allclose(cloud[fin], cpu[fin], rtol=1e-5, atol=1e-5)  # (tests/test_gpu_eval.py: the 4x4 transform in float32)


def _dense_conditions(rig, ref):
    st = ref["stats"]
    assert st["n_inliers"] >= 0.4 * st["n_events"]
    assert ref["y"][0] == 0 and ref["y"][-1] == rig.h - 1  # (raster order) inliers in the first and in the last camera row
    assert (ref["disp"] == 0).any()  # rows whose cloud point is not finite


def _blocks(idx):
    return sorted(set((np.asarray(idx) // K.RED_CHUNK).tolist()))


# ---- the surfaces: name -> (builder of [(key, surface)], the oracle-only check of what the case is for) -------------------------
def _c_unit(rig):
    surf = K.unit(rig.shape)
    ref = rig.oracle("unit", surf)
    _dense_conditions(rig, ref)
    assert surf.dtype == np.float64 and 0.1 <= ref["stats"]["lo"] and ref["stats"]["hi"] < 0.9
    return [("unit", surf)]


def _c_us_f32(rig):
    surf = K.us_f32(rig.shape)
    ref = rig.oracle("us_f32", surf)
    _dense_conditions(rig, ref)
    assert surf.dtype == np.float32 and ref["stats"]["lo"] >= 1e6 and np.spacing(np.float32(ref["stats"]["lo"])) >= 1 / 16
    wide = surf.astype(np.float64)
    assert np.array_equal(wide, np.rint(wide))  # integers: the cast is exact, and so is everything behind it
    return [("us_f32", surf), ("us_f32", wide)]  # the float32 file and its float64 cast: one oracle result for both


def _c_neg(rig):
    surf = K.neg(rig.shape)
    ref = rig.oracle("neg", surf)
    _dense_conditions(rig, ref)
    st = ref["stats"]
    assert st["lo"] < 0 and st["n_events"] > st["n_nonzero"] and st["n_events"] == surf.size - 1  # the zeros are events
    return [("neg", surf)]


def _c_two_values(rig):
    surf = K.two_values(rig.shape)
    ref = rig.oracle("two_values", surf)
    st = ref["stats"]
    assert np.array_equal(np.unique(surf), [0.0, 1.0, 2.0]) and st["t_min"] == st["t_max"] == 1.0
    assert st["n_inliers"] >= 0.1 * st["n_events"] > 0
    return [("two_values", surf)]


def _c_sparse(rig):
    surf = K.sparse(rig.shape)
    ref = rig.oracle("sparse", surf)
    tiles_x, n_seg = K.geometry(rig.w, rig.h)[1], K.geometry(rig.w, rig.h)[3]
    assert ref["stats"]["n_inliers"] >= 50
    assert len(set((ref["y"] * tiles_x + ref["x"] // K.TILE_W).tolist())) <= n_seg // 2  # most segments count 0
    return [("sparse", surf)]


def _c_extrema_at_ends(rig):
    out = []
    px = rig.w * rig.h
    for swapped in (False, True):
        surf = K.extrema_at_ends(rig.shape, swapped)
        ref = rig.oracle(f"extrema_at_ends{int(swapped)}", surf)
        _dense_conditions(rig, ref)
        at_lo, at_hi = np.flatnonzero(surf == ref["stats"]["lo"]), np.flatnonzero(surf == ref["stats"]["hi"])
        assert (at_lo.tolist(), at_hi.tolist()) == (([0], [px - 1]) if swapped else ([px - 1], [0]))
        assert (px - 1) // K.RED_CHUNK == K.geometry(rig.w, rig.h)[0] - 1  # the last reduction block ...
        if rig.name == "tall":
            assert (px - 1) // K.RED_CHUNK >= 64  # ... which is in the second trip of the loops over the partials
        out.append((f"extrema_at_ends{int(swapped)}", surf))
    return out


def _c_ties(rig):
    surf = K.ties(rig.shape)
    ref = rig.oracle("ties", surf)
    _dense_conditions(rig, ref)
    st, nb_red = ref["stats"], K.geometry(rig.w, rig.h)[0]
    at_lo, at_hi = np.flatnonzero(surf == st["lo"]), np.flatnonzero(surf == st["hi"])
    assert len(at_lo) == len(at_hi) == 5 and st["n_events"] == st["n_nonzero"] - 5  # every lo is dropped
    mid = (surf.size // 2) // K.RED_CHUNK
    for blocks in (_blocks(at_lo), _blocks(at_hi)):  # in the first, a middle and the last reduction block
        assert blocks[0] == 0 and blocks[-1] == nb_red - 1 and mid in blocks and 0 < mid < nb_red - 1
    assert np.signbit(surf).sum() == 4 and not ref["depth"][np.signbit(surf)].any()  # -0.0: no event
    return [("ties", surf)]


CASES = {"unit": _c_unit, "us_f32": _c_us_f32, "neg": _c_neg, "two_values": _c_two_values, "sparse": _c_sparse,
         "extrema_at_ends": _c_extrema_at_ends, "ties": _c_ties}
RUNS = [(cam, case) for cam in ("tall", "wide") for case in CASES] + \
       [(cam, case) for cam in ("on_bound", "past_bound") for case in ("unit", "us_f32", "neg")]


@pytest.mark.parametrize("camera,case", RUNS, ids=[f"{a}-{b}" for a, b in RUNS])
def test_entry_equals_the_oracle(rigs, camera, case):
    rig = rigs(camera, column0_defined=case == "two_values")  # (two_values: the degenerate column must have inliers)
    surfaces = CASES[case](rig)  # the oracle and the case's conditions, before the GPU is touched
    outs = []
    for key, surf in surfaces:
        got = rig.engine.process_time_surfaces([surf], want_cloud=True)[0]
        _check(rig, rig.oracle(key, surf), got)
        outs.append(got)
    if case == "us_f32":  # the float32 file and its exact float64 cast: identical output
        (d32, c32, s32), (d64, c64, s64) = outs
        assert _same_bits(d32, d64) and _same_bits(c32, c64) and s32 == s64


# ---- groups and scratch (tall) ------------------------------------------------------------------------------------------------
def _group_members(rig):
    """[unit, zeros, neg, two_values, sparse, one-pixel] on the default tables: non-empty members behind and in front of empty
    ones, so that an offset into the partials, the segment counts or the wave counters that is one surface off changes a result"""
    members = [("unit", K.unit(rig.shape)), ("zeros", np.zeros(rig.shape)), ("neg", K.neg(rig.shape)),
               ("two_values", K.two_values(rig.shape)), ("sparse", K.sparse(rig.shape)), ("one_pixel", K.one_pixel(rig.shape))]
    refs = [rig.oracle(k, s) for k, s in members]
    inl = [r["stats"]["n_inliers"] for r in refs]
    assert inl[0] > 1000 and inl[2] > 1000 and inl[4] >= 50 and inl[1] == inl[3] == inl[5] == 0
    # three ways to be empty: no entry, events without inliers (t_min == t_max lands in the undefined column 0), one value
    assert [r["stats"]["n_events"] for r in refs][1::2] == [0, refs[3]["stats"]["n_nonzero"] - 1, 0]
    assert [r["stats"]["n_nonzero"] for r in refs][1::2] == [0, refs[3]["stats"]["n_nonzero"], 1]
    return members, refs


def test_group_members_equal_the_oracle_and_stale_scratch_cannot_pass(rigs):
    rig = rigs("tall")
    members, refs = _group_members(rig)
    extrema = K.extrema_at_ends(rig.shape)
    ref_extrema = rig.oracle("extrema_at_ends0", extrema)
    # 1. the group of 6 with clouds
    out = rig.engine.process_time_surfaces([s for _, s in members], want_cloud=True)
    assert len(out) == 6
    for got, ref in zip(out, refs):
        _check(rig, ref, got)
    for i in (1, 3, 5):
        assert not out[i][0].any() and out[i][1].shape == (0, 3)
    # 2. a group of 1, depth only: what the larger call left in the scratch (member 0: unit) is not this surface's
    assert not np.array_equal(ref_extrema["depth"], refs[0]["depth"]) and ref_extrema["stats"] != refs[0]["stats"]
    _check(rig, ref_extrema, rig.engine.process_time_surfaces([extrema], want_cloud=False)[0], want_cloud=False)
    # 3. a group of 2 with clouds, neither member where call 1 or call 2 had it
    out = rig.engine.process_time_surfaces([members[4][1], members[2][1]], want_cloud=True)
    assert len(out) == 2
    _check(rig, refs[4], out[0])
    _check(rig, refs[2], out[1])


# ---- XM_MEM_DEVICE without clouds and statistics (wide) ---------------------------------------------------------------------------
def test_device_pointers_depth_only(rigs):
    from x_maps_amd import _native as N
    rig = rigs("wide")
    eng = rig.engine
    members = [("neg", K.neg(rig.shape)), ("unit", K.unit(rig.shape))]
    refs = [rig.oracle(k, s) for k, s in members]
    assert all(r["stats"]["n_inliers"] > 1000 for r in refs)
    grp = np.stack([s for _, s in members])
    n, px = len(grp), rig.w * rig.h
    d_in = eng.to_device(grp)
    d_depth = eng.dev_alloc(n * px * 4)
    try:
        N.check(eng._lib.xm_process_time_surfaces(eng._h, C.c_void_p(d_in), N.XM_T_FLOAT64, n, N.XM_MEM_DEVICE, C.c_void_p(d_depth),
                                                  None, None))
        eng.sync()
        depth = np.empty((n,) + rig.shape, np.float32)
        eng.dev_download(depth, d_depth)
    finally:
        eng.dev_free(d_in)
        eng.dev_free(d_depth)
    for i, ref in enumerate(refs):
        _check_depth(rig, ref, depth[i])
