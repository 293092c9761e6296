"""CPU: the rigs of tests/rig_maps_cases.py reach the edges the GPU tests of the rig-map kernels rely on (values beyond int16 and
beyond 2^24, exact .5 ties that round both ways, a border that is really taken, a map mapf_to_i16 refuses), and the elementwise
restatement of undistort_points the kernels follow equals calibration.py's in every float32 bit."""
import numpy as np
import pytest

import rig_maps_cases as RC
from x_maps_amd import calibration as C
from x_maps_amd import esl_init


def _beyond_i16(m):
    m = np.asarray(m, np.float64)
    return ~np.isfinite(m) | (np.abs(np.where(np.isfinite(m), m, 0.0)) > 32767.0)


def _fwd(rig, which):
    return np.stack(RC.forward_expected(rig, which))


def _time_map_rect(rig):
    cp, kw = RC.params(rig), RC.TABLE_KW[rig]
    tm = C.generate_linear_projector_time_map(cp.projector_width, cp.projector_height, kw["scan_upwards"])
    fwd = RC.forward_views(rig)[1] if kw["zero_undistort_proj_map"] else RC.views(rig)[1]
    mx, my = C.init_undistort_rectify_map(*fwd.args, fwd.rect_size)
    return C.remap_nearest(tm, mx, my, kw["time_map_border"]), mx, my


def test_shapes_leave_every_tile_and_block():
    for rig in ("S", "S2", "L", "T"):
        for v in RC.views(rig):
            for w, h in (v.size, v.rect_size):
                assert w % 64 and h % 64 and w * h > 256, (v.name, w, h)
    assert RC.views("S")[0].rect_size == (405, 720) and RC.views("L")[0].rect_size == (220, 165)


def test_rig_s_saturates_and_takes_the_border():
    cam = _fwd("S", 0)
    assert int(_beyond_i16(cam).sum()) >= 1             # esl_init._pair_i16 has something to saturate
    pair = esl_init._pair_i16(*RC.forward_expected("S", 0))
    assert (pair == 32767).any() or (pair == -32768).any()
    tm, _, _ = _time_map_rect("S")
    assert 0.90 < float((tm == 0).mean()) < 0.99        # mostly border, not only border
    assert int(RC.ties(np.stack(RC.inverse_expected("S", 1))).sum()) >= 1


def test_rig_s2_reaches_far_beyond_every_image():
    cam = _fwd("S2", 0)
    assert np.isfinite(cam).all()
    a = np.abs(cam.astype(np.float64))
    assert int(_beyond_i16(cam).sum()) >= 1 and int((a > 2.0 ** 24).sum()) >= 1 and float(a.max()) < 2.0 ** 31
    assert int(RC.ties(cam).sum()) >= 1
    for which in (0, 1):  # both inverse maps still fit int16
        for m in RC.inverse_expected("S2", which):
            C.mapf_to_i16(m)


def test_rig_l_replicates_on_every_side():
    _, mx, my = _time_map_rect("L")
    cp = RC.params("L")
    ix, iy = np.rint(mx), np.rint(my)
    assert (ix < 0).any() or (iy < 0).any()
    assert (ix > cp.projector_width - 1).any() or (iy > cp.projector_height - 1).any()
    inside = (ix >= 0) & (ix < cp.projector_width) & (iy >= 0) & (iy < cp.projector_height)
    assert inside.any() and not inside.all()


def test_rig_t_is_all_ties_and_rounds_both_ways():
    for m in RC.inverse_expected("T", 0):
        assert RC.ties(m).all()
        d = np.rint(m) - m
        assert (d == 0.5).any() and (d == -0.5).any()   # half to even: up to one even neighbour, down to the other
        assert (np.rint(m).astype(np.int64) % 2 == 0).all()


def test_shifted_projector_map_leaves_int16():
    v = RC.out_of_i16_view()
    mx, my = C.init_undistort_rectify_map_inverse(*v.args, v.size)
    with pytest.raises(AssertionError):
        C.mapf_to_i16(mx)
    C.mapf_to_i16(my)  # (only the x map: the error has one map to name)


@pytest.mark.parametrize("rig", ["S", "S2", "full"])
def test_elementwise_undistort_points_is_calibrations(rig):
    for v in RC.views(rig):
        want = C.init_undistort_rectify_map_inverse(*v.args, v.size)
        got = RC.undistort_points_elementwise(*v.args, v.size)
        for a, b in zip(got, want):
            assert a.dtype == np.float32 and np.array_equal(a.view(np.int32), b.view(np.int32)), v.name
    if rig == "full":  # the inputs that decide rint: the full-size rig has them in both inverse maps
        for which in (0, 1):
            assert int(RC.ties(np.stack(RC.inverse_expected("full", which))).sum()) >= 1
