"""GPU: the rig-map kernels (csrc/xmaps_rigmaps.hpp; x_maps_amd/rig_maps.py) against x_maps_amd/calibration.py's NumPy, bit for
bit, on the small rigs of tests/rig_maps_cases.py (tests/test_rig_maps_cases_cpu.py shows which edges they reach), and the
maps_on_device switch of the three table builders against the same call without it."""
import ctypes as C

import numpy as np
import pytest

import rig_maps_cases as RC
from x_maps_amd import _native as N
from x_maps_amd import calibration as cal
from x_maps_amd import esl_init, mc3d, rig_maps

pytestmark = pytest.mark.gpu


def _same_array(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == np.float32:
        return RC.bits_equal(a, b)
    return bool(np.array_equal(a, b))


def _same_dict(got: dict, want: dict):
    assert set(got) == set(want), set(got) ^ set(want)
    for k, w in want.items():
        g = got[k]
        if isinstance(w, tuple):
            assert isinstance(g, tuple) and len(g) == len(w) and all(_same_array(x, y) for x, y in zip(g, w)), k
        elif isinstance(w, np.ndarray):
            assert isinstance(g, np.ndarray) and _same_array(g, w), (k, g.dtype, w.dtype, g.shape, w.shape)
        else:
            assert type(g) is type(w) and g == w, (k, g, w)


def _linear_time(cp, scan_upwards):
    return (cp.projector_width, cp.projector_height, scan_upwards)


# ---- the forward map -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1], ids=["camera", "projector-D0"])
@pytest.mark.parametrize("rig", ["S", "S2", "L"])
def test_forward_map_is_numpys(rig, which):
    v = RC.forward_views(rig)[which]
    want = RC.forward_expected(rig, which)
    r = rig_maps.forward_map(*v.args, v.rect_size, want_pair=True)
    assert RC.bits_equal(r["mapx"], want[0]) and RC.bits_equal(r["mapy"], want[1])
    assert r["pair_i16"].dtype == np.int16 and np.array_equal(r["pair_i16"], esl_init._pair_i16(*want))
    mx, my = rig_maps.init_undistort_rectify_map(*v.args, v.rect_size)
    assert RC.bits_equal(mx, want[0]) and RC.bits_equal(my, want[1])


# ---- the inverse map -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1], ids=["camera", "projector"])
@pytest.mark.parametrize("rig", ["S", "S2", "L", "T"])
def test_inverse_map_is_numpys(rig, which):
    v = RC.views(rig)[which]
    want = RC.inverse_expected(rig, which)
    r = rig_maps.inverse_map(*v.args, v.size, want_i16=True, want_pair=True)
    assert RC.bits_equal(r["mapx"], want[0]) and RC.bits_equal(r["mapy"], want[1])
    ix, iy = cal.mapf_to_i16(want[0]), cal.mapf_to_i16(want[1])
    assert r["mapx_i16"].dtype == np.int16 and np.array_equal(r["mapx_i16"], ix) and np.array_equal(r["mapy_i16"], iy)
    assert np.array_equal(r["pair_i16"], np.stack((ix, iy), -1))
    mx, my = rig_maps.init_undistort_rectify_map_inverse(*v.args, v.size)
    assert RC.bits_equal(mx, want[0]) and RC.bits_equal(my, want[1])


def test_inverse_map_outside_int16_is_an_error_that_names_the_map():
    bad, good = RC.out_of_i16_view(), RC.views("S2")[1]
    with pytest.raises(ValueError, match=r"mapx has entries outside int16"):
        rig_maps.inverse_map(*bad.args, bad.size, want_i16=True)
    with pytest.raises(ValueError, match=r"mapx has entries outside int16"):
        rig_maps.inverse_map(*bad.args, bad.size, want_maps=False, want_pair=True)
    mx, _ = rig_maps.init_undistort_rectify_map_inverse(*bad.args, bad.size)  # the float maps alone: nothing to refuse
    assert float(mx.min()) > 32767.0
    r = rig_maps.inverse_map(*good.args, good.size, want_i16=True)  # the flag does not outlive the call
    assert np.array_equal(r["mapx_i16"], cal.mapf_to_i16(RC.inverse_expected("S2", 1)[0]))


# ---- the remap ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scan_upwards", [False, True], ids=["down", "up"])
@pytest.mark.parametrize("rig", ["S", "S2", "L"])
def test_linear_time_map_is_remapped_in_place(rig, scan_upwards):
    cp, border = RC.params(rig), RC.TABLE_KW[rig]["time_map_border"]
    v = RC.forward_views(rig)[1]
    mx, my = RC.forward_expected(rig, 1)
    tm = cal.generate_linear_projector_time_map(cp.projector_width, cp.projector_height, scan_upwards)
    want = cal.remap_nearest(tm, mx, my, border)
    r = rig_maps.forward_map(*v.args, v.rect_size, want_maps=False, linear_time=_linear_time(cp, scan_upwards), border=border)
    assert set(r) == {"remap", "kernel_ms"} and RC.bits_equal(r["remap"], want)
    assert 0 < int((want != 0).sum()) < want.size  # (a remap that is all border, or has none, shows nothing)
    if not scan_upwards:  # esl_init's projector time surface is the same expression
        ts = esl_init.get_projector_time_surface(cp.projector_width, cp.projector_height)
        assert RC.bits_equal(r["remap"], cal.remap_nearest(ts, mx, my, border))


@pytest.mark.parametrize("which", [0, 1], ids=["camera", "projector-D0"])
@pytest.mark.parametrize("rig", ["S", "S2", "L"])
def test_image_in_device_memory_is_remapped_and_host_and_device_outputs_agree(rig, which):
    import torch
    border = RC.TABLE_KW[rig]["time_map_border"]
    v = RC.forward_views(rig)[which]
    w, h = v.rect_size
    sw, sh = v.size
    img = np.random.default_rng(7 + which).standard_normal((sh, sw)).astype(np.float32)
    mx, my = RC.forward_expected(rig, which)
    want = cal.remap_nearest(img, mx, my, border, 0.0)
    host = rig_maps.forward_map(*v.args, v.rect_size, want_pair=True, src=img, border=border)
    assert RC.bits_equal(host["remap"], want)
    dev = torch.device("cuda", 0)
    d_img = torch.from_numpy(img).to(dev)
    d_mx, d_my, d_re = (torch.full((h, w), 7.0, dtype=torch.float32, device=dev) for _ in range(3))
    d_pair = torch.full((h, w, 2), 7, dtype=torch.int16, device=dev)
    cfg = rig_maps.forward_config(*v.args, v.rect_size, src=d_img.data_ptr(), src_size=(sw, sh), border=border, border_value=0.0)
    out = N.xm_rig_forward_outputs(d_mx.data_ptr(), d_my.data_ptr(), d_pair.data_ptr(), d_re.data_ptr())
    N.check(N.load_library().xm_rig_forward_map(0, C.byref(cfg), C.byref(out), N.XM_MEM_DEVICE))
    assert out.kernel_ms > 0
    assert RC.bits_equal(d_re.cpu().numpy(), want)
    assert RC.bits_equal(d_mx.cpu().numpy(), host["mapx"]) and RC.bits_equal(d_my.cpu().numpy(), host["mapy"])
    assert np.array_equal(d_pair.cpu().numpy(), host["pair_i16"])
    # calibration.remap_nearest's own arguments: a caller's maps are read instead of computed
    assert RC.bits_equal(rig_maps.remap_nearest(img, mx, my, border, 0.0), want)
    if border == "constant":
        assert RC.bits_equal(rig_maps.remap_nearest(img, mx, my, "constant", -2.5), cal.remap_nearest(img, mx, my, "constant", -2.5))


@pytest.mark.parametrize("rig", ["S2", "T"])
def test_inverse_map_host_and_device_outputs_agree(rig):
    import torch
    v = RC.views(rig)[1]
    w, h = v.size
    host = rig_maps.inverse_map(*v.args, v.size, want_i16=True, want_pair=True)
    dev = torch.device("cuda", 0)
    d_mx, d_my = (torch.full((h, w), 7.0, dtype=torch.float32, device=dev) for _ in range(2))
    d_ix, d_iy = (torch.full((h, w), 7, dtype=torch.int16, device=dev) for _ in range(2))
    d_pair = torch.full((h, w, 2), 7, dtype=torch.int16, device=dev)
    cfg = rig_maps.inverse_config(*v.args, v.size)
    out = N.xm_rig_inverse_outputs(d_mx.data_ptr(), d_my.data_ptr(), d_ix.data_ptr(), d_iy.data_ptr(), d_pair.data_ptr())
    N.check(N.load_library().xm_rig_inverse_map(0, C.byref(cfg), C.byref(out), N.XM_MEM_DEVICE))
    assert RC.bits_equal(d_mx.cpu().numpy(), host["mapx"]) and RC.bits_equal(d_my.cpu().numpy(), host["mapy"])
    assert np.array_equal(d_ix.cpu().numpy(), host["mapx_i16"]) and np.array_equal(d_iy.cpu().numpy(), host["mapy_i16"])
    assert np.array_equal(d_pair.cpu().numpy(), host["pair_i16"])


def test_bad_arguments_are_refused_before_any_gpu_work():
    lib = N.load_library()
    v = RC.views("T")[0]
    cfg = rig_maps.inverse_config(*v.args, v.size)
    assert lib.xm_rig_inverse_map(0, C.byref(cfg), C.byref(N.xm_rig_inverse_outputs()), N.XM_MEM_HOST) == N.XM_ERR_INVALID  # no output
    cfg.struct_size -= 8
    buf = np.empty((v.size[1], v.size[0]), np.float32)
    out = N.xm_rig_inverse_outputs(buf.ctypes.data)
    assert lib.xm_rig_inverse_map(0, C.byref(cfg), C.byref(out), N.XM_MEM_HOST) == N.XM_ERR_INVALID
    fcfg = rig_maps.forward_config(*v.args, v.rect_size)  # a remap without a source
    fout = N.xm_rig_forward_outputs(None, None, None, buf.ctypes.data)
    assert lib.xm_rig_forward_map(0, C.byref(fcfg), C.byref(fout), N.XM_MEM_HOST) == N.XM_ERR_INVALID
    with pytest.raises(ValueError):
        rig_maps.forward_map(*v.args, v.rect_size, border="reflect")


# ---- the table builders' switch ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def l_tables():
    """build_tables on L as the pipe calls it, without and with the switch (shared: read-only)"""
    cp = RC.params("L")
    return cp, cal.build_tables(cp), cal.build_tables(cp, maps_on_device=True)


def test_build_tables_on_the_live_rig(l_tables):
    cp, want, got = l_tables
    _same_dict(got, want)
    assert got["proj_x_map"].dtype == np.int16 and got["time_map_rect"].dtype == np.float32 and got["cam_mapx_f32"].dtype == np.float32
    assert int((got["proj_x_map"] != 0).sum()) > 0
    N.debug_option("XM_XMAP_SCAN", "1")
    scan = cal.build_tables(cp, maps_on_device=True)
    N.debug_option("XM_XMAP_SCAN", None)
    assert np.array_equal(scan["proj_x_map"], want["proj_x_map"])


@pytest.mark.parametrize("rig,builder", [("S", "build_eval_tables"), ("S", "build_tables"), ("L", "build_eval_tables")])
def test_build_tables_with_the_switch_equal_those_without(rig, builder):
    cp, fn = RC.params(rig), getattr(cal, builder)
    want, got = fn(cp, z_near=0.2, z_far=1.1), fn(cp, z_near=0.2, z_far=1.1, maps_on_device=True)
    _same_dict(got, want)
    assert 0 < int((got["time_map_rect"] != 0).sum())
    N.debug_option("XM_XMAP_SCAN", "1")
    scan = fn(cp, maps_on_device=True)
    N.debug_option("XM_XMAP_SCAN", None)
    assert np.array_equal(scan["proj_x_map"], want["proj_x_map"])


def test_build_tables_takes_a_callers_rectified_time_map_and_refuses_x_map_fn(l_tables):
    cp, want, _ = l_tables
    tm = np.ascontiguousarray(want["time_map_rect"][::-1] * np.float32(0.5))
    _same_dict(cal.build_tables(cp, projector_time_map_rectified=tm, maps_on_device=True),
               cal.build_tables(cp, projector_time_map_rectified=tm))
    with pytest.raises(ValueError, match="x_map_fn"):
        cal.build_tables(cp, x_map_fn=lambda *a: None, maps_on_device=True)


def test_esl_init_and_mc3d_tables_with_the_switch_equal_those_without():
    cp = RC.params("S")
    with np.errstate(all="ignore"):
        want_e, want_m = esl_init.build_esl_init_tables(cp), mc3d.build_mc3d_tables(cp)
    _same_dict(esl_init.build_esl_init_tables(cp, maps_on_device=True), want_e)
    _same_dict(mc3d.build_mc3d_tables(cp, maps_on_device=True), want_m)
    assert int((want_e["cam_to_rect_map"] == 32767).sum() + (want_e["cam_to_rect_map"] == -32768).sum()) > 0
    assert 0 < int((want_e["proj_rect"] != 0).sum()) < want_e["proj_rect"].size
    rs = (cp.rect_image_width, cp.rect_image_height)
    _same_dict(mc3d.build_mc3d_tables(cp, rectify_size=rs, maps_on_device=True), mc3d.build_mc3d_tables(cp, rectify_size=rs))


def test_engine_on_device_built_tables_produces_the_same_frame(l_tables):
    from x_maps_amd import XMapsEngine, rig
    cp, want, got = l_tables
    evs, _ = rig.render_events(cp, want, row_stride=3)
    assert len(evs) > 1000
    frames = []
    for tb in (want, got):
        with XMapsEngine(tb) as eng:
            depth, bgr, st = eng.process_events(evs, raise_on_index_error=False)
        frames.append((depth, bgr, st.n_inliers))
    assert frames[0][2] == frames[1][2] > 0
    assert np.array_equal(frames[0][0], frames[1][0]) and np.array_equal(frames[0][1], frames[1][1])
    assert int((frames[1][0] > 0).sum()) > 0
