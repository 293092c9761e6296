"""No GPU: the NumPy oracle of the frame -> time surface entry (tests/frame_surface_cases.py) against a plain per-event loop on
every frame of the group, and every frame against what it claims to exercise -- so that a GPU test that passes on these frames
has met duplicates, left-out events, a base held by a left-out / a negative event, and float32 conversions that round."""
import numpy as np
import pytest

import frame_surface_cases as K
from x_maps_amd import synthetic as S

SIZES = [(K.CAM_W, K.CAM_H), (S.C_TINY.cam_w, S.C_TINY.cam_h)]


@pytest.mark.parametrize("cam", SIZES, ids=lambda c: f"{c[0]}x{c[1]}")
@pytest.mark.parametrize("use_polarity", [False, True])
@pytest.mark.parametrize("select", K.SELECTS)
def test_the_oracle_equals_the_event_loop(cam, select, use_polarity):
    names, frames = K.group(*cam)
    for name, evs in zip(names, frames):
        for dtype in (np.float32, np.float64):
            a, sa = K.oracle(evs, *cam, select, dtype, use_polarity)
            b, sb = K.oracle_loop(evs, *cam, select, dtype, use_polarity)
            assert a.dtype == b.dtype == dtype and a.shape == (cam[1], cam[0])
            assert np.array_equal(a, b) and sa == sb, (name, dtype)


@pytest.mark.parametrize("cam", SIZES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_every_frame_reaches_what_it_is_for(cam):
    w, h = cam
    f = K.frames(w, h)
    assert list(f)[-3:] == ["wide_span", "empty_between", "after_empty"] and len(f["wide_span"]) > 1000 and len(f["after_empty"]) > 1000
    assert len(f["empty"]) == len(f["empty_between"]) == 0 and len(f["single"]) == 1
    assert w * h % 64 != 0 or (w, h) != (K.CAM_W, K.CAM_H)
    if (w, h) == (K.CAM_W, K.CAM_H):
        assert w * h == 2590 and w * h % 1024 != 0 and w * h > 1024

    def st(name, select="last", dtype=np.float64, pol=False):
        return K.oracle(f[name], w, h, select, dtype, pol)

    # long: 5 000 events, several per cell -- "last" and "first" differ
    assert len(f["long"]) == 5000 and st("long")[1]["n_pixels"] < 5000
    assert not np.array_equal(st("long")[0], st("long", "first")[0])
    # one pixel
    s, d = st("one_pixel")
    assert d["n_pixels"] == 1 and d["n_events"] == 700 and s[2, 3] == d["t_span"] + 1
    assert st("one_pixel", "first")[0][2, 3] == 1
    # about 60 % duplicates
    d = st("duplicates")[1]
    assert 0.55 <= 1 - d["n_pixels"] / d["n_events"] <= 0.65, d
    # shuffled: the earliest event is not the first, stamps are out of order, and index order != time order at some pixel
    ev = f["shuffled"]
    assert int(np.argmin(ev["t"])) == 777 and (np.diff(ev["t"]) < 0).sum() > 500
    by_time = K.oracle(np.sort(ev, order="t", kind="stable"), w, h)[0]
    assert not np.array_equal(by_time, st("shuffled")[0])
    assert st("shuffled")[1]["t_base"] == 2_999_990 and st("shuffled")[0].min() == 0
    # equal t: every hit pixel holds 1
    s, d = st("equal_t")
    assert d["t_span"] == 0 and set(np.unique(s).tolist()) == {0.0, 1.0}
    # outside: five events left out, one of which holds the minimum
    ev = f["outside"]
    s, d = st("outside")
    assert d["n_index_errors"] == 5 and d["t_base"] == 5_999_000 == int(ev["t"][1]) and ev["x"][1] == w
    assert (ev["y"] == h).sum() == 1 and (ev["x"] == 65535).sum() == 2 and (ev["y"] == 65535).sum() == 2
    assert s[s > 0].min() > 1000  # (nobody inside the sensor fired at the base)
    # polarity: a negative event holds the smallest t
    ev = f["polarity"]
    assert 0.2 < (ev["p"] == 0).mean() < 0.4 and ev["p"][0] == 0
    assert st("polarity")[1]["t_base"] == 7_990_000 != st("polarity", pol=True)[1]["t_base"]
    assert st("polarity")[1]["n_events"] == 1300 > st("polarity", pol=True)[1]["n_events"]
    assert not np.array_equal(st("polarity")[0], st("polarity", pol=True)[0])
    # wide span: float32 rounds down, up, and ties both ways; float64 is exact
    for select in K.SELECTS:
        s64, d = st("wide_span", select)
        s32 = st("wide_span", select, np.float32)[0]
        assert d["t_span"] >= 1 << 24 and d["t_base"] == 9_000_000
        want = [(1 << 24) + 1, (1 << 24) + 3, (1 << 24) + 2, (1 << 24) + 6, (1 << 25) + 2, (1 << 25) + 6, (1 << 26) + 12345, (1 << 26) + 12351]
        assert s64[0, :8].astype(np.int64).tolist() == want
        got = s32[0, :8].astype(np.int64).tolist()
        assert got == [1 << 24, (1 << 24) + 4, (1 << 24) + 2, (1 << 24) + 6, 1 << 25, (1 << 25) + 8, (1 << 26) + 12344, (1 << 26) + 12352]
        assert sum(g < v for g, v in zip(got, want)) == 3 and sum(g > v for g, v in zip(got, want)) == 3
        assert (s64 % 2 == 1).sum() > 100  # odd values throughout


def test_the_entry_points_are_declared():
    """header, bindings (what tests/test_cabi_symbols.py compares with the library) and the Python layers name the new entries"""
    import os

    from x_maps_amd import _native as N
    from x_maps_amd.depth_reprojection_processor import RuntimeParams
    from x_maps_amd.engine import XMapsEngine
    from x_maps_amd.ingest import DeviceIngest
    header = open(os.path.join(N.ROOT, "include", "xmaps.h")).read()
    for name in ("xm_frames_to_time_surfaces", "xm_ingest_set_surface_output", "xm_ingest_copy_surface"):
        assert name in N.SYMBOLS and f"int {name}(" in header
    assert (N.XM_SURFACE_LAST, N.XM_SURFACE_FIRST) == (1, 2) and "#define XM_API_VERSION 5" in header
    assert hasattr(XMapsEngine, "frames_to_time_surfaces") and hasattr(DeviceIngest, "surface") and hasattr(DeviceIngest, "set_surface_output")
    assert "surface_callback" in RuntimeParams.__dataclass_fields__
