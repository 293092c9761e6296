"""No GPU: the oracle of the frame -> point cloud entry (tests/frame_cloud_cases.py, a composition of oracle.xmaps_oracle functions)
against a plain per-event loop on every frame of the group, and every frame against what it claims to exercise -- so that a GPU
test that passes on these frames has met left-out events that hold the extrema, exact column ties, disparity-0 rows, duplicates
and the wave and chunk boundaries of the kernels."""
import functools
import os
from fractions import Fraction

import numpy as np
import pytest

import frame_cloud_cases as K


@functools.lru_cache(maxsize=None)
def _tb():
    return K.rig_tables()


@functools.lru_cache(maxsize=None)
def _frames():
    return K.frames(_tb())


@pytest.mark.parametrize("use_polarity", [False, True])
def test_the_oracle_equals_the_event_loop(use_polarity):
    tb = _tb()
    for name, evs in _frames().items():
        o = K.oracle(tb, evs, use_polarity)
        rows, stats = K.oracle_loop(tb, evs, use_polarity)
        assert o["stats"] == stats, name
        assert o["cloud"].shape == (len(rows), 3) and o["cloud"].dtype == np.float32, name
        assert [(float(a), float(b), int(d)) for a, b, d in zip(o["xr_f"], o["yr_f"], o["disp"])] == rows, name


def test_every_frame_reaches_what_it_is_for():
    tb, f = _tb(), _frames()
    w, h, S_ = tb["cam_w"], tb["cam_h"], tb["t_px_scale"]
    st = {k: K.oracle(tb, v) for k, v in f.items()}
    assert len(f["empty"]) == len(f["empty_between"]) == 0 and len(f["single"]) == 1
    assert st["empty"]["stats"] == dict.fromkeys(K.STAT_FIELDS, 0) and st["empty"]["cloud"].shape == (0, 3)
    # wave and chunk boundaries really straddled
    assert [len(f[f"n{n}"]) for n in (63, 64, 65, 1023, 1024, 1025)] == [K.WAVE - 1, K.WAVE, K.WAVE + 1, K.CHUNK - 1, K.CHUNK, K.CHUNK + 1]
    assert len(f["long"]) > 2 * K.CHUNK and -(-len(f["long"]) // K.CHUNK) == 4  # two trips of two blocks under XM_FC_MAX_BLOCKS=2
    for k in ("n65", "n1025", "long"):  # inliers on both sides of the boundary
        m = np.zeros(len(f[k]), bool)
        m[np.flatnonzero(st[k]["on"])[st[k]["mask"]]] = True
        b = K.WAVE if k == "n65" else K.CHUNK
        assert m[:b].any() and m[b:].any(), k
    # the dense frames
    for k in K.DENSE:
        share = st[k]["stats"]["n_inliers"] / st[k]["stats"]["n_events"]
        assert 0.3 <= share <= 0.9, (k, share)
    assert st["no_inlier"]["stats"]["n_inliers"] == 0 and st["no_inlier"]["stats"]["n_events"] >= 100
    # (the one event that holds t_min lies in the X-map's undefined column 0: frame_cloud_cases._select)
    a = st["all_inlier"]
    assert a["stats"]["n_inliers"] == a["stats"]["n_events"] - 1 >= 256 and not a["mask"][0] and a["mask"][1:].all()
    assert (f["all_inlier"]["t"][1:] > a["stats"]["t_min"]).all() and a["stats"]["n_index_errors"] == 0
    # outside: five events left out, the first and the last of the frame among them, and they hold the extrema
    ev, s = f["outside"], st["outside"]["stats"]
    assert s["n_index_errors"] == 5 and ev["x"][0] >= w and ev["x"][-1] >= w
    assert s["t_min"] == int(ev["t"][0]) < int(ev["t"][1:-1].min()) + 1 and s["t_max"] == int(ev["t"][-1])
    on = ev[(ev["x"] < w) & (ev["y"] < h)]
    assert (int(on["t"].min()), int(on["t"].max())) != (s["t_min"], s["t_max"])  # (the extrema are NOT those of the events that take part)
    # polarity: a negative event holds the smallest t
    ev = f["polarity"]
    a, b = st["polarity"], K.oracle(tb, ev, True)
    assert 0.2 < (ev["p"] == 0).mean() < 0.4 and ev["p"][0] == 0
    assert a["stats"]["t_min"] == 7_990_000 != b["stats"]["t_min"] and a["stats"]["n_events"] == 1300 > b["stats"]["n_events"]
    assert a["stats"]["n_inliers"] != b["stats"]["n_inliers"]
    # shuffled: the earliest event is not the first, and the rows are in stream order, not in time order
    ev = f["shuffled"]
    assert int(np.argmin(ev["t"])) == 777 and (np.diff(ev["t"]) < 0).sum() > 500
    by_time = K.oracle(tb, np.sort(ev, order="t", kind="stable"))
    assert by_time["stats"] == st["shuffled"]["stats"] and not np.array_equal(by_time["cloud"], st["shuffled"]["cloud"], equal_nan=True)
    # equal t: column 0 for everybody, which is undefined in the X-map -- no rows, where the same pixels with a span have some
    assert st["equal_t"]["stats"]["t_min"] == st["equal_t"]["stats"]["t_max"] and st["equal_t"]["stats"]["n_events"] == 900
    assert st["equal_t"]["stats"]["n_inliers"] == 0
    spread = f["equal_t"].copy()
    spread["t"] += np.arange(900)
    assert K.oracle(tb, spread)["stats"]["n_inliers"] > 300
    # exact .5 ties
    ev, s = f["tie"], st["tie"]["stats"]
    ties = [Fraction(int(t) - s["t_min"], s["t_max"] - s["t_min"]) * S_ for t in ev["t"]]
    assert sum(q.denominator == 2 for q in ties) >= 200
    # disparity 0
    assert (st["disp0"]["disp"] == 0).sum() >= 1
    assert not np.isfinite(st["disp0"]["cloud"]).all()
    # heavy duplicates of one pixel
    ev = f["one_pixel"]
    assert len(set(zip(ev["x"].tolist(), ev["y"].tolist()))) == 1 and st["one_pixel"]["stats"]["n_inliers"] > 1
    # 33 frames with empties in between
    order = K.group33(tb)
    assert len(order) == 33


def test_the_entry_points_are_declared():
    """header, bindings (what tests/test_cabi_symbols.py compares with the library) and the Python layers name the new entries"""
    from x_maps_amd import _native as N
    from x_maps_amd.depth_reprojection_processor import RuntimeParams
    from x_maps_amd.engine import XMapsEngine
    from x_maps_amd.ingest import DeviceIngest
    header = open(os.path.join(N.ROOT, "include", "xmaps.h")).read()
    for name in ("xm_cloud_set_tables", "xm_frames_to_point_clouds", "xm_ingest_set_cloud_output", "xm_ingest_copy_cloud"):
        assert name in N.SYMBOLS and f"int {name}(" in header
    assert "#define XM_API_VERSION 5" in header and "xm_frame_cloud_stats" in header
    assert [n for n, _ in N.xm_frame_cloud_stats._fields_] == list(K.STAT_FIELDS)
    assert hasattr(XMapsEngine, "frames_to_point_clouds") and hasattr(XMapsEngine, "set_frame_cloud_tables")
    assert hasattr(DeviceIngest, "cloud") and hasattr(DeviceIngest, "set_cloud_output")
    assert RuntimeParams.__dataclass_fields__["cloud_callback"].default is None
    assert RuntimeParams.__dataclass_fields__["cloud_max_points"].default == 262144
