"""-m gpu: every K1 family at the borders of its time-stamp domain (the frames: tests/stamp_edge_cases.py; that they are what they
claim: tests/test_stamp_edge_cases_cpu.py).  int64 frames that span 2^32 - 2 .. 2^63 - 1 us from zero, small and negative bases,
with probe stamps around every column boundary; one wild stamp 2^34 us ahead; all stamps equal; dense float32 / float64 frames.
Through K0 + the tiled K1 on 64-bit keys, the one-thread-per-event K1, the compact key frame of both views, the column tiles and
the owner tiles, lone, in groups and in captured groups.

Every comparison is np.array_equal on depth, BGR and the inlier count against oracle/xmaps_oracle.py:process_ev_frame on the same
stamps in the same dtype; where a path exposes them, A3's u16 disparity frame and the per-event outputs as well, so that a
coincidence in K2 cannot hide an error of K1.  Every test asserts the path it meant to take (path_counts / sorted_fallbacks).

What the paths make of a long frame, read from the code:
  * K0 + tiled / direct K1 (64-bit keys): TimeNorm<long long>::column_exact whenever the span or t - tmin leaves 32 bits; exact.
  * compact key frame (KEY32 / CAM32): the same TimeNorm on (t[0], t[n-1]); it carries no 32-bit quantity of time, so it TAKES
    every span and only objects where an event's column leaves the tile's LDS window -- a stretched frame has the short frame's
    columns, so no frame here is redone.
  * column / owner tiles: a = t - tmin in 32 bits; the boundary pass writes "K1 objects" for a span >= 0xffffffff, every tile then
    objects and the frame is redone on the 64-bit path (by the host, or inside a captured group by the kernels); spans up to
    2^32 - 2 run on the tiles."""
import numpy as np
import pytest

from conftest import xm_option

import stamp_edge_cases as K
import xmaps_oracle as O
from x_maps_amd import XMapsEngine
from x_maps_amd import _native as N
from x_maps_amd import synthetic as S

pytestmark = pytest.mark.gpu

T_CODE = {"int64": N.XM_T_INT64, "float32": N.XM_T_FLOAT32, "float64": N.XM_T_FLOAT64}


class _Dev:
    """device buffers of one test, through the engine's own allocator"""

    def __init__(self, eng):
        self.eng, self.ptrs = eng, []

    def alloc(self, nbytes):
        p = self.eng.dev_alloc(max(int(nbytes), 16))
        self.ptrs.append(p)
        return p

    def up(self, arr, shift=0):
        """upload `arr`, `shift` elements behind a 16-byte aligned address"""
        arr = np.ascontiguousarray(arr)
        p = self.alloc(arr.nbytes + 16 * arr.itemsize) + shift * arr.itemsize
        if arr.nbytes:
            self.eng.dev_upload(p, arr)
        return p

    def down(self, ptr, shape, dtype):
        out = np.empty(shape, dtype)
        self.eng.dev_download(out, ptr)
        return out

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.eng.dev_free(p)
        return False


def _same(d, b, n_inliers, r, label):
    assert n_inliers is None or n_inliers == int(r["mask"].sum()), label
    assert np.array_equal(d, r["depth"]), label
    assert np.array_equal(b, r["bgr"]), label


def _run_device(eng, x, y, t, p=None, shift=0):
    """one frame from device-resident SoA columns (shift = 1: columns aligned to their element only, not to 16 bytes)"""
    with _Dev(eng) as dv:
        px = eng.out_h * eng.out_w
        d_d, d_b = dv.alloc(px * 4), dv.alloc(px * 3)
        X, Y, T = dv.up(x, shift), dv.up(y, shift), dv.up(t, shift)
        P = None if p is None else dv.up(np.ascontiguousarray(p, dtype=np.int16), shift)
        eng.process_frame_device(X, Y, T, P, len(t), d_d, d_b, t_dtype=T_CODE[str(np.asarray(t).dtype)])
        eng.sync()
        st = eng.last_frame_stats()
        return dv.down(d_d, (eng.out_h, eng.out_w), np.float32), dv.down(d_b, (eng.out_h, eng.out_w, 3), np.uint8), st


def _run_layout(eng, evs, layout):
    if layout == "aos":
        return eng.process_events(evs)
    x, y, t, _ = S.to_soa(evs)
    return _run_device(eng, x, y, t, shift=0 if layout == "soa" else 1)


def _check_event_outputs(eng, x, y, t, r, scale, label):
    """xm_debug_event_outputs against the oracle's per-event arrays: the time column of EVERY event, rectified coordinates, mask
    and disparity"""
    dbg = eng.debug_event_outputs(x, y, t)
    assert np.array_equal(dbg["ts"], O.time_to_xmap_column(t, scale)), label
    assert np.array_equal(dbg["xr"], r["xr"]) and np.array_equal(dbg["yr"], r["yr"]), label
    assert np.array_equal(dbg["mask"], r["mask"]) and np.array_equal(dbg["disp"][r["mask"]], r["disp"]), label


def _group_soa(eng, dv, frames, t_kind="int64", ps=None):
    """frames [(x, y, t)] as one set of device columns: (launch(), read() -> (depth [F], bgr [F]), pointers for graph_create)"""
    F, px = len(frames), eng.out_h * eng.out_w
    offs = np.concatenate(([0], np.cumsum([len(f[2]) for f in frames]))).astype(np.uint64)
    X = dv.up(np.concatenate([f[0] for f in frames]).astype(np.uint16))
    Y = dv.up(np.concatenate([f[1] for f in frames]).astype(np.uint16))
    T = dv.up(np.concatenate([f[2] for f in frames]))
    P = None if ps is None else dv.up(np.concatenate(ps).astype(np.int16))
    d_d, d_b = dv.alloc(F * px * 4), dv.alloc(F * px * 3)

    def read():
        return dv.down(d_d, (F, eng.out_h, eng.out_w), np.float32), dv.down(d_b, (F, eng.out_h, eng.out_w, 3), np.uint8)

    def clear():
        eng.dev_upload(d_d, np.full(F * px, 7.0, np.float32))
        eng.dev_upload(d_b, np.full(F * px * 3, 9, np.uint8))

    return (X, Y, T, P, offs, d_d, d_b, T_CODE[t_kind]), read, clear


# ---- int64 spans: K0, then the tiled K1 on 64-bit keys (dense) or the one-thread-per-event K1 (sparse) ------------------------------
@pytest.mark.parametrize("layout", ["soa", "soa_unaligned", "aos"])
@pytest.mark.parametrize("n", [K.N_SPARSE, K.N_DENSE, K.N_RAGGED])
@pytest.mark.parametrize("camera", [False, True])
def test_general_path_is_exact_at_every_span(camera, n, layout):
    _, tb = K.rig("tiny")
    cases = K.int64_cases("tiny", n)
    with XMapsEngine(tb, camera_perspective=camera, try_sorted=False) as eng:
        for name, span, evs in cases:
            r = K.ref_events("tiny", (name, n), evs, camera)
            d, b, st = _run_layout(eng, evs, layout)
            _same(d, b, st.n_inliers, r, name)
            assert st.n_index_errors == 0 and st.n_unsorted == 0, name
            assert (st.t_min, st.t_max) == (float(evs["t"][0]), float(evs["t"][-1])), name  # (K0's extrema, as float64)
            if layout == "soa":
                x, y, t, _ = S.to_soa(evs)
                _check_event_outputs(eng, x, y, t, r, tb["t_px_scale"], name)
        pc = eng.path_counts()
        assert pc == {"general": len(cases), "sorted_key64": 0, "key32": 0, "cols": 0}, pc
        assert eng.sorted_fallbacks() == 0


# ---- the engine's default: the verified (t[0], t[n-1]) shortcut ---------------------------------------------------------------------
@pytest.mark.parametrize("n", [K.N_SPARSE, K.N_DENSE, K.N_RAGGED])
@pytest.mark.parametrize("camera", [False, True])
def test_default_engine_takes_every_span_on_the_compact_key_frame(camera, n):
    """Lone frames, library defaults (no column tiles for lone frames).  Dense frames take the compact key frame -- key32 in
    projector view, cam32 in camera view -- at EVERY span: it holds no time in 32 bits (TimeNorm's exact form serves the long
    frames), and the stretched frames' columns are the short frame's, which stays inside the tiles' LDS windows: nothing is redone.
    Sparse frames: the shortcut in front of the one-thread-per-event K1 (counter sorted_key64)."""
    cfg, tb = K.rig("tiny")
    cases = K.int64_cases("tiny", n)
    with XMapsEngine(tb, camera_perspective=camera) as eng:
        short = K.base_events(cfg, n)
        d, b, st = eng.process_events(short)
        _same(d, b, st.n_inliers, K.ref_events("tiny", ("short", n), short, camera), "short")
        assert eng.sorted_fallbacks() == 0  # the short frame holds the windows; so do its stretched forms
        for i, (name, span, evs) in enumerate(cases):
            r = K.ref_events("tiny", (name, n), evs, camera)
            if i % 2:
                d, b, st = eng.process_events(evs)
            else:
                x, y, t, _ = S.to_soa(evs)
                d, b, st = eng.process_frame(x, y, t)
            _same(d, b, st.n_inliers, r, name)
            assert st.n_unsorted == 0 and (st.t_min, st.t_max) == (float(evs["t"][0]), float(evs["t"][-1])), name
        pc = eng.path_counts()
        want = "key32" if n >= K.N_DENSE else "sorted_key64"
        assert pc[want] == len(cases) + 1 and sum(pc.values()) == len(cases) + 1, pc
        assert eng.sorted_fallbacks() == 0


@pytest.mark.parametrize("rig_name,n,mode", [("tiny", K.N_DENSE, "cols"), ("shared", K.N_SHARED, "own")])
@pytest.mark.parametrize("kind", ["stretch", "probes"])
def test_lone_frames_on_the_tiles_up_to_their_largest_span(kind, rig_name, n, mode):
    """XM_COLS=2 sends lone frames to the column tiles (C-tiny) / the owner tiles (C-shared).  Up to a span of 2^32 - 2 they run
    there (A3's u16 frame is compared as well); from 0xffffffff on the boundary pass objects, every tile objects, and the host redoes
    the frame on the 64-bit path: sorted_fallbacks() == 1, the result exact.  (One engine per frame: three redone frames in a row
    would pause the compact paths.)"""
    xm_option("XM_COLS", "2")
    _, tb = K.rig(rig_name)
    for name, span, evs in K.int64_cases(rig_name, n):
        if not name.startswith(kind):
            continue
        r = K.ref_events(rig_name, (name, n), evs)
        with XMapsEngine(tb) as eng:
            assert eng.cols_info()["mode"] == mode
            x, y, t, _ = S.to_soa(evs)
            d, b, st = eng.process_frame(x, y, t)
            _same(d, b, st.n_inliers, r, name)
            pc = eng.path_counts()
            if span <= K.TILE_SPAN_MAX:
                assert pc == {"general": 0, "sorted_key64": 0, "key32": 0, "cols": 1} and eng.sorted_fallbacks() == 0, (name, pc)
                assert st.n_unsorted == 0, name
                assert np.array_equal(eng.debug_last_disp_frame(), np.asarray(r["disp_map"]).astype(np.uint16)), name
            else:
                assert pc["cols"] == 1 and pc["key32"] == 0 and sum(pc.values()) == 2 and eng.sorted_fallbacks() == 1, (name, pc)
            d, b, st = eng.process_events(evs)  # the same frame as records, on the same slot
            _same(d, b, st.n_inliers, r, name)
            assert eng.path_counts()["cols"] == 2 and eng.sorted_fallbacks() == (0 if span <= K.TILE_SPAN_MAX else 2), name


# ---- groups: a short frame, one at the tiles' largest span, one past it -----------------------------------------------------------
def _group_refs(rig_name, n):
    frames = K.group_frames(rig_name, n)
    return frames, [K.ref_events(rig_name, ("group", n, i), e) for i, e in enumerate(frames)]


@pytest.mark.parametrize("rig_name,n,mode", [("tiny", K.N_DENSE, "cols"), ("shared", K.N_SHARED, "own")])
@pytest.mark.parametrize("layout", ["aos", "soa"])
def test_groups_redo_only_the_frame_that_is_too_long(rig_name, n, mode, layout):
    """Three frames in one set of multi-frame launches, twice on the same slots: all take the tiles (column tiles on C-tiny, owner
    tiles on C-shared); the frame of 2^32 + 1 us objects and is redone, the other two are not; every frame is exact both times --
    no cell of a neighbour, of the attempt or of the previous round shows."""
    _, tb = K.rig(rig_name)
    frames, refs = _group_refs(rig_name, n)
    with XMapsEngine(tb, n_slots=3) as eng:
        assert eng.cols_info()["mode"] == mode
        for rep in range(2):
            if layout == "aos":
                out = eng.process_event_frames(frames)
            else:
                with _Dev(eng) as dv:
                    args, read, clear = _group_soa(eng, dv, [S.to_soa(e)[:3] for e in frames])
                    clear()
                    eng.process_batch_device(*args[:5], args[5], args[6], t_dtype=args[7])
                    eng.sync()
                    out = list(zip(*read()))
            for f, (d, b) in enumerate(out):
                _same(d, b, None, refs[f], (rep, f))
            assert eng.path_counts()["cols"] == 3 * (rep + 1) and eng.sorted_fallbacks() == rep + 1, (rep, eng.path_counts())
        pc = eng.path_counts()
        assert pc["key32"] == 0 and sum(pc.values()) == 6 + 2, pc  # (a redone frame counts twice)


@pytest.mark.parametrize("rig_name,n,mode", [("tiny", K.N_DENSE, "cols"), ("shared", K.N_SHARED_CAPTURED, "own")])
def test_captured_groups_redo_the_long_frame_on_the_device(rig_name, n, mode):
    """The same three frames captured into a graph (n_slots = 4: one group of three): no host is at hand for the redo, the kernels
    decide per frame on the device.  Launched twice, every frame exact both times.  (C-shared: 80 000 events per frame -- a captured
    group takes the tiles only where it is dense enough for the tiled K1 too, which redoes its frames.)"""
    _, tb = K.rig(rig_name)
    frames, refs = _group_refs(rig_name, n)
    with XMapsEngine(tb, n_slots=4, default_priority_streams=True) as eng:
        assert eng.cols_info()["mode"] == mode
        with _Dev(eng) as dv:
            args, read, clear = _group_soa(eng, dv, [S.to_soa(e)[:3] for e in frames])
            g = eng.graph_create(*args[:5], args[5], args[6], t_dtype=args[7])
            assert eng.path_counts()["cols"] == 3, eng.path_counts()  # captured with the tiles in front
            for rep in range(2):
                clear()
                g.launch()
                eng.sync()
                d, b = read()
                for f in range(3):
                    _same(d[f], b[f], None, refs[f], (rep, f))
            g.close()
        assert eng.sorted_fallbacks() == 0  # (the host redid nothing)


# ---- one wild stamp -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [None, "2"])
@pytest.mark.parametrize("camera", [False, True])
def test_one_wild_stamp_lone(camera, cols):
    """Event k moved 2^34 us ahead.  k in the middle: the stream is unsorted, the event lies outside [t[0], t[n-1]], every
    shortcut objects (n_unsorted > 0) and the frame is redone with K0.  k = n - 1: sorted, span past 2^32; every other event falls
    into column 0 and the last into column S -- in projector view outside its tile's LDS window of 5 time columns (compact key frame),
    or the span is refused (column tiles): redone; in camera view the compact frame orders any event exactly: not redone."""
    if cols:
        xm_option("XM_COLS", cols)
    _, tb = K.rig("tiny")
    for k, evs in K.wild_frames("tiny", K.N_DENSE).items():
        r = K.ref_events("tiny", ("wild", K.N_DENSE, k), evs, camera)
        with XMapsEngine(tb, camera_perspective=camera) as eng:
            x, y, t, _ = S.to_soa(evs)
            d, b, st = eng.process_frame(x, y, t)
            _same(d, b, st.n_inliers, r, k)
            assert (st.t_min, st.t_max) == (float(t.min()), float(t.max())), k
            pc = eng.path_counts()
            first = "cols" if cols and not camera else "key32"
            redone = 0 if camera and k == "last" else 1
            assert pc[first] == 1 and sum(pc.values()) == 1 + redone and eng.sorted_fallbacks() == redone, (k, pc)
            if k == "middle":
                assert st.n_unsorted > 0
            _check_event_outputs(eng, x, y, t, r, tb["t_px_scale"], k)


@pytest.mark.parametrize("rig_name,n", [("tiny", K.N_DENSE), ("shared", K.N_SHARED)])
def test_one_wild_stamp_in_a_group(rig_name, n):
    _, tb = K.rig(rig_name)
    cfg, _ = K.rig(rig_name)
    w = K.wild_frames(rig_name, n)
    frames = [K.base_events(cfg, n, 1), w["middle"], w["last"]]
    refs = [K.ref_events(rig_name, ("group", n, 0), frames[0]), K.ref_events(rig_name, ("wild", n, "middle"), frames[1]),
            K.ref_events(rig_name, ("wild", n, "last"), frames[2])]
    with XMapsEngine(tb, n_slots=3) as eng:
        out = eng.process_event_frames(frames)
        for f, (d, b) in enumerate(out):
            _same(d, b, None, refs[f], f)
        assert eng.path_counts()["cols"] == 3 and eng.sorted_fallbacks() == 2, eng.path_counts()


# ---- float stamps, dense ----------------------------------------------------------------------------------------------------------------
def _float_frames(kind, use_p):
    """[(name, sorted?, x, y, t of the kind, p | None, the events the reference sees)]"""
    out = []
    rng = np.random.default_rng(31)
    for name, is_sorted, x, y, t64 in K.float_cases("tiny", K.N_DENSE, kind):
        t = t64.astype(kind)
        p = rng.integers(0, 2, len(t)).astype(np.int16) if use_p else None
        out.append((name, is_sorted, x, y, t, p))
    return out


def _float_ref(kind, name, x, y, t, p, camera):
    if p is None:
        return K.ref("tiny", (kind, name), x, y, t, camera)
    keep = p == 1
    return K.ref("tiny", (kind, name, "p"), x[keep], y[keep], t[keep], camera)


@pytest.mark.parametrize("use_p", [False, True])
@pytest.mark.parametrize("kind", ["float32", "float64"])
@pytest.mark.parametrize("camera", [False, True])
def test_dense_float_frames_lone(camera, kind, use_p):
    """K0<T> and the lone tiled K1<T> (64-bit keys) on 24 000 float events per frame: view x type x polarity column, 16-byte
    aligned and element-aligned columns."""
    _, tb = K.rig("tiny")
    frames = _float_frames(kind, use_p)
    with XMapsEngine(tb, camera_perspective=camera, try_sorted=False) as eng:
        for name, _, x, y, t, p in frames:
            r = _float_ref(kind, name, x, y, t, p, camera)
            for shift in (0, 1):
                d, b, st = _run_device(eng, x, y, t, p, shift)
                _same(d, b, st.n_inliers, r, (name, shift))
                assert st.n_used == (len(t) if p is None else int((p == 1).sum())), name
            d, b, st = eng.process_frame(x, y, t, p)
            _same(d, b, st.n_inliers, r, name)
            if p is None:
                _check_event_outputs(eng, x, y, t, r, tb["t_px_scale"], name)
        pc = eng.path_counts()
        assert pc == {"general": 3 * len(frames), "sorted_key64": 0, "key32": 0, "cols": 0}, pc


@pytest.mark.parametrize("use_p", [False, True])
@pytest.mark.parametrize("kind", ["float32", "float64"])
@pytest.mark.parametrize("camera", [False, True])
def test_dense_float_frames_in_groups(camera, kind, use_p):
    """The same matrix through xm_process_batch with t_dtype (k_scatter_tiled_batch<T>), on an engine that runs K0 for every frame
    and on the default engine.  On the default engine a group without a polarity column takes the verified shortcut and the compact
    key frame -- float stamps never take the column tiles (cols_events) --, and the raster-ordered frame fails the shortcut and is
    redone; with a polarity column every frame runs K0."""
    _, tb = K.rig("tiny")
    frames = _float_frames(kind, use_p)
    F = len(frames)
    refs = [_float_ref(kind, name, x, y, t, p, camera) for name, _, x, y, t, p in frames]
    n_unsorted = sum(not f[1] for f in frames)
    for try_sorted in (False, True):
        with XMapsEngine(tb, camera_perspective=camera, n_slots=F, try_sorted=try_sorted) as eng, _Dev(eng) as dv:
            args, read, clear = _group_soa(eng, dv, [(f[2], f[3], f[4]) for f in frames], kind, [f[5] for f in frames] if use_p else None)
            for rep in range(2):
                clear()
                eng.process_batch_device(*args[:5], args[5], args[6], t_dtype=args[7])
                eng.sync()
                d, b = read()
                for f in range(F):
                    _same(d[f], b[f], None, refs[f], (try_sorted, rep, frames[f][0]))
            pc = eng.path_counts()
            assert pc["cols"] == 0, pc
            if try_sorted and not use_p:
                assert pc["key32"] == 2 * F and eng.sorted_fallbacks() == 2 * n_unsorted and sum(pc.values()) == 2 * (F + n_unsorted), pc
            else:
                assert pc == {"general": 2 * F, "sorted_key64": 0, "key32": 0, "cols": 0} and eng.sorted_fallbacks() == 0, pc


@pytest.mark.parametrize("kind", ["float32", "float64"])
@pytest.mark.parametrize("camera", [False, True])
def test_sorted_float_frames_take_the_shortcut_and_the_compact_key_frame(camera, kind):
    """The engine's default on a dense, sorted float frame: (t[0], t[n-1]) as the extrema, verified per event in T's own order
    (TimeCodec<T>), then the compact key frame -- KEY32 (projector view) / CAM32 (camera view) with T = float / double.  The same
    frames with K0 in front give the same arrays."""
    _, tb = K.rig("tiny")
    frames = [f for f in _float_frames(kind, False) if f[1]]
    assert len(frames) >= 2
    got = []
    with XMapsEngine(tb, camera_perspective=camera) as eng:
        for name, _, x, y, t, _p in frames:
            r = _float_ref(kind, name, x, y, t, None, camera)
            d, b, st = eng.process_frame(x, y, t)
            _same(d, b, st.n_inliers, r, name)
            assert st.n_unsorted == 0 and (st.t_min, st.t_max) == (float(t[0]), float(t[-1])), name
            d2, b2, st2 = _run_device(eng, x, y, t, None, 1)
            _same(d2, b2, st2.n_inliers, r, (name, "element-aligned"))
            got.append((d, b, st.n_inliers))
        pc = eng.path_counts()
        assert pc == {"general": 0, "sorted_key64": 0, "key32": 2 * len(frames), "cols": 0} and eng.sorted_fallbacks() == 0, pc
    with XMapsEngine(tb, camera_perspective=camera, try_sorted=False) as eng:
        for (name, _, x, y, t, _p), (d0, b0, n0) in zip(frames, got):
            d, b, st = eng.process_frame(x, y, t)
            assert np.array_equal(d, d0) and np.array_equal(b, b0) and st.n_inliers == n0, name
        assert eng.path_counts()["general"] == len(frames)


@pytest.mark.parametrize("kind", ["int64", "float32", "float64"])
@pytest.mark.parametrize("camera", [False, True])
def test_all_stamps_equal(camera, kind):
    """tmax == tmin: 0 / 0 -> column 0 for every event (`degenerate`), which no X-map defines: an empty frame, on every path."""
    cfg, tb = K.rig("tiny")
    evs = K.equal(K.base_events(cfg, K.N_DENSE, 6))
    x, y, t, _ = S.to_soa(evs)
    t = (t - t[0] + 1_048_576).astype(kind)  # 2^20: exact in every type
    r = K.ref("tiny", ("equal", kind), x, y, t, camera)
    assert not r["depth"].any()
    for try_sorted, cols in ((False, None), (True, None), (True, "2")):
        xm_option("XM_COLS", cols)
        with XMapsEngine(tb, camera_perspective=camera, try_sorted=try_sorted) as eng:
            d, b, st = eng.process_frame(x, y, t)
            _same(d, b, st.n_inliers, r, (try_sorted, cols))
            assert st.n_inliers == 0 and st.n_index_errors == 0 and st.t_min == st.t_max == float(t[0])
            _check_event_outputs(eng, x, y, t, r, tb["t_px_scale"], (try_sorted, cols))
            pc = eng.path_counts()
            want = "general" if not try_sorted else "cols" if cols and kind == "int64" and not camera else "key32"
            assert pc[want] == 1 and sum(pc.values()) == 1 and eng.sorted_fallbacks() == 0, (try_sorted, cols, pc)
