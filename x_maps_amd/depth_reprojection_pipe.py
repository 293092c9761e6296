"""DepthReprojectionPipe with the reference's interface (python/depth_reprojection_pipe.py:37-175) and the
hot path on the GPU.

    pipe = DepthReprojectionPipe(params, stats_printer, frame_callback)
    pipe.process_events(evs)        # packets from the camera / file reader
    pipe.process_ev_frame(evs)      # one projector frame of EventCD records -> frame_callback(BGR u8)

`process_ev_frame` is the function the trigger finder calls (trigger_finder.py:172).  In the reference it
runs six NumPy/Numba/OpenCV stages; here it is one C-ABI call (xm_process_frame_aos) = three HIP kernels,
and the frame handed to `frame_callback` is a fresh (H, W, 3) uint8 BGR array exactly as before.
The packet side mirrors pipe:110-119: polarity filter -> activity-noise filter -> trigger finder -- by default (round 6) as
kernels of the device ingest (RuntimeParams.device_ingest: process_events(packet) stages the packet and returns; the frames
arrive through frame_callback as the consumer's own arrays; with RuntimeParams.device_frame_filters a selected frame event filter
is a stage of that ingest, too), or on the host (the opt-out, and whenever a frame event filter -- without that parameter -- or a
caller-supplied activity filter is selected) with x_maps_amd.activity_filter.ActivityNoiseFilterAlgorithm (the same kernels behind one call);
Metavision's own filter is a binary of the SDK, so the rule is this build's definition (oracle/ingest_oracle.py).
Out of scope in this build: the timing watchdog.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, Optional

import numpy as np

from .cam_proj_calibration import CamProjMaps, load_tables_npz
from .disp_to_depth import DisparityToDepth
from .frame_event_filter import FrameEventFilterProcessor, NoFilter
from .stats import StatsPrinter
from .trigger_finder import RobustTriggerFinder
from .x_maps_disparity import XMapsDisparity


_ACT_WARNED = False


def _warn_activity_rule_unpinned() -> None:
    """Once per process: this build's activity-noise rule (an earlier event at one of the 8 neighbours within T, inclusive; the own
    pixel does not count; per-pixel maximum stamp) is its own definition -- Metavision's ActivityNoiseFilterAlgorithm
    (depth_reprojection_pipe.py:65-67 of the reference) ships as a binary and no fixture of it exists yet
    (tests/golden/g10_metavision.npz, written by tools/pin_thirdparty.py on a reference installation).  Frames may differ from the
    reference's by the events the two rules judge differently; pass `activity_filter=` (Metavision's own) for the reference's rule."""
    global _ACT_WARNED
    if _ACT_WARNED:
        return
    _ACT_WARNED = True
    import os
    import warnings
    if not os.path.exists(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "g10_metavision.npz")):
        warnings.warn("x_maps_amd: the activity-noise filter runs this build's own rule, unpinned against Metavision's "
                      "ActivityNoiseFilterAlgorithm (no g10_metavision.npz fixture yet: tools/pin_thirdparty.py); pass the SDK's "
                      "filter as DepthReprojectionPipe(activity_filter=...) or RuntimeParams(activity_filter=False) to leave it out",
                      RuntimeWarning, stacklevel=3)


@dataclass
class DepthReprojectionPipe:
    params: "RuntimeParams"
    stats_printer: StatsPrinter
    frame_callback: Callable

    calib_maps: CamProjMaps = field(init=False)
    x_maps_disp: XMapsDisparity = field(init=False)
    disp_to_depth: DisparityToDepth = field(init=False)
    trigger_finder: RobustTriggerFinder = field(init=False)
    # host path: callable(pos_events) -> kept events.  None = this build's filter when RuntimeParams.activity_filter is on
    # (the default, as in the reference); plug Metavision's own filter in here where the SDK is installed
    activity_filter: Optional[Callable[[np.ndarray], np.ndarray]] = None
    fused: bool = True  # False = run the reference's six stages one by one (each still a HIP kernel)

    def __post_init__(self):
        p = self.params
        self._frame_sync = getattr(p, "frame_sync", "pauses")  # (checked before anything is made on the device)
        if self._frame_sync not in ("pauses", "ext_trigger"):
            raise ValueError('RuntimeParams.frame_sync must be "pauses" or "ext_trigger"')
        if getattr(p, "ext_trigger_edge", "rising") not in ("rising", "falling", "both"):
            raise ValueError('RuntimeParams.ext_trigger_edge must be "rising", "falling" or "both"')
        tables = getattr(p, "tables", None)
        if tables is None:
            if isinstance(p.calib, str) and p.calib.endswith(".npz"):
                tables = load_tables_npz(p.calib)  # exported from a reference installation
            elif isinstance(p.calib, str):
                # the reference's own calibration YAML: tables from the cv2-free builder (x_maps_amd/calibration.py; the
                # rectifying rotations are pinned to OpenCV's, focal length / principal point are unpinned -- DESIGN.md),
                # X-map built on the GPU.  Mirrors pipe:69-90.
                from . import calibration as calib
                cp = calib.CamProjCalibrationParams.from_yaml(p.calib, p.camera_width, p.camera_height,
                                                              p.projector_width, p.projector_height)
                tm = np.load(p.projector_time_map) if p.projector_time_map else None
                tables = calib.build_tables(cp, z_near=p.z_near, z_far=p.z_far, device=getattr(p, "device", 0),
                                            projector_time_map_rectified=tm,
                                            maps_on_device=bool(getattr(p, "tables_on_device", False)))
                self.stats_printer.log("tables built by the cv2-free builder")
            else:
                raise ValueError("RuntimeParams.calib must be a calibration .yaml, an exported tables .npz, or set .tables")
        tables = dict(tables)
        tables.setdefault("z_near", p.z_near)
        tables.setdefault("z_far", p.z_far)
        tables["z_near"], tables["z_far"] = p.z_near, p.z_far
        cam_h, cam_w = np.asarray(tables["cam_mapx_i16"]).shape
        if (cam_w, cam_h) != (p.camera_width, p.camera_height):
            raise ValueError(f"tables are for a {cam_w}x{cam_h} camera, params say {p.camera_width}x{p.camera_height}")
        # frames cut out of the camera stream by the trigger finder are time-sorted (NoFilter): let the GPU take
        # (tmin, tmax) = (t[0], t[-1]) and verify it; an unsorted frame handed to process_ev_frame directly is detected
        # on the device and redone on the general path inside the same call, so results are exact either way
        self.calib_maps = CamProjMaps(tables, camera_perspective=p.camera_perspective,
                                      device=getattr(p, "device", 0), assume_time_sorted=True)
        self.x_maps_disp = XMapsDisparity(self.calib_maps)
        self.disp_to_depth = DisparityToDepth(stats=self.stats_printer, calib_maps=self.calib_maps,
                                              z_near=p.z_near, z_far=p.z_far)
        self.ev_filter_proc = FrameEventFilterProcessor(self.calib_maps.engine)
        self.trigger_finder = RobustTriggerFinder(projector_fps=p.projector_fps, stats=self.stats_printer,
                                                  frame_callback=self.process_ev_frame)
        # device-side ingest (row N2): raw packets go to the GPU, which filters, buffers, cuts frames and runs the hot path on
        # them without the event stream (or any index into it) coming back to the host
        self.ingest = None
        self._raw_dev, self._raw_host = {}, {}  # RAW / DAT decoders (process_evt3_words / _evt2_words / _evt21_words / process_dat_records), created on first use
        self._own_act_filter = None
        self._host_chain_active = False
        self._device_frame_filters = bool(getattr(p, "device_frame_filters", False))
        self._ingest_filter = (0, False)  # what the ingest has been told (DeviceIngest.set_frame_filter)
        self._ingest_filter_refused = False
        self._ingest_failed = False  # an ingest call has raised: the error has reached the caller, close() does not ask again
        self._closed = False
        self._surface_callback = getattr(p, "surface_callback", None)
        self._surface_kind = (getattr(p, "surface_select", "last"), getattr(p, "surface_dtype", np.float32))
        self._cloud_callback = getattr(p, "cloud_callback", None)
        if self._cloud_callback is not None:  # (tables without the float rectify maps or Q: ValueError, here and not at the first frame)
            self.calib_maps.engine.set_frame_cloud_tables()
        self._record_callback = getattr(p, "record_callback", None)
        self._record_kind = (bool(getattr(p, "record_use_vectors", True)), int(getattr(p, "record_max_words", 1 << 21)))
        # frames cut at the recording's EXT_TRIGGER words instead of pauses (RuntimeParams.frame_sync; ext_trigger.py): a chain of its
        # own behind process_*_words -- decoder with extraction on, TriggeredFrames, the group entries on the device buffer --
        # made on first use; neither the ingest nor the host chain exists in this mode
        self._trig, self._trig_dev, self._trig_bgr = None, {}, None
        self._trig_filter, self._trig_filter_refused = (0, False), False  # what the buffer has been told (TriggeredFrames.set_frame_filter)
        if self._frame_sync == "ext_trigger":
            return
        if self.activity_filter is None and getattr(p, "activity_filter", True):
            _warn_activity_rule_unpinned()
        # a caller-supplied activity filter (Metavision's own, where the SDK is installed) runs on the host: so does the chain
        if getattr(p, "device_ingest", True) and self.activity_filter is None:
            from .ingest import DeviceIngest
            self.ingest = DeviceIngest(self.calib_maps.engine, p.projector_fps, use_polarity=True,
                                       activity_filter=bool(getattr(p, "activity_filter", True)), want_depth=False,
                                       activity_thresh_us=self._activity_thresh_us(), activity_include_self=bool(getattr(p, "activity_include_self", False)),
                                       result_ring=int(getattr(p, "ingest_result_ring", 16)),
                                       lossless=not p.should_drop_frames)  # no_frame_dropping (the default): never lap the ring
            self._ingest_views = bool(getattr(p, "ingest_frame_views", False))
            if self._surface_callback is not None:  # (before the first push: every frame of the stream gets a surface)
                self.ingest.set_surface_output(*self._surface_kind)
            if self._cloud_callback is not None:
                self.ingest.set_cloud_output(True, int(getattr(p, "cloud_max_points", 262144)))
            if self._record_callback is not None:
                self.ingest.set_record_output(True, *self._record_kind)
        else:
            self._ensure_host_chain()

    def _activity_thresh_us(self) -> int:
        """int(1e6 / fps) as the reference passes it (pipe:65-68); one less for the strict comparison (integer stamps)"""
        p = self.params
        return int(1e6 / p.projector_fps) - (1 if getattr(p, "activity_strict", False) else 0)

    def _ensure_host_chain(self):
        """the host chain's activity filter (pipe:65-67), made when the chain is first needed"""
        p = self.params
        if self.activity_filter is None and getattr(p, "activity_filter", True):
            from .activity_filter import ActivityNoiseFilterAlgorithm
            self._own_act_filter = ActivityNoiseFilterAlgorithm(self.calib_maps.engine, self._activity_thresh_us(),  # pipe:65-67
                                                                include_self=bool(getattr(p, "activity_include_self", False)))
            self.activity_filter = self._own_act_filter

    def _use_ingest(self) -> bool:
        """Packets go to the device ingest unless a frame event filter is selected (pipe:131-139: those filters re-order the cut
        frame's events on the host, between the trigger finder and the hot path) -- then the host chain takes the stream, from a
        clean start on either side (a switch is a user pressing E: the frames around it are not comparable anyway)."""
        if self.ingest is None:
            return False
        sel = self.ev_filter_proc.selected_filter()
        want_host = not isinstance(sel, NoFilter)
        if self._device_frame_filters:
            # RuntimeParams.device_frame_filters: the filter is a stage of the ingest -- the stream stays where it is, the ingest is
            # told which filter the packets from now on are pushed under; only a filter it refuses takes the host chain
            want = (int(getattr(sel, "filter_id", 0)), bool(getattr(sel, "intended_semantics", False))) if want_host else (0, False)
            if want != self._ingest_filter:
                try:
                    self.ingest.set_frame_filter(*want)
                    self._ingest_filter_refused = False
                except ValueError as e:
                    self._ingest_filter_refused = True
                    self.stats_printer.log(f"{sel}: not available on the device ingest ({e}); the host chain takes the stream")
                self._ingest_filter = want
            want_host = want_host and self._ingest_filter_refused
        if want_host != self._host_chain_active:
            self._host_chain_active = want_host
            if want_host:
                self.flush()
                self.ingest.reset()
                self._ensure_host_chain()
                if self._own_act_filter is not None:
                    self._own_act_filter.reset()
            self.trigger_finder.reset()
        return not want_host

    # ---- packets -> frames (host side, in front of the hot path) ---------------------------------------
    def _deliver_ingest_frames(self):
        for fr in self.ingest.poll(copy=not self._ingest_views):
            if fr.lost:  # the result ring was lapped before the host polled: the frame's images are gone (never shown)
                self.stats_printer.count("frame lost")
                continue
            self.stats_printer.count("trig ✅")
            self.stats_printer.add_metric("frame len [ms]", (fr.t_last - fr.t_first) / 1000)
            if self._device_frame_filters and fr.n_events:
                self.stats_printer.add_metric("frame evs filtered out [%]", 100 - fr.n_kept / fr.n_events * 100)
            self.last_ingest_frame = fr
            if self._surface_callback is not None:
                surf = self.ingest.surface(fr.seq)
                if surf is None:  # (the surface ring is as long as the result ring: lapped only where the frame is lost too)
                    self.stats_printer.count("surface lost")
                else:
                    self._surface_callback(surf)
            if self._cloud_callback is not None:
                cloud = self.ingest.cloud(fr.seq)
                if cloud is None:  # (the cloud ring is as long as the result ring: lapped only where the frame is lost too)
                    self.stats_printer.count("cloud lost")
                else:
                    self._cloud_callback(cloud)
            if self._record_callback is not None:
                rec = self.ingest.record(fr.seq)
                if rec is None:  # (the record ring is as long as the result ring: lapped only where the frame is lost too)
                    self.stats_printer.count("record lost")
                else:
                    self._record_callback(*rec)
            # a fresh array copied out of the pinned result ring, or (RuntimeParams.ingest_frame_views) a view into it that stays
            # valid until ingest_result_ring - 1 further frames have been produced
            self.frame_callback(fr.bgr)

    def flush(self):
        """Device ingest: wait for the packets pushed so far and deliver the frames they produced.  Never needed for
        correctness -- reset() and close() do the same -- only to see the frames sooner."""
        if self.ingest is not None and not self._ingest_failed:
            try:
                self.ingest.flush()
                self._deliver_ingest_frames()
            except BaseException:
                self._ingest_failed = True
                raise

    def process_evt3_words(self, words):
        """A chunk of a recording's EVT 3.0 words (x_maps_amd.evt3.read_raw_words) instead of an EventCD packet: decoded on the
        device in front of the ingest when `device_ingest` is on (the words cross PCIe as the file stores them), on the host
        otherwise.  What Metavision's reader + process_events do together in the reference (bias_events_iterator.py:53-96)."""
        self._process_raw_words(words, 3)

    def process_evt2_words(self, words):
        """the same for EVT 2.0 words (x_maps_amd.evt2.read_raw_words): 32-bit words, the encoding of older sensors"""
        self._process_raw_words(words, 2)

    def process_evt21_words(self, words):
        """the same for EVT 2.1 words (x_maps_amd.evt21.read_raw_words): 64-bit words of up to 32 events, in the half order
        RuntimeParams.raw_legacy_halves names"""
        self._process_raw_words(words, 21)

    def process_dat_records(self, records):
        """the same for the records of a DAT file (x_maps_amd.dat.read_raw_words): 8 bytes per event"""
        self._process_raw_words(records, "dat")

    def _raw_format(self, fmt):
        """-> (as_words, device decoder factory, host decoder factory) of a format process_*_words / _records takes"""
        from . import dat, evt2, evt21, evt3
        wait = bool(getattr(self.params, "raw_wait_for_time_base", False))
        eng = self.calib_maps.engine
        if fmt == 21:
            legacy = bool(getattr(self.params, "raw_legacy_halves", False))
            return (lambda w: np.ascontiguousarray(w, dtype="<u8"),
                    lambda: evt21.DeviceEvt21Decoder(eng, max_words=1 << 20, wait_for_time_base=wait, legacy_halves=legacy),
                    lambda: evt21.Evt21Decoder(wait, legacy))
        if fmt == "dat":
            return dat.as_records, lambda: dat.DeviceDatDecoder(eng, max_words=1 << 20), lambda: dat.DatDecoder()
        mod, dt, cls, host = (evt2, "<u4", evt2.DeviceEvt2Decoder, evt2.Evt2Decoder) if fmt == 2 else (evt3, "<u2", evt3.DeviceEvt3Decoder, evt3.Evt3Decoder)
        return (lambda w: np.ascontiguousarray(w, dtype=dt), lambda: cls(eng, max_words=1 << 20, wait_for_time_base=wait),
                lambda: host(wait))

    # ---- frame_sync = "ext_trigger": words -> trigger records + events -> frames cut at the triggers, all on the device ----
    MIN_EVENTS_PER_FRAME = 1000  # the reference's (python/trigger_finder.py): frames of that many events or fewer are not shown

    def _triggered_chain(self, fmt):
        """-> (decoder of `fmt` with extraction on, the TriggeredFrames), made on first use"""
        p = self.params
        eng = self.calib_maps.engine
        cap = int(getattr(p, "ext_trigger_cap_events", 1 << 22))
        if self._trig is None:
            from .ext_trigger import TriggeredFrames
            self._trig = TriggeredFrames(eng, cap_events=cap, id=int(getattr(p, "ext_trigger_id", -1)),
                                         edge=getattr(p, "ext_trigger_edge", "rising"), min_events=self.MIN_EVENTS_PER_FRAME,
                                         positive_only=True)  # PolarityFilterAlgorithm(1), pipe:43,114
            if getattr(p, "ext_trigger_activity_filter", False) and getattr(p, "activity_filter", True):  # pipe:65-68,116-117
                _warn_activity_rule_unpinned()
                self._trig.set_activity(self._activity_thresh_us(), bool(getattr(p, "activity_include_self", False)))
        dev = self._trig_dev.get(fmt)
        if dev is None:
            from . import evt2, evt21, evt3
            wait = bool(getattr(p, "raw_wait_for_time_base", False))
            max_words = 1 << 20
            # (a chunk never decodes to more events than the buffer holds: XM_ERR_TOO_MANY then leaves the decoder where it was)
            per_word = {3: 2, 2: 1, 21: 4}[fmt]
            kw = dict(max_words=max_words, max_events=min(per_word * max_words, cap), wait_for_time_base=wait)
            if fmt == 21:
                dev = evt21.DeviceEvt21Decoder(eng, legacy_halves=bool(getattr(p, "raw_legacy_halves", False)), **kw)
            else:
                dev = (evt2.DeviceEvt2Decoder if fmt == 2 else evt3.DeviceEvt3Decoder)(eng, **kw)
            dev.set_ext_triggers(1 << 16)
            self._trig_dev[fmt] = dev
        return dev, self._trig

    def _group_engine(self):
        """the engine of process_ev_frames: the library's default flags and a slot per frame of a group"""
        if getattr(self, "_replay_engine", None) is None:
            from .engine import XMapsEngine
            self._replay_engine = XMapsEngine(self.calib_maps.tables, camera_perspective=self.params.camera_perspective,
                                              device=getattr(self.params, "device", 0), n_slots=self.replay_group)
        return self._replay_engine

    def _deliver_triggered_frames(self):
        """Every ready frame, in runs of at most replay_group: surfaces, clouds and the frames' launches on the device buffer, one
        xm_sync, then per frame surface_callback, cloud_callback, frame_callback; the run is released behind its last callback."""
        tf = self._trig
        sel = self.ev_filter_proc.selected_filter()
        on_device = False  # RuntimeParams.device_frame_filters: the selected filter is a stage on the run, the stream stays on the device
        if self.fused and self._device_frame_filters:
            want = (0, False) if isinstance(sel, NoFilter) else (int(getattr(sel, "filter_id", 0)), bool(getattr(sel, "intended_semantics", False)))
            if want != self._trig_filter:
                try:
                    tf.set_frame_filter(want[0], want[1], max_frames=self.replay_group)
                    self._trig_filter_refused = False
                except ValueError as e:
                    self._trig_filter_refused = True
                    self.stats_printer.log(f"{sel}: not available on the device ({e}); the frames go through the host path")
                self._trig_filter = want
            on_device = want[0] != 0 and not self._trig_filter_refused
        while True:
            ptr, offs, _ = tf.ready(self.replay_group)
            n = len(offs) - 1
            if n == 0:
                return
            if not on_device and (not self.fused or not isinstance(sel, NoFilter)):
                frames = tf.download(ptr, offs)  # (the frame event filters re-order a frame's events on the host: pipe:131-139)
                tf.release(n)
                for evs in frames:
                    self.stats_printer.count("trig ✅")
                    self.process_ev_frame(evs)
                continue
            eng = self._group_engine()
            px = eng.out_h * eng.out_w * 3
            if self._trig_bgr is None:
                self._trig_bgr = eng.dev_alloc(self.replay_group * px)
            surfs = clouds = recs = None
            with self.stats_printer.measure_time("x-maps frames (fused, groups)"):
                if self._surface_callback is not None:
                    surfs, _ = eng.frames_to_time_surfaces_device(ptr, offs, *self._surface_kind)
                if self._cloud_callback is not None:
                    clouds = eng.frames_to_point_clouds_device(ptr, offs)
                if self._record_callback is not None:
                    recs = eng.frames_to_evt3_words(ptr, offs, self._record_kind[0], device=True)
                fptr, foffs = ptr, offs
                if on_device:  # (surfaces and clouds are the cut frames', in front of the filter: as the ingest orders its stages)
                    fptr, foffs, _, _ = tf.ready_filtered(n)
                    assert len(foffs) == n + 1
                    for f in range(n):
                        self.stats_printer.add_metric("frame evs filtered out [%]",
                                                      100 - int(foffs[f + 1] - foffs[f]) / max(int(offs[f + 1] - offs[f]), 1) * 100)
                eng.process_events_batch_device(fptr, foffs, None, self._trig_bgr)
                eng.sync()  # (also redoes frames whose verified shortcut failed)
                bgr = np.empty((n, eng.out_h, eng.out_w, 3), np.uint8)
                eng.dev_download(bgr, self._trig_bgr)
            for f in range(n):
                self.stats_printer.count("trig ✅")
                if surfs is not None:
                    self._surface_callback(surfs[f])
                if clouds is not None:
                    self._cloud_callback(clouds[f][0][:int(getattr(self.params, "cloud_max_points", 262144))])
                if recs is not None:
                    self._record(recs[0][f], recs[1][f])
                self.frame_callback(bgr[f])
            tf.release(n)

    def _process_raw_words_triggered(self, words, fmt):
        if fmt == "dat":
            raise ValueError('frame_sync="ext_trigger": CD DAT records carry no trigger words')
        dev, tf = self._triggered_chain(fmt)
        from ._native import XMapsTooMany
        w = dev._as_words(words)

        def push(piece):
            try:
                tf.push(dev, piece)
            except XMapsTooMany:  # (more events or trigger words than a chunk's buffers hold; nothing has advanced)
                if len(piece) < 2:
                    raise
                push(piece[:len(piece) // 2])
                push(piece[len(piece) // 2:])
                return
            self._deliver_triggered_frames()
        for a in range(0, len(w), dev.max_words):
            push(w[a:a + dev.max_words])

    def _process_raw_words(self, words, fmt):
        if self._frame_sync == "ext_trigger":
            return self._process_raw_words_triggered(words, fmt)
        as_words, make_dev, make_host = self._raw_format(fmt)
        if self._use_ingest():
            dev = self._raw_dev.get(fmt)
            if dev is None:
                dev = self._raw_dev[fmt] = make_dev()
            from ._native import XMapsTooMany
            w = as_words(words)

            def push(piece):
                try:
                    dev.push(self.ingest, piece)
                except XMapsTooMany:  # (vector words: up to 12 or 32 events each -- more than a packet slot holds; nothing has advanced)
                    if len(piece) < 2:
                        raise
                    push(piece[:len(piece) // 2])
                    push(piece[len(piece) // 2:])
                    return
                self._deliver_ingest_frames()
            try:
                for a in range(0, len(w), dev.max_words):
                    push(w[a:a + dev.max_words])
            except BaseException:
                self._ingest_failed = True
                raise
            return
        host = self._raw_host.get(fmt)
        if host is None:
            host = self._raw_host[fmt] = make_host()
        evs = host.decode(words)
        if len(evs):
            self.process_events(evs)

    def process_events(self, evs):
        if self._frame_sync == "ext_trigger":
            raise ValueError('frame_sync="ext_trigger": EventCD packets carry no trigger words (process_evt3_words / _evt2_words / _evt21_words do)')
        if self._use_ingest():
            # asynchronous: the frames this packet cuts are delivered by a later call -- at the latest by reset() / close()
            try:
                self.ingest.push(evs)
                self._deliver_ingest_frames()
            except BaseException:
                self._ingest_failed = True
                raise
            return
        pos = evs[evs["p"] == 1]  # PolarityFilterAlgorithm(1), pipe:43,114
        if self.activity_filter is not None:
            pos = self.activity_filter(pos)
        self.trigger_finder.process_events(pos)

    def _record(self, words, st):
        """record_callback as the ingest's record stage calls it: no words (None) for a frame with more than record_max_words"""
        self._record_callback(words if st.n_words <= self._record_kind[1] else None, st)

    # ---- one frame of events -> BGR frame (the hot path) ------------------------------------------------
    def process_ev_frame(self, evs):
        if len(evs) == 0:
            raise ValueError("zero-size array to reduction operation minimum which has no identity")  # xmd:12
        if self._surface_callback is not None:  # (the cut frame's, in front of any frame event filter: as the ingest's stage)
            surfs, _ = self.calib_maps.engine.frames_to_time_surfaces([evs], *self._surface_kind)
            self._surface_callback(surfs[0])
        if self._cloud_callback is not None:  # (the same: a group of one through the group entry, the ingest stage's row limit)
            cloud, _ = self.calib_maps.engine.frames_to_point_clouds([evs])[0]
            self._cloud_callback(cloud[:int(getattr(self.params, "cloud_max_points", 262144))])
        if self._record_callback is not None:  # (the same: a group of one, the ingest stage's all-or-nothing word limit)
            words, st = self.calib_maps.engine.frames_to_evt3_words([evs], use_vectors=self._record_kind[0])
            self._record(words[0], st[0])
        if not isinstance(self.ev_filter_proc.selected_filter(), NoFilter):  # pipe:131-139
            with self.stats_printer.measure_time("frame ev filter"):
                n_before = len(evs)
                xr, _ = self.calib_maps.rectify_cam_coords_i16(evs)
                evs = self.ev_filter_proc.filter_events(evs, xr)
                self.stats_printer.add_metric("frame evs filtered out [%]", 100 - len(evs) / n_before * 100)
        if not self.fused:
            return self._process_ev_frame_staged(evs)
        with self.stats_printer.measure_time("x-maps frame (fused)"):
            _, bgr, st = self.calib_maps.engine.process_events(evs, use_polarity=False, want_depth=False)
        self.stats_printer.add_metric("frame evs filtered out [%]", 0.0)
        self.last_stats = st
        self.frame_callback(bgr)

    def process_ev_frames(self, frames):
        """Offline replay: a list of event frames (what the trigger finder would hand to process_ev_frame one by one) through
        the engine's multi-frame launches, `frame_callback(bgr)` once per frame, in order.  Same frames as calling
        process_ev_frame on each (no frame event filter selected); the kernels of a group keep the chip full, which a single
        frame's launches do not (groups take the column-tile K1)."""
        if not self.fused or not isinstance(self.ev_filter_proc.selected_filter(), NoFilter):
            for evs in frames:
                self.process_ev_frame(evs)
            return
        # an engine of its own with the library's default flags (verified shortcut with automatic redo: the mode in which
        # groups take the column tiles) and enough slots for a group; the per-frame engine declares its frames sorted
        with self.stats_printer.measure_time("x-maps frames (fused, groups)"):
            outs = self._group_engine().process_event_frames(list(frames), want_depth=False)
        for _, bgr in outs:
            self.frame_callback(bgr)

    def depth_frame(self, evs):
        """Same frame as process_ev_frame but returning the f32 depth map (A5 output) instead of calling back."""
        depth, _, st = self.calib_maps.engine.process_events(evs, want_bgr=False)
        self.last_stats = st
        return depth

    def _process_ev_frame_staged(self, evs):
        sp = self.stats_printer
        with sp.measure_time("ev rect"):
            xr, yr = self.calib_maps.rectify_cam_coords_i16(evs)
        with sp.measure_time("x-maps disp"):
            disp, mask = self.x_maps_disp.compute_event_disparity(events=evs, ev_x_rect_i16=xr, ev_y_rect_i16=yr)
        with sp.measure_time("disp map"):
            if self.params.camera_perspective:
                disp_map = self.calib_maps.compute_disp_map_camera_view(events=evs, inlier_mask=mask,
                                                                        ev_disparity_f32=disp)
            else:
                disp_map = self.calib_maps.compute_disp_map_projector_view(
                    ev_x_rect_i16=xr, ev_y_rect_i16=yr, inlier_mask=mask, ev_disparity_f32=disp)
        if not self.params.camera_perspective:
            disp_map = self.disp_to_depth.remap_rectified_disp_map_to_proj(disp_map)
        with sp.measure_time("disp2rgb"):
            depth_map = self.disp_to_depth.colorize_depth_from_disp(disp_map)
        self.frame_callback(depth_map)

    def select_next_frame_event_filter(self):
        new_filter = self.ev_filter_proc.select_next_filter()
        self.stats_printer.log(f"Selected event filter: {new_filter}")

    def reset(self):
        # the frames cut so far belong to the old stream and were shown by now in the reference (its callback is synchronous):
        # deliver them before the stream starts over
        self.flush()
        self.trigger_finder.reset()
        if self._trig is not None:  # (frame_sync = "ext_trigger": the open frame is not a frame; the decoders start a stream)
            self._trig.reset()
            for dev in self._trig_dev.values():
                dev.reset()
        if self.ingest is not None:
            self.ingest.reset()  # (buffered events and the activity filter's history: the stream starts over)
        if self._own_act_filter is not None:
            self._own_act_filter.reset()

    replay_group = 16  # frames per group of process_ev_frames

    def close(self):
        """Delivers the frames the device ingest still holds (every frame cut from the packets pushed so far reaches
        frame_callback: the reference's loop has no flush), then releases everything.  A second call does nothing.  When the
        last frames cannot be had (a launch-side error nobody has seen yet) everything is released all the same and the error is
        raised once, here."""
        if getattr(self, "_closed", False):
            return
        self._closed = True
        try:
            self.flush()  # (before the decoders, the ingest and its result ring go: views are delivered while they are valid)
        finally:
            if getattr(self, "_trig", None) is not None:
                self._trig.close()
                self._trig = None
            for dev in getattr(self, "_trig_dev", {}).values():
                dev.close()
            self._trig_dev = {}
            if getattr(self, "_replay_engine", None) is not None:
                if getattr(self, "_trig_bgr", None):
                    self._replay_engine.dev_free(self._trig_bgr)
                    self._trig_bgr = None
                self._replay_engine.close()
                self._replay_engine = None
            for dev in getattr(self, "_raw_dev", {}).values():  # (before the engine they belong to)
                dev.close()
            self._raw_dev = {}
            if self.ingest is not None:
                self.ingest.close()
            if self._own_act_filter is not None:
                self._own_act_filter.close()
                self._own_act_filter = None
            self.calib_maps.engine.close()
