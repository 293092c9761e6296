"""RuntimeParams / DepthReprojectionProcessor with the reference's interface
(python/depth_reprojection_processor.py:13-36, 50-114):

    with DepthReprojectionProcessor(params) as proc:
        for evs in event_packets:
            proc.process_events(evs)
            if proc.should_close(): break

The window is pluggable; without Metavision's MTWindow the reference's own FakeWindow behaviour is used
(processor.py:39-47).  Frames reach `window.show_async(bgr)` exactly as in the reference.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, Callable, Optional

from .depth_reprojection_pipe import DepthReprojectionPipe
from .stats import StatsPrinter


@dataclass
class RuntimeParams:
    camera_width: int
    camera_height: int

    projector_width: int
    projector_height: int

    projector_fps: int

    z_near: float
    z_far: float

    calib: Any  # path of the exported tables (.npz); the reference takes the calibration YAML here

    projector_time_map: Optional[str] = None

    no_frame_dropping: bool = True

    camera_perspective: bool = False

    # additions of this build (defaults keep the reference's positional signature valid)
    tables: Optional[dict] = None  # pre-built tables instead of `calib`
    device: int = 0
    # polarity / activity filter + buffering + frame segmentation on the GPU (x_maps_amd/ingest.py): process_events(packet) stages
    # the packet and returns, the frames are cut and processed on the device and handed to frame_callback as the consumer's own
    # arrays (the pinned buffers their DMA filled).  THE DEFAULT since round 6 -- the same frames as the host chain, which stays
    # as the opt-out (False: NumPy polarity mask + one GPU call per packet for the activity filter + the NumPy trigger finder,
    # 20 x slower) and takes over by itself while a frame event filter (key E) or a caller-supplied activity filter is selected.
    # DELIVERY: a frame reaches frame_callback from a later process_events call than the one that cut it, at the latest from
    # reset() / close() / the end of the `with` block; same frames, same order, none lost (with no_frame_dropping: whatever the
    # packets' sizes and ingest_result_ring).  flush() only brings them forward.
    device_ingest: bool = True
    # The activity-noise filter behind the polarity filter, on every packet, as the reference runs it unconditionally
    # (depth_reprojection_pipe.py:65-67,116-117): kernels of the device ingest, or one GPU call per packet in front of the host's
    # trigger finder.  The rule is this build's own definition (Metavision's is a binary: oracle/ingest_oracle.py); False
    # switches the stage off (round 4's default).
    activity_filter: bool = True
    # the two variants of that rule a fixture of Metavision's filter (tools/pin_thirdparty.py) may call for, as configuration:
    # a strict comparison t - t' < T (= threshold T - 1 on integer stamps) and a 3 x 3 window that includes the event's own pixel
    activity_strict: bool = False
    activity_include_self: bool = False
    # device ingest only: hand frame_callback / window.show_async a VIEW into the ingest's ring of pinned result buffers instead of
    # an array of the consumer's own.  LIFETIME of such a view: until `ingest_result_ring` - 1 further frames have been produced.
    # (Since round 6 the default frames cost no host copy either -- xm_ingest_poll_owned --, so views only save the pool.)
    ingest_frame_views: bool = False
    ingest_result_ring: int = 16
    # device ingest only: a frame event filter (key E) runs as a stage of the ingest, on the device between the cut and the frame
    # kernels (DeviceIngest.set_frame_filter), instead of moving the stream to the host chain while it is selected.  Same frames;
    # nothing is reset at the switch (the reference does not reset either).  Off by default: the pipe behaves as before.  A filter
    # the ingest refuses (FirstEventPerYT on a rig whose cell map would be too large) still takes the host chain, and says so.
    device_frame_filters: bool = False
    # process_evt3_words / process_evt2_words: events in front of a recording's first EVT_TIME_HIGH word are dropped (a reader that
    # waits for the first time base) instead of emitted at time base 0.  Which of the two Metavision's reader does is unpinned
    # (tools/pin_thirdparty.py decides); it matters for the first few words of a file only.
    raw_wait_for_time_base: bool = False
    # process_evt21_words: the recording stores every 64-bit word as two 32-bit halves with the HIGH half first ("endianness=legacy"
    # in its header's format line: x_maps_amd.evt21.raw_legacy_halves); the decoders put the halves back where they load a word.
    raw_legacy_halves: bool = False
    # `calib` is a calibration YAML: its rectification maps, the rectified time map and the X-map are built in one device call
    # (calibration.build_tables(maps_on_device=True), x_maps_amd/rig_maps.py) instead of NumPy on the host.  The same tables,
    # bit for bit.
    tables_on_device: bool = False
    # surface_callback(surface) for every shown frame, immediately before that frame's frame_callback: the frame's camera time
    # surface (float32 [camera_height][camera_width]; per pixel the stamp of the frame's last event there as t - the frame's first
    # stamp + 1, 0 = no event: XMapsEngine.frames_to_time_surfaces), built from the CUT frame, in front of any frame event filter.
    # On the device ingest it is a stage of the ingest (DeviceIngest.set_surface_output); on the host chain one call of the
    # group entry on the frame's events.  The same arrays either way.  What the evaluation entries take as `scans_np`.
    surface_callback: Optional[Callable] = None
    # which event of a pixel stamps the surface ("last" or "first") and the surface's dtype (float32 or float64): the time-map
    # calibration (tools/calibrate_time_map.py) takes first events in float64
    surface_select: str = "last"
    surface_dtype: Any = "float32"
    # cloud_callback(cloud) for every shown frame, immediately before that frame's frame_callback (behind its surface_callback,
    # if both are set): the frame's per-event point cloud (float32 [n][3]: the reference's construct_point_cloud on the frame's
    # inlier events in stream order, XMapsEngine.frames_to_point_clouds), built from the CUT frame, in front of any frame event
    # filter; at most cloud_max_points rows, the frame's first.  On the device ingest it is a stage of the ingest
    # (DeviceIngest.set_cloud_output); on the host chain one call of the group entry on the frame's events.  The same arrays
    # either way.  Needs tables with cam_mapx_f32, cam_mapy_f32 and Q (ValueError at construction otherwise).
    cloud_callback: Optional[Callable] = None
    cloud_max_points: int = 262144
    # record_callback(words, stats) for every shown frame, immediately before that frame's frame_callback (behind its surface and
    # cloud callbacks): the frame's EVT 3.0 words (uint16: evt3.encode_evt3(frame, record_use_vectors), the encoder's state fresh
    # for the frame, XMapsEngine.frames_to_evt3_words) and its Evt3RecordStats, built from the CUT frame -- behind the polarity and
    # activity filters, in front of any frame event filter.  A frame with more than record_max_words words comes with words None
    # (all or nothing; stats.n_words is the true count).  On the device ingest it is a stage of the ingest
    # (DeviceIngest.set_record_output); on the host chain, and on the ext_trigger chain, one call of the group entry on the frame's
    # events or device records.  The same arrays either way.  evt3.FrameRecordingWriter turns the calls into a .raw file that
    # frame_sync="ext_trigger" replays to the same frames.
    record_callback: Optional[Callable] = None
    record_use_vectors: bool = True
    record_max_words: int = 1 << 21
    # How the stream is cut into projector frames.  "pauses" (the default; nothing changes): the reference's software trigger finder,
    # on the device ingest or the host chain.  "ext_trigger": at the recording's EXT_TRIGGER words -- the pulses of the camera's
    # sync jack, for rigs whose projector is wired to it (the paper's section 3.4; x_maps_amd/ext_trigger.py).  Only
    # process_evt3_words / _evt2_words / _evt21_words carry those words: process_events and process_dat_records raise ValueError
    # in this mode.  Frame k = the positive events (PolarityFilterAlgorithm(1)) between the k-th and the next selected trigger,
    # nothing trimmed; frames of MIN_EVENTS_PER_FRAME = 1000 events or fewer are skipped, as the reference's trigger finder skips
    # them.  The activity filter is a stage of this chain when ext_trigger_activity_filter is set (below); without it the chain
    # has none and activity_filter is ignored, as before.  DELIVERY is synchronous, as in the
    # reference: a frame reaches frame_callback (its surface_callback and cloud_callback in front) inside the call whose words hold
    # its closing trigger.  While a frame event filter (key E) is selected every frame is downloaded and goes through
    # process_ev_frame -- or, with device_frame_filters, is filtered where it lies (TriggeredFrames.ready_filtered: the run's
    # surfaces and clouds from the cut frames, its launches on the survivors; the same frames).
    # ext_trigger_id: the trigger channel (-1: any); ext_trigger_edge: "rising", "falling" or "both";
    # ext_trigger_cap_events: the device buffer the frames are cut from, in events -- an open frame that cannot keep its events
    # plus one more chunk's inside it is dropped (counted; cutting resumes at the next trigger).
    frame_sync: str = "pauses"
    ext_trigger_id: int = -1
    ext_trigger_edge: str = "rising"
    ext_trigger_cap_events: int = 1 << 22
    # frame_sync = "ext_trigger" only: polarity filter -> ACTIVITY FILTER -> cut, what the reference's pipe does to every packet
    # (pipe:110-119), on the device inside the append.  False (the default) is the chain as it was: no activity filter.  True:
    # activity_filter, activity_strict, activity_include_self and int(1e6 / projector_fps) apply to this chain as they do to the
    # ingest (this build's rule; unpinned against Metavision, like the ingest's), and MIN_EVENTS_PER_FRAME applies to the filtered
    # frames.
    ext_trigger_activity_filter: bool = False

    @property
    def should_drop_frames(self):
        return not self.no_frame_dropping


def _enum_name(v) -> str:
    """'KEY_E' for UIKeyEvent.KEY_E, 'RELEASE' for UIAction.RELEASE, 'E' for "e", '69' for 69"""
    name = getattr(v, "name", None)
    if isinstance(name, str):
        return name.upper()
    return str(v).rsplit(".", 1)[-1].upper()


class FakeWindow:
    """Headless window: keeps the last frame so callers/tests can look at it."""

    def __init__(self):
        self.last_frame = None
        self.frames_shown = 0
        self._close = False

    def should_close(self):
        return self._close

    def set_close_flag(self):
        self._close = True

    def show_async(self, img):
        self.last_frame = img
        self.frames_shown += 1

    def set_keyboard_callback(self, cb):
        pass


@dataclass
class DepthReprojectionProcessor:
    params: RuntimeParams
    stats_printer: StatsPrinter = field(default_factory=StatsPrinter)
    window: Any = None  # anything with should_close() / show_async(img); default FakeWindow

    _pipe: DepthReprojectionPipe = field(init=False, default=None)
    _window: Any = field(init=False, default=None)

    def should_close(self):
        return self._window.should_close()

    def show_async(self, depth_map):
        self._window.show_async(depth_map)
        self.stats_printer.count("frames shown")

    def __enter__(self):
        self._pipe = DepthReprojectionPipe(params=self.params, stats_printer=self.stats_printer,
                                           frame_callback=self.show_async)
        self._window = self.window if self.window is not None else FakeWindow()
        if hasattr(self._window, "set_keyboard_callback"):
            self._window.set_keyboard_callback(self.keyboard_cb)
        return self

    def __exit__(self, exc_type=None, exc=None, tb=None):
        # The reference's loop has no flush(): the frames the device ingest still holds are delivered here, before the statistics
        # are printed ("frames shown" counts them).  An error of that last delivery is raised once everything is released --
        # unless an exception is leaving the block already: that one goes on, this one is logged.
        err = None
        try:
            self._pipe.flush()
        except Exception as e:
            err = e
        try:
            self.stats_printer.print_stats()
        finally:
            try:
                self._pipe.close()
            except Exception as e:
                err = err or e
        if err is not None:
            if exc_type is None:
                raise err
            self.stats_printer.log(f"the last frames were not delivered: {err!r}")
        return False

    def keyboard_cb(self, key, scancode=None, action=None, mods=None):
        """Window key callback with Metavision's signature (key, scancode, action, mods), processor.py:96-105: acts on key
        RELEASE only; Q / Escape close, E selects the next frame event filter, S silences the statistics.  `key` / `action` may be
        metavision_sdk_ui's UIKeyEvent / UIAction enum members (compared by name, so the SDK need not be importable here), GLFW
        integers, or plain strings; a caller that passes no action (tests, a headless driver) means "released"."""
        if action is not None and _enum_name(action) not in ("RELEASE", "0"):  # (GLFW_RELEASE == 0)
            return
        k = _enum_name(key)
        if k in ("KEY_ESCAPE", "ESCAPE", "ESC", "256", "KEY_Q", "Q", "81"):
            self._window.set_close_flag()
        elif k in ("KEY_E", "E", "69"):
            self._pipe.select_next_frame_event_filter()
        elif k in ("KEY_S", "S", "83"):
            self.stats_printer.toggle_silence()

    def process_events(self, evs):
        self.stats_printer.print_stats_if_needed()
        self.stats_printer.count("processed evs", len(evs))
        self._pipe.process_events(evs)
        self.stats_printer.print_stats_if_needed()

    def process_evt3_words(self, words):
        """A chunk of a recording's EVT 3.0 words (x_maps_amd.evt3.read_raw_words) instead of an EventCD packet; with
        the device ingest (RuntimeParams.device_ingest, the default) the words are decoded on the device in front of it."""
        self.stats_printer.print_stats_if_needed()
        self._pipe.process_evt3_words(words)
        self.stats_printer.print_stats_if_needed()

    def process_evt2_words(self, words):
        """the same for a chunk of EVT 2.0 words (x_maps_amd.evt2.read_raw_words)"""
        self.stats_printer.print_stats_if_needed()
        self._pipe.process_evt2_words(words)
        self.stats_printer.print_stats_if_needed()

    def process_evt21_words(self, words):
        """the same for a chunk of EVT 2.1 words (x_maps_amd.evt21.read_raw_words; RuntimeParams.raw_legacy_halves: their half order)"""
        self.stats_printer.print_stats_if_needed()
        self._pipe.process_evt21_words(words)
        self.stats_printer.print_stats_if_needed()

    def process_dat_records(self, records):
        """the same for a chunk of a DAT file's records (x_maps_amd.dat.read_raw_words)"""
        self.stats_printer.print_stats_if_needed()
        self._pipe.process_dat_records(records)
        self.stats_printer.print_stats_if_needed()

    def flush(self):
        """Device ingest: wait for the packets pushed so far and deliver the frames they produced now.  Optional: reset() and
        leaving the `with` block deliver them too, no frame is lost without it."""
        self._pipe.flush()

    def reset(self):
        self._pipe.reset()
