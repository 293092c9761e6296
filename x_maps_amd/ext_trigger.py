"""Frames cut at a recording's external trigger events (the camera's sync jack wired to the projector: the paper's section 3.4).

A Prophesee recording stores one EXT_TRIGGER word (type 0xA) per pulse of the sync line.  Per encoding (the vendor's published
format description; unpinned against Metavision, like the decoders):

    EVT 3.0  [15:12] = 0xA   [11:8] id   [0] value      the time is the state machine's current TIME_HIGH / TIME_LOW, exactly as for
                                                        a CD event at that word
    EVT 2.0  [31:28] = 0xA   [27:22] t[5:0]   [12:8] id   [0] value      t = (loops << 34) | (time_high << 6) | t[5:0]
    EVT 2.1  [63:60] = 0xA   [59:54] t[5:0]   [44:40] id  [32] value     the same (legacy halves swapped back first)

A trigger word changes no decoder state.  A trigger RECORD (evt3.EXT_TRIGGER_DTYPE; include/xmaps.h: xm_ext_trigger) is
{t, event_index, id, value}: event_index = the number of events the decoder emits for the chunk in front of the word, so a
frame boundary is exact in stream order whatever the stamps are.

    ExtTriggerExtractor      the host form (NumPy, stateful over chunks), beside the host decoders; the device form is
                             DeviceEvtDecoder.set_ext_triggers / last_ext_triggers (csrc/xmaps_exttrigger.hpp)
    insert_ext_triggers      puts trigger words into an encoded stream in front of given events (tests, rendered recordings)
    TriggerFrameCutter       THE CUT RULE of this build (include/xmaps.h states it; csrc/host/xm_trigger_cut.hpp is the same in C++)
    TriggeredFrames          the device-resident buffer the rule cuts from (xm_trigframes): frames as (device records, host offsets);
                             its two filters, both off by default (csrc/xmaps_trigfilter.hpp): the activity filter in front of the
                             cut (set_activity: this build's rule, the ingest's) and the frame event filters on a run of ready
                             frames (set_frame_filter / ready_filtered)
    keep_where               the host form of the buffer's append for an arbitrary keep mask (keep_positive: p == 1)
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import evt2, evt21, evt3
from .evt3 import EXT_TRIGGER_DTYPE
from .synthetic import EVENT_CD_DTYPE

T_EXT_TRIGGER = 0xA
EDGES = {"rising": 0, "falling": 1, "both": 2}  # XM_TRIG_RISING / _FALLING / _BOTH
_U = np.uint64


def _fmt(fmt) -> int:
    f = {3: 3, 2: 2, 21: 21, "3": 3, "2": 2, "21": 21, "3.0": 3, "2.0": 2, "2.1": 21, "evt3": 3, "evt2": 2, "evt21": 21}.get(
        fmt.lower() if isinstance(fmt, str) else fmt)
    if f is None:
        raise ValueError(f"unknown RAW encoding {fmt!r} (3, 2 or 21; DAT carries no trigger words)")
    return f


_DTYPES = {3: "<u2", 2: "<u4", 21: "<u8"}


def trigger_word(fmt, id: int, value: int, t_low6: int = 0) -> int:
    """one EXT_TRIGGER word (EVT 2.1: in the little half order); t_low6 = t & 63, which EVT 3.0 has no field for"""
    f = _fmt(fmt)
    if f == 3:
        return (T_EXT_TRIGGER << 12) | ((id & 0xf) << 8) | (value & 1)
    if f == 2:
        return (T_EXT_TRIGGER << 28) | ((t_low6 & 0x3f) << 22) | ((id & 0x1f) << 8) | (value & 1)
    return (T_EXT_TRIGGER << 60) | ((t_low6 & 0x3f) << 54) | ((id & 0x1f) << 40) | ((value & 1) << 32)


def _popcount32(v: np.ndarray) -> np.ndarray:
    return np.unpackbits(v.astype("<u4").view(np.uint8).reshape(-1, 4), axis=1).sum(axis=1).astype(np.int64)


class ExtTriggerExtractor:
    """The host form: `extract(words)` -> (events, triggers) of one chunk, the decoder's state carried from chunk to chunk.

    Evaluated with the format's host decoder (evt3.Evt3Decoder / evt2.Evt2Decoder / evt21.Evt21Decoder) on the chunk with every
    trigger word replaced by a CD word that changes no state either (EVT 3.0: an EVT_ADDR_X; EVT 2.x: a CD word with the same
    t[5:0]): the marker events carry the triggers' stamps and obey the start-of-stream rule, their places in the event stream are
    the triggers' event_index once the markers in front are taken out."""

    def __init__(self, fmt, wait_for_time_base: bool = False, legacy_halves: bool = False):
        self.fmt = _fmt(fmt)
        self.legacy_halves = bool(legacy_halves) and self.fmt == 21
        self._dec = (evt3.Evt3Decoder(wait_for_time_base) if self.fmt == 3 else evt2.Evt2Decoder(wait_for_time_base) if self.fmt == 2
                     else evt21.Evt21Decoder(wait_for_time_base, legacy_halves))

    def extract(self, words: np.ndarray):
        w = np.ascontiguousarray(words, dtype=_DTYPES[self.fmt])
        if self.fmt == 21 and self.legacy_halves:
            w = evt21.swap_halves(w)
        if len(w) == 0:
            return np.zeros(0, EVENT_CD_DTYPE), np.zeros(0, EXT_TRIGGER_DTYPE)
        if self.fmt == 3:
            typ = (w >> 12).astype(np.int64)
            ident, value = (w >> 8) & 0xf, w & 1
            marker = np.full(len(w), evt3.T_ADDR_X << 12, w.dtype)
            per = np.where(typ == evt3.T_ADDR_X, 1, np.where(typ == evt3.T_VECT_12, _popcount32(w & 0xfff),
                                                              np.where(typ == evt3.T_VECT_8, _popcount32(w & 0xff), 0)))
        elif self.fmt == 2:
            typ = (w >> 28).astype(np.int64)
            ident, value = (w >> 8) & 0x1f, w & 1
            marker = w & np.uint32(0x3f << 22)
            per = (typ <= 1).astype(np.int64)
        else:
            typ = (w >> _U(60)).astype(np.int64)
            ident, value = (w >> _U(40)) & _U(0x1f), (w >> _U(32)) & _U(1)
            marker = (w & _U(0x3f << 54)) | _U(1)
            per = np.where(typ <= 1, _popcount32(w & _U(0xffffffff)), 0)
        is_trig = typ == T_EXT_TRIGGER
        sub = np.where(is_trig, marker, w).astype(w.dtype)
        per = np.where(is_trig, 1, per)
        if self._dec.wait_for_time_base and not self._dec.have_time:  # in front of the stream's first TIME_HIGH: nothing is emitted
            hi = np.nonzero(typ == 0x8)[0]
            per[:hi[0] if len(hi) else len(w)] = 0
        ev = self._dec.decode(evt21.swap_halves(sub) if self.legacy_halves else sub)
        end = np.cumsum(per)
        assert len(ev) == (end[-1] if len(end) else 0)
        tw = np.nonzero(is_trig & (per > 0))[0]  # the emitted triggers' words
        pos = end[tw] - 1                         # ... their markers among the decoded events
        trig = np.zeros(len(tw), EXT_TRIGGER_DTYPE)
        trig["t"] = ev["t"][pos]
        trig["event_index"] = pos - np.arange(len(tw))
        trig["id"], trig["value"] = ident[tw], value[tw]
        keep = np.ones(len(ev), bool)
        keep[pos] = False
        out = np.zeros(int(keep.sum()), EVENT_CD_DTYPE)
        out[:] = ev[keep]
        return out, trig

    def reset(self):
        self.__init__(self.fmt, self._dec.wait_for_time_base, self.legacy_halves)


def _time_words(fmt: int, t: int) -> list:
    """the words that set the decoder's time to t (EVT 2.x: the high field; the trigger word carries t & 63 itself)"""
    if fmt == 3:
        return [(evt3.T_TIME_HIGH << 12) | ((t >> 12) & 0xfff), (evt3.T_TIME_LOW << 12) | (t & 0xfff)]
    if fmt == 2:
        return [(evt2.T_TIME_HIGH << 28) | ((t >> 6) & 0x0fffffff)]
    return [((evt21.T_TIME_HIGH << 28) | ((t >> 6) & 0x0fffffff)) << 32]


def insert_ext_triggers(words, fmt, at_event, id=0, value=1, t=None, legacy_halves: bool = False) -> np.ndarray:
    """An encoded stream with EXT_TRIGGER words in front of the events `at_event` (indices into the stream's decoded events, in
    ascending order; len(events) = behind the last one; equal indices give adjacent trigger words).  id / value / t: scalars or
    one per trigger.  t = None: no time words are added -- the trigger takes the stream's time at that place (EVT 3.0) or the
    high field there and t[5:0] of the event in front of it (EVT 2.x; 0 at the stream's start); otherwise the words that set
    the time to t go in front of the trigger word.

    Built on the encoders: the stream is decoded (host decoder), cut at `at_event`, and every piece encoded on its own with
    encode_evt3 / encode_evt2 / encode_evt21 -- each piece starts with its own time words, so whatever a trigger's time words set
    is put right again.  The events decode unchanged; the word sequence is the encoder's, not the input's."""
    f = _fmt(fmt)
    at = np.atleast_1d(np.asarray(at_event, dtype=np.int64))
    n_t = len(at)
    ids = np.broadcast_to(np.asarray(id, dtype=np.int64), (n_t,))
    vals = np.broadcast_to(np.asarray(value, dtype=np.int64), (n_t,))
    ts = None if t is None else np.broadcast_to(np.asarray(t, dtype=np.int64), (n_t,))
    w = np.ascontiguousarray(words, dtype=_DTYPES[f])
    dec = evt3.Evt3Decoder() if f == 3 else evt2.Evt2Decoder() if f == 2 else evt21.Evt21Decoder(legacy_halves=legacy_halves)
    evs = dec.decode(w)
    if np.any(np.diff(at) < 0) or (n_t and (at[0] < 0 or at[-1] > len(evs))):
        raise ValueError("at_event must be ascending indices into the stream's events (0 .. len(events))")
    enc = evt3.encode_evt3 if f == 3 else evt2.encode_evt2 if f == 2 else evt21.encode_evt21
    out, a = [], 0
    for j in range(n_t):
        b = int(at[j])
        if b > a:
            out += [int(v) for v in enc(evs[a:b])]
            a = b
        if ts is not None:
            out += _time_words(f, int(ts[j]))
            low = int(ts[j]) & 0x3f
        else:
            low = int(evs["t"][b - 1]) & 0x3f if b > 0 else 0
        out.append(trigger_word(f, int(ids[j]), int(vals[j]), low))
    if len(evs) > a:
        out += [int(v) for v in enc(evs[a:])]
    res = np.array(out, dtype=np.uint64).astype(_DTYPES[f])
    return evt21.swap_halves(res) if f == 21 and legacy_halves else res


def keep_where(events: np.ndarray, triggers: np.ndarray, mask):
    """The append of xm_trigframes_push for an arbitrary keep mask (one bool per event of the chunk): (the kept events in stream
    order, the triggers with event_index remapped to "kept events with chunk index < event_index")"""
    keep = np.asarray(mask, dtype=bool)
    if keep.shape != (len(events),):
        raise ValueError("one keep flag per event of the chunk")
    before = np.concatenate(([0], np.cumsum(keep)))
    out = triggers.copy()
    out["event_index"] = before[np.minimum(triggers["event_index"].astype(np.int64), len(events))]
    kept = np.zeros(int(keep.sum()), EVENT_CD_DTYPE)
    kept[:] = events[keep]
    return kept, out


def keep_positive(events: np.ndarray, triggers: np.ndarray):
    """PolarityFilterAlgorithm(1) on a chunk and its triggers: keep_where(p == 1) -- what xm_trigframes_push does with
    positive_only (and no activity filter)"""
    return keep_where(events, triggers, events["p"] == 1)


class TriggerFrameCutter:
    """The cut rule (include/xmaps.h, "THE CUT RULE of this build"), the mirror of csrc/host/xm_trigger_cut.hpp on a NumPy buffer of
    cap_events records: push(kept events of a chunk, its triggers in kept records) -> ready() -> release(n).

    A trigger is selected when (id < 0 or its id matches) and its value matches the edge; frame k = the kept events between the
    k-th and the next selected trigger, nothing trimmed; events in front of the first selected trigger belong to no frame;
    min_events > 0 skips frames with n <= min_events; an open frame that cannot keep its events plus the next chunk's inside
    cap_events is dropped and cutting resumes at the next selected trigger."""

    COUNTERS = ("events_in", "events_kept", "triggers_seen", "triggers_selected", "frames_cut", "frames_skipped",
                "events_before_first_trigger", "events_dropped_open_frame", "front_moves")

    def __init__(self, cap_events: int = 1 << 22, id: int = -1, edge: str = "rising", min_events: int = 0, max_frames_ready: int = 0):
        if edge not in EDGES:
            raise ValueError('edge must be "rising", "falling" or "both"')
        self.cap_events, self.id, self.edge = int(cap_events), int(id), edge
        self.min_events, self.max_frames_ready = int(min_events), int(max_frames_ready)
        self.buf = np.zeros(self.cap_events, EVENT_CD_DTYPE)
        self.stats = dict.fromkeys(self.COUNTERS, 0)
        self.reset()

    def reset(self):
        self.stream_pos = self.lo = self.hi = self.open_pos = 0
        self.open = self.dropping = False
        self.open_trig = None
        self.frames = []  # ready: [begin, end, opening trigger]

    def selected(self, trig) -> bool:
        if self.id >= 0 and int(trig["id"]) != self.id:
            return False
        return self.edge == "both" or int(trig["value"]) == (1 if self.edge == "rising" else 0)

    def _trim(self):
        if not self.open:
            self.hi = self.frames[-1][1] if self.frames else 0
        self.lo = self.frames[0][0] if self.frames else self.open_pos if self.open else 0
        if not self.frames and not self.open:
            self.lo = self.hi = 0

    def _room(self, n_in: int) -> int:
        st = self.stats
        if self.hi + n_in <= self.cap_events:
            return self.hi
        if self.hi - self.lo + n_in > self.cap_events and self.open:
            st["events_dropped_open_frame"] += self.hi - self.open_pos
            self.hi, self.open, self.dropping = self.open_pos, False, True
            self._trim()
        if self.hi - self.lo + n_in > self.cap_events:
            raise ValueError(f"{len(self.frames)} ready frames leave no room for a chunk of {n_in} events (release them first)")
        if self.hi + n_in > self.cap_events:
            lo, n = self.lo, self.hi - self.lo
            self.buf[:n] = self.buf[lo:lo + n].copy()
            for f in self.frames:
                f[0] -= lo
                f[1] -= lo
            if self.open:
                self.open_pos -= lo
            self.hi, self.lo = n, 0
            st["front_moves"] += 1
        return self.hi

    def push(self, events: np.ndarray, triggers: np.ndarray, n_in: int | None = None) -> int:
        """events: the chunk's KEPT events; triggers: its records, event_index in kept events; n_in: the chunk's decoded events
        (what room is asked for; default len(events)).  Returns the number of ready frames."""
        n_kept = len(events)
        n_in = n_kept if n_in is None else int(n_in)
        st = self.stats
        if n_in > self.cap_events:
            raise ValueError(f"the chunk decodes to {n_in} events, the buffer holds {self.cap_events}")
        base = self._room(n_in)
        self.buf[base:base + n_kept] = events
        st["events_in"] += n_in
        st["events_kept"] += n_kept
        cursor = 0
        for tr in triggers:
            st["triggers_seen"] += 1
            if not self.selected(tr):
                continue
            st["triggers_selected"] += 1
            idx = min(int(tr["event_index"]), n_kept)
            if self.open:
                n = base + idx - self.open_pos
                if self.min_events > 0 and n <= self.min_events:
                    st["frames_skipped"] += 1
                else:
                    self.frames.append([self.open_pos, base + idx, self.open_trig])
                    st["frames_cut"] += 1
            else:
                st["events_dropped_open_frame" if self.dropping else "events_before_first_trigger"] += idx - cursor
            self.open, self.dropping = True, False
            self.open_pos, self.open_trig, cursor = base + idx, tr.copy(), idx
        if not self.open:
            st["events_dropped_open_frame" if self.dropping else "events_before_first_trigger"] += n_kept - cursor
        self.hi = base + n_kept
        self.stream_pos += n_kept
        self._trim()
        return len(self.frames)

    def run(self, cap_frames: int = 1 << 30) -> int:
        """the length of the next run of ready frames that lie back to back (a skipped frame ends a run)"""
        lim = min(cap_frames, self.max_frames_ready) if self.max_frames_ready > 0 else cap_frames
        n = 0
        while n < lim and n < len(self.frames) and (n == 0 or self.frames[n][0] == self.frames[n - 1][1]):
            n += 1
        return n

    def ready(self, cap_frames: int = 1 << 30):
        """-> [(events, opening trigger)] of the next run (copies); release(n) when done"""
        out = []
        for b, e, tr in self.frames[:self.run(cap_frames)]:
            ev = np.zeros(e - b, EVENT_CD_DTYPE)
            ev[:] = self.buf[b:e]
            out.append((ev, tr))
        return out

    def release(self, n: int):
        if n < 0 or n > len(self.frames):
            raise ValueError(f"{n} frames to release, {len(self.frames)} are ready")
        del self.frames[:n]
        self._trim()

    def cut_all(self, chunks):
        """convenience: [(events, triggers)] chunks -> every frame, released as they come (the oracle of the tests)"""
        out = []
        for ev, tr in chunks:
            self.push(ev, tr)
            while True:
                got = self.ready()
                if not got:
                    break
                out += got
                self.release(len(got))
        return out


class TriggeredFrames:
    """xm_trigframes: the device-resident buffer the cut rule works on.

        dec.set_ext_triggers(4096)
        tf = TriggeredFrames(engine, cap_events=1 << 22, min_events=1000, positive_only=True)
        n_ready = tf.push(dec, words)                  # decode + append (+ p == 1 compaction) + cut; synchronous
        ptr, offsets, opening = tf.ready(16)           # device base pointer, len(frames) + 1 host offsets, opening triggers
        engine.process_events_batch_device(ptr, offsets, None, d_bgr); engine.sync()
        tf.release(len(offsets) - 1)
    """

    created = 0  # objects made in this process (the pipe's default mode makes none)

    FILTER_COUNTERS = ("events_positive", "events_active", "chunks_sequential", "frames_filtered", "events_after_frame_filter",
                       "index_errors")

    def __init__(self, engine, cap_events: int = 1 << 22, id: int = -1, edge: str = "rising", min_events: int = 0,
                 positive_only: bool = False, max_frames_ready: int = 0, activity_thresh_us=None, activity_include_self: bool = False):
        from . import _native as N
        if edge not in EDGES:
            raise ValueError('edge must be "rising", "falling" or "both"')
        self._N, self._e, self._lib = N, engine, engine._lib
        cfg = N.xm_trigframes_config(C.sizeof(N.xm_trigframes_config), int(id), EDGES[edge], int(bool(positive_only)), int(cap_events),
                                     int(min_events), int(max_frames_ready), 0)
        self._tf = C.c_void_p(None)
        N.check(self._lib.xm_trigframes_create(engine._h, C.byref(cfg), C.byref(self._tf)))
        TriggeredFrames.created += 1
        if activity_thresh_us is not None:
            try:
                self.set_activity(activity_thresh_us, activity_include_self)
            except Exception:
                self.close()
                raise

    def set_activity(self, thresh_us, include_self: bool = False):
        """The activity filter as a stage of push (this build's rule, the ingest's: oracle/ingest_oracle.py), from the next chunk on;
        thresh_us None or < 0: off.  Needs positive_only; switching it on starts from an empty history."""
        self._N.check(self._lib.xm_trigframes_set_activity(self._tf, -1 if thresh_us is None else int(thresh_us), int(bool(include_self))))

    def set_frame_filter(self, filter_id: int, intended_semantics: bool = False, max_frames: int = 16):
        """The frame event filter ready_filtered applies (0: none; frame_event_filter's filter_id numbers), on runs of at most
        max_frames frames.  ValueError (nothing changes): an unknown filter, FirstEventPerYT on a rig whose cell map is too large."""
        self._N.check(self._lib.xm_trigframes_set_frame_filter(self._tf, int(filter_id), int(bool(intended_semantics)), int(max_frames)))

    def ready_filtered(self, cap_frames: int = 64):
        """ready()'s run with each frame replaced by what the selected filter hands on -> (device pointer of the survivors buffer,
        offsets uint64 [n + 1] from 0, opening triggers [n], n_index_errors uint64 [n]); no filter selected: ready()'s values"""
        ptr, n = C.c_void_p(None), C.c_int(0)
        offs = np.zeros(cap_frames + 1, np.uint64)
        opening = np.zeros(cap_frames, EXT_TRIGGER_DTYPE)
        bad = np.zeros(cap_frames, np.uint64)
        self._N.check(self._lib.xm_trigframes_ready_filtered(self._tf, C.byref(ptr), C.c_void_p(offs.ctypes.data), int(cap_frames), C.byref(n),
                                                             C.c_void_p(opening.ctypes.data), C.c_void_p(bad.ctypes.data)))
        return int(ptr.value or 0), offs[:n.value + 1].copy(), opening[:n.value].copy(), bad[:n.value].copy()

    def filter_stats(self) -> dict:
        st = self._N.xm_trigframes_filter_counters()
        self._N.check(self._lib.xm_trigframes_filter_stats(self._tf, C.byref(st)))
        return {k: int(getattr(st, k)) for k in self.FILTER_COUNTERS}

    def close(self):
        if getattr(self, "_tf", None) is not None and self._tf.value:
            self._lib.xm_trigframes_destroy(self._tf)
            self._tf = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def reset(self):
        self._N.check(self._lib.xm_trigframes_reset(self._tf))

    def push(self, decoder, words, pinned: bool = False) -> int:
        w = decoder._as_words(words)
        n = C.c_int(0)
        self._N.check(self._lib.xm_trigframes_push(self._tf, decoder._d, C.c_void_p(w.ctypes.data), len(w), int(bool(pinned)), C.byref(n)))
        return int(n.value)

    def ready(self, cap_frames: int = 64):
        """-> (device pointer of the buffer, offsets uint64 [n + 1], opening triggers [n]); n = 0: offsets has one element"""
        ptr, n = C.c_void_p(None), C.c_int(0)
        offs = np.zeros(cap_frames + 1, np.uint64)
        opening = np.zeros(cap_frames, EXT_TRIGGER_DTYPE)
        self._N.check(self._lib.xm_trigframes_ready(self._tf, C.byref(ptr), C.c_void_p(offs.ctypes.data), int(cap_frames), C.byref(n),
                                                    C.c_void_p(opening.ctypes.data)))
        return int(ptr.value or 0), offs[:n.value + 1].copy(), opening[:n.value].copy()

    def release(self, n_frames: int):
        self._N.check(self._lib.xm_trigframes_release(self._tf, int(n_frames)))

    def stats(self) -> dict:
        st = self._N.xm_trigframes_counters()
        self._N.check(self._lib.xm_trigframes_stats(self._tf, C.byref(st)))
        return {k: int(getattr(st, k)) for k in TriggerFrameCutter.COUNTERS}

    def download(self, ptr: int, offsets) -> list:
        """the records of the frames ready() named, as host arrays (tests, the frame event filters' host path)"""
        out = []
        for a, b in zip(offsets[:-1], offsets[1:]):
            ev = np.zeros(int(b) - int(a), EVENT_CD_DTYPE)
            if len(ev):
                self._e.dev_download(ev, ptr + 16 * int(a))
            out.append(ev)
        return out
