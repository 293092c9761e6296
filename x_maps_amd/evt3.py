"""Prophesee EVT 3.0 RAW decoder ("next" row N4): the reader in front of the pipe, without the Metavision SDK.

The reference reads its recordings through Metavision's closed readers (python/bias_events_iterator.py:53-96:
RawReaderBase(input_filename, delta_t).load_delta_t(-1) yields EventCD packets).  EVT 3.0 itself is a public, documented
format: an ASCII header (lines starting with '%'), then little-endian 16-bit words whose top 4 bits are the type:

    0x0 EVT_ADDR_Y    y[10:0]                          (bit 11: camera id)      sets the current row
    0x2 EVT_ADDR_X    x[10:0], polarity bit 11                                  ONE event at (x, current y, current t)
    0x3 VECT_BASE_X   x[10:0], polarity bit 11                                  base column + polarity of the vectors below
    0x4 VECT_12       12 valid bits                                             events at base + i for every set bit; base += 12
    0x5 VECT_8        8 valid bits                                              same with 8; base += 8
    0x6 EVT_TIME_LOW  t[11:0]          0x8 EVT_TIME_HIGH  t[23:12]              current time (us), 24 bits, wraps every 16.8 s
    0xA EXT_TRIGGER, 0xE OTHERS, 0x7 / 0xF CONTINUED                            skipped here

The decoder is a state machine over the words; `decode_evt3` evaluates it for a whole buffer at once with forward fills
(np.maximum.accumulate of "index of the last word of type T") -- the same shape a device kernel would have (scan + gather).
PARITY: unpinned against Metavision (closed, and no recording ships with the reference); pinned by a round trip through the
encoder below and by hand-built word sequences (tests/test_evt3.py).
"""
from __future__ import annotations

import numpy as np

from .synthetic import EVENT_CD_DTYPE

T_ADDR_Y, T_ADDR_X, T_VECT_BASE_X, T_VECT_12, T_VECT_8, T_TIME_LOW, T_TIME_HIGH = 0x0, 0x2, 0x3, 0x4, 0x5, 0x6, 0x8
_FORMAT_NAMES = ("3.0", "3", "EVT3", "EVT3.0")
# one EXT_TRIGGER word as a record (include/xmaps.h: xm_ext_trigger; ext_trigger.py)
EXT_TRIGGER_DTYPE = np.dtype({"names": ["t", "event_index", "id", "value", "reserved"], "formats": ["<i8", "<u4", "u1", "u1", "<u2"],
                              "offsets": [0, 8, 12, 13, 14], "itemsize": 16})


def split_raw_header(blob: bytes) -> tuple[dict, int]:
    """ASCII header of a .raw file: lines '% key value'; returns (fields, offset of the first data byte)."""
    off, fields = 0, {}
    while off < len(blob) and blob[off:off + 1] == b"%":
        end = blob.find(b"\n", off)
        if end < 0:
            break
        line = blob[off + 1:end].decode("ascii", "replace").strip()
        off = end + 1
        if line == "end":
            break
        k, _, v = line.partition(" ")
        fields[k] = v
    return fields, off


def raw_format(fields: dict, default: str = "") -> str:
    """The encoding a RAW header names: "% evt 3.0" (older headers) or "% format EVT3;height=720;width=1280" (newer ones): the
    first token decides."""
    return fields.get("evt", fields.get("format", default)).split(";")[0].strip().upper()


def read_raw_chunks(path: str, names: tuple, dtype: str, chunk_words: int, default: str = ""):
    """Yields the words of a .raw file chunk by chunk, undecoded, once its header names one of `names` as the encoding (a header
    that names none counts as `default`): the header check and the word view of both encodings' readers."""
    with open(path, "rb") as f:
        blob = f.read()
    fields, off = split_raw_header(blob)
    if raw_format(fields, default) not in names:
        raise ValueError(f"{path}: not an EVT {names[0]} file (header says {fields.get('evt', fields.get('format'))!r})")
    words = np.frombuffer(blob, dtype=dtype, offset=off, count=(len(blob) - off) // np.dtype(dtype).itemsize)
    for a in range(0, len(words), chunk_words):
        yield words[a:a + chunk_words]


def _ffill_index(mask: np.ndarray) -> np.ndarray:
    """index of the last True at or before each position (-1 if none)"""
    idx = np.where(mask, np.arange(len(mask)), -1)
    return np.maximum.accumulate(idx)


class Evt3Decoder:
    """Streaming decoder: feed chunks of words, get EventCD arrays; state (row, base column, time, overflow count) carries over."""

    def __init__(self, wait_for_time_base: bool = False):
        self.y = 0
        self.base_x = 0
        self.base_p = 0
        self.t_low = 0
        self.t_high = 0
        self.t_loops = 0  # number of 24-bit wrap-arounds seen
        # start-of-stream rule: True = events in front of the stream's first EVT_TIME_HIGH word are not emitted (a reader that waits
        # for the first time base); False (default) = they carry the initial time base 0.  Unpinned against Metavision.
        self.wait_for_time_base = bool(wait_for_time_base)
        self.have_time = False  # an EVT_TIME_HIGH word has been read

    def decode(self, words: np.ndarray) -> np.ndarray:
        w = np.ascontiguousarray(words, dtype="<u2").astype(np.int64)
        n = len(w)
        if n == 0:
            return np.zeros(0, EVENT_CD_DTYPE)
        typ = w >> 12
        pos = np.arange(n)
        # ---- time: last TIME_HIGH / TIME_LOW before each word; 24-bit wrap-arounds counted on the TIME_HIGH sequence ----
        ih, il = _ffill_index(typ == T_TIME_HIGH), _ffill_index(typ == T_TIME_LOW)
        hi_words = np.nonzero(typ == T_TIME_HIGH)[0]
        th_seq = w[hi_words] & 0xfff
        prev = np.concatenate(([self.t_high], th_seq[:-1])) if len(th_seq) else th_seq
        # a wrap: the 12-bit high field falls back by (much) more than jitter would explain
        wraps = np.cumsum((prev - th_seq) > 0x800) if len(th_seq) else np.zeros(0, np.int64)
        loops_at = np.full(n, self.t_loops, np.int64)
        if len(hi_words):
            loops_at = np.where(ih >= 0, self.t_loops + wraps[np.searchsorted(hi_words, np.maximum(ih, 0))], self.t_loops)
        t_high = np.where(ih >= 0, w[np.maximum(ih, 0)] & 0xfff, self.t_high)
        t_low = np.where(il >= 0, w[np.maximum(il, 0)] & 0xfff, self.t_low)
        if len(hi_words):
            # a TIME_HIGH word that CHANGES the high field restarts the low field at 0 until the next TIME_LOW word (the stale
            # low would put the stamp up to 4095 us too late, and stamps must not run backwards when the TIME_LOW arrives);
            # the redundant TIME_HIGH words that repeat the current value change nothing
            changed = np.concatenate(([th_seq[0] != self.t_high], th_seq[1:] != th_seq[:-1]))
            last_change = _ffill_index(np.isin(pos, hi_words[changed]))
            t_low = np.where(last_change > il, 0, t_low)
        t = (loops_at << 24) | (t_high << 12) | t_low
        # ---- row: last ADDR_Y ----
        iy = _ffill_index(typ == T_ADDR_Y)
        y = np.where(iy >= 0, w[np.maximum(iy, 0)] & 0x7ff, self.y)
        # ---- single events ----
        sx = np.nonzero(typ == T_ADDR_X)[0]
        # ---- vector events: base column of each VECT word = last VECT_BASE_X + what earlier VECT words since it consumed ----
        adv = np.where(typ == T_VECT_12, 12, np.where(typ == T_VECT_8, 8, 0))
        cum = np.cumsum(adv)
        ib = _ffill_index(typ == T_VECT_BASE_X)
        base = np.where(ib >= 0, w[np.maximum(ib, 0)] & 0x7ff, self.base_x)
        pol = np.where(ib >= 0, (w[np.maximum(ib, 0)] >> 11) & 1, self.base_p)
        cum_at_base = np.where(ib >= 0, cum[np.maximum(ib, 0)], 0)
        vbase = base + (cum - adv - cum_at_base)
        vw = np.nonzero(adv > 0)[0]
        bits = (w[vw, None] >> np.arange(12)[None, :]) & 1
        bits[typ[vw] == T_VECT_8, 8:] = 0
        vr, vb = np.nonzero(bits)
        vi = vw[vr]
        # ---- merge in word order (a vector word's events in ascending column order) ----
        n_ev = len(sx) + len(vi)
        out = np.zeros(n_ev, EVENT_CD_DTYPE)
        order_key = np.concatenate((sx * 16, vi * 16 + vb))
        order = np.argsort(order_key, kind="stable")
        xs = np.concatenate((w[sx] & 0x7ff, vbase[vi] + vb))[order]
        ys = np.concatenate((y[sx], y[vi]))[order]
        ps = np.concatenate(((w[sx] >> 11) & 1, pol[vi]))[order]
        ts = np.concatenate((t[sx], t[vi]))[order]
        out["x"], out["y"], out["p"], out["t"] = xs, ys, ps, ts
        if self.wait_for_time_base and not self.have_time:
            src = np.concatenate((sx, vi))[order]            # the word each event came from
            out = out[ih[src] >= 0]                           # ... has a TIME_HIGH word at or before it in this chunk
        self.have_time = self.have_time or len(hi_words) > 0
        # ---- carry the state over to the next chunk ----
        self.y = int(y[-1])
        self.t_high, self.t_low = int(t_high[-1]), int(t_low[-1])
        self.t_loops = int(loops_at[-1])
        if ib[-1] >= 0 or len(vw):
            self.base_x = int(base[-1] + (cum[-1] - cum_at_base[-1]))
            self.base_p = int(pol[-1])
        return out


def decode_evt3(words: np.ndarray, wait_for_time_base: bool = False) -> np.ndarray:
    return Evt3Decoder(wait_for_time_base).decode(words)


class DeviceEvtDecoder:
    """A RAW decoder as three kernels per chunk (csrc/xmaps_evt.hpp): the words cross PCIe as the recording stores them, the records
    stay on the device.  One native decoder object serves every format (csrc/host/xm_api_evt3.hpp); a subclass names the word
    dtype and the three entry points that differ: DeviceEvt3Decoder below, evt2.DeviceEvt2Decoder, evt21.DeviceEvt21Decoder,
    dat.DeviceDatDecoder."""

    _dtype = _create = _decode = _push = None

    def __init__(self, engine, max_words: int = 1 << 20, max_events: int = 0, wait_for_time_base: bool = False):
        import ctypes as C

        from . import _native as N
        self._C, self._N, self._e = C, N, engine
        self._lib = engine._lib
        self._d = C.c_void_p(None)
        self.max_words = int(max_words)
        N.check(getattr(self._lib, self._create)(engine._h, int(max_words), int(max_events), C.byref(self._d)))
        if wait_for_time_base:  # (Evt3Decoder's option: events in front of the stream's first EVT_TIME_HIGH are not emitted)
            N.check(self._lib.xm_evt3_wait_for_time_base(self._d, 1))

    def close(self):
        if getattr(self, "_d", None) is not None and self._d.value:
            self._lib.xm_evt3_destroy(self._d)  # (one decoder type serves every format)
            self._d = self._C.c_void_p(None)

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
        self._N.check(self._lib.xm_evt3_reset(self._d))

    def _as_words(self, words) -> np.ndarray:
        return np.ascontiguousarray(words, dtype=self._dtype)

    def set_ext_triggers(self, max_triggers: int):
        """EXT_TRIGGER words -> trigger records beside the events (xm_evt_set_ext_triggers; ext_trigger.py): max_triggers = room for
        one chunk's records, 0 = off (the default).  From the next chunk on; decode / decode_device only, push ignores it."""
        self._N.check(self._lib.xm_evt_set_ext_triggers(self._d, int(max_triggers)))
        self._max_triggers = int(max_triggers)

    def last_ext_triggers(self) -> np.ndarray:
        """the trigger records of the last decode_device (fields t, event_index, id, value); empty when extraction is off"""
        C = self._C
        out = np.zeros(getattr(self, "_max_triggers", 0), EXT_TRIGGER_DTYPE)
        n = C.c_size_t(0)
        self._N.check(self._lib.xm_evt_last_ext_triggers(self._d, C.c_void_p(out.ctypes.data), len(out), C.byref(n)))
        return out[:int(n.value)]

    def decode_device(self, words: np.ndarray):
        C = self._C
        w = self._as_words(words)
        ptr, n = C.c_void_p(None), C.c_size_t(0)
        self._N.check(getattr(self._lib, self._decode)(self._d, C.c_void_p(w.ctypes.data), len(w), C.byref(ptr), C.byref(n)))
        return int(ptr.value or 0), int(n.value)

    def decode(self, words: np.ndarray) -> np.ndarray:
        out = []
        w = self._as_words(words)
        for a in range(0, max(len(w), 1), self.max_words):
            ptr, n = self.decode_device(w[a:a + self.max_words])
            ev = np.zeros(n, EVENT_CD_DTYPE)
            if n:
                self._e.dev_download(ev, ptr)
            out.append(ev)
        cat = np.zeros(sum(len(e) for e in out), EVENT_CD_DTYPE)  # (np.concatenate hands back the packed 14-byte layout under NumPy 2)
        o = 0
        for e in out:
            cat[o:o + len(e)] = e
            o += len(e)
        return cat

    def push(self, ingest, words: np.ndarray, pinned: bool = False, count: bool = True):
        """One chunk = one packet of `ingest`.  pinned=True: `words` lies in pinned host memory (XMapsEngine.host_empty): no
        staging copy.  count=True: waits for the decoder and returns the chunk's event count; count=False: nothing is waited
        for (the ingest's kernels read the count on the device), returns None."""
        C = self._C
        w = self._as_words(words)
        ingest._backpressure(1)
        n = C.c_size_t(0) if count else None
        self._N.check(getattr(self._lib, self._push)(ingest._g, self._d, C.c_void_p(w.ctypes.data), len(w), int(bool(pinned)),
                                                     C.byref(n) if count else None))
        return int(n.value) if count else None


class DeviceEvt3Decoder(DeviceEvtDecoder):
    """The same decoder as three kernels (csrc/xmaps_evt3.hpp: the state machine as scans): the words cross PCIe as the
    recording stores them, the records stay on the device.

        dec = DeviceEvt3Decoder(engine)
        ptr, n = dec.decode_device(words)       # 16-byte EventCD records in device memory, valid until the next call
        evs = dec.decode(words)                 # ... copied back (tests)
        n = dec.push(ingest, words)             # one chunk = one packet of a DeviceIngest (xm_ingest_push_evt3)

    State (row, time, vector base, 24-bit wraps) carries over from chunk to chunk, as in Evt3Decoder."""

    _dtype, _create, _decode, _push = "<u2", "xm_evt3_create", "xm_evt3_decode", "xm_ingest_push_evt3"


def read_raw(path: str, chunk_words: int = 1 << 22):
    """Yields EventCD packets of a .raw file (EVT 3.0)."""
    dec = Evt3Decoder()
    for w in read_raw_words(path, chunk_words):
        ev = dec.decode(w)
        if len(ev):
            yield ev


def read_raw_words(path: str, chunk_words: int = 1 << 20):
    """Yields the EVT 3.0 words of a .raw file chunk by chunk, undecoded: for DeviceEvt3Decoder / process_evt3_words."""
    return read_raw_chunks(path, _FORMAT_NAMES, "<u2", chunk_words, default="3.0")


def encode_evt3(evs: np.ndarray, use_vectors: bool = True) -> np.ndarray:
    """EventCD (time-ordered) -> EVT 3.0 words.  Test helper / file writer: runs of events that share (t, y, p) and have
    increasing columns within a 12-column window become VECT_BASE_X + VECT_12, everything else EVT_ADDR_X."""
    words = []
    cur_y = cur_hi = cur_lo = None
    x, y, p, t = (evs[k].astype(np.int64) for k in ("x", "y", "p", "t"))
    n, i = len(evs), 0
    while i < n:
        hi, lo = (t[i] >> 12) & 0xfff, t[i] & 0xfff
        if hi != cur_hi:
            words.append((T_TIME_HIGH << 12) | hi)
            cur_hi = hi
            cur_lo = None  # a TIME_HIGH that changes the high field restarts the low field at 0 in the decoders: always re-send it
        if lo != cur_lo:
            words.append((T_TIME_LOW << 12) | lo)
            cur_lo = lo
        if y[i] != cur_y:
            words.append((T_ADDR_Y << 12) | (y[i] & 0x7ff))
            cur_y = y[i]
        j = i + 1
        while (use_vectors and j < n and t[j] == t[i] and y[j] == y[i] and p[j] == p[i] and x[j] > x[j - 1]
               and x[j] - x[i] < 12):
            j += 1
        if j - i >= 2:
            mask = 0
            for k in range(i, j):
                mask |= 1 << int(x[k] - x[i])
            words.append((T_VECT_BASE_X << 12) | ((p[i] & 1) << 11) | (x[i] & 0x7ff))
            words.append((T_VECT_12 << 12) | mask)
        else:
            words.append((T_ADDR_X << 12) | ((p[i] & 1) << 11) | (x[i] & 0x7ff))
            j = i + 1
        i = j
    return np.array(words, dtype="<u2")


def encode_evt3_singles(evs: np.ndarray) -> np.ndarray:
    """EventCD (time-ordered) -> EVT 3.0 words without vector words, vectorised (the file writer above is a Python loop): per
    event [TIME_HIGH if the high field changed] [TIME_LOW if the low or the high field changed] [ADDR_Y if the row changed] ADDR_X."""
    n = len(evs)
    if n == 0:
        return np.zeros(0, "<u2")
    x, y, p, t = (evs[k].astype(np.int64) for k in ("x", "y", "p", "t"))
    hi, lo = (t >> 12) & 0xfff, t & 0xfff
    first = np.zeros(n, bool)
    first[0] = True
    c_hi = first | (np.concatenate(([0], hi[:-1])) != hi)
    c_lo = first | c_hi | (np.concatenate(([0], lo[:-1])) != lo)  # (a changed high field restarts the low field: re-send it)
    c_y = first | (np.concatenate(([0], y[:-1])) != y)
    per = c_hi.astype(np.int64) + c_lo + c_y + 1
    end = np.cumsum(per)  # one past the event's ADDR_X word
    words = np.zeros(int(end[-1]), np.int64)
    words[end - 1] = (T_ADDR_X << 12) | ((p & 1) << 11) | (x & 0x7ff)
    pos = end - 1 - c_y
    words[pos[c_y]] = ((T_ADDR_Y << 12) | (y & 0x7ff))[c_y]
    pos = pos - c_lo
    words[pos[c_lo]] = ((T_TIME_LOW << 12) | lo)[c_lo]
    pos = pos - c_hi
    words[pos[c_hi]] = ((T_TIME_HIGH << 12) | hi)[c_hi]
    return words.astype("<u2")


def _raw_header(width: int, height: int) -> bytes:
    return f"% evt 3.0\n% format EVT3;height={height};width={width}\n% geometry {width}x{height}\n% end\n".encode("ascii")


def write_raw(path: str, evs: np.ndarray, width: int = 640, height: int = 480):
    with open(path, "wb") as f:
        f.write(_raw_header(width, height))
        f.write(encode_evt3(evs).tobytes())


T_EXT_TRIGGER = 0xA
REPLAY_MIN_EVENTS = 1000  # frame_sync="ext_trigger" skips frames of this many events or fewer (MIN_EVENTS_PER_FRAME)


class FrameRecordingWriter:
    """A recording of the frames a pipeline SHOWED, replayable through frame_sync="ext_trigger" (ext_trigger_id=0): host code only.

        with FrameRecordingWriter("session.raw", width, height) as rec:
            params = RuntimeParams(..., record_callback=rec)      # record_callback(words, stats) = rec.write_frame(words, stats)

    Per frame: the two time words of stats.t_first, one EXT_TRIGGER word (id 0, value 1), then the frame's words as the device
    encoded them (XMapsEngine.frames_to_evt3_words / the ingest's record stage: they begin with their own EVT_TIME_HIGH,
    EVT_TIME_LOW and EVT_ADDR_Y, so nothing of the previous frame reaches into them).  close() writes the time words of the last
    frame's t_last and a closing trigger.  The header is write_raw's.  What is recorded is the stream behind the polarity and
    activity filters and behind the cut: it replays to the same frames whatever the filters' rules are by then.

    Two things a reader of the file must know:
     - STAMPS come back shifted by a multiple of 2^24 us: EVT 3.0 carries 24 bits of time and a decoder counts a recording's first
       loop as 0, so a session whose stamps start at 40 000 000 replays from 40 000 000 - 2 * 2^24.  Every output of the pipeline
       depends on differences inside a frame only.
     - a pause-cut frame may hold 997 .. 1000 events (the reference's trigger finder asks for more than 1000 and then trims 4),
       while the ext_trigger chain skips frames of <= 1000 events: such a frame is written like every other, comes back from a
       cutter with min_events=0, and is NOT shown by the replaying pipeline.  `frames_below_replay_minimum` counts them.
    Frames that came without words (more than record_max_words: all or nothing) cannot be written: `frames_without_words`."""

    def __init__(self, path: str, width: int, height: int):
        self._f = open(path, "wb")
        self._f.write(_raw_header(width, height))
        self.frames = 0
        self.frames_below_replay_minimum = 0
        self.frames_without_words = 0
        self.words_written = 0
        self._t_last = None

    def _put(self, words):
        w = np.ascontiguousarray(words, dtype="<u2")
        self._f.write(w.tobytes())
        self.words_written += len(w)

    @staticmethod
    def _trigger_at(t: int) -> list:
        return [(T_TIME_HIGH << 12) | ((int(t) >> 12) & 0xfff), (T_TIME_LOW << 12) | (int(t) & 0xfff), (T_EXT_TRIGGER << 12) | 1]

    def write_frame(self, words, stats):
        if self._f is None:
            raise ValueError("the recording is closed")
        if words is None or not stats.n_events:
            self.frames_without_words += 1
            return
        if len(words) != stats.n_words:
            raise ValueError(f"{len(words)} words, the statistics say {stats.n_words}")
        self._put(self._trigger_at(stats.t_first))
        self._put(words)
        self._t_last = int(stats.t_last)
        self.frames += 1
        self.frames_below_replay_minimum += int(stats.n_events <= REPLAY_MIN_EVENTS)

    __call__ = write_frame

    def close(self):
        if self._f is None:
            return
        if self._t_last is not None:
            self._put(self._trigger_at(self._t_last))
        self._f.close()
        self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
