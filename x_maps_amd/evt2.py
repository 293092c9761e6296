"""Prophesee EVT 2.0 RAW decoder ("next" row N4: "EVT2/EVT3 RAW reader"): the oldest of the three public RAW encodings.

The reference reads its recordings through Metavision's closed readers (python/bias_events_iterator.py:53-96); which encoding a
.raw file holds is the camera's choice (Gen3 sensors: EVT 2.0, Gen4: EVT 3.0 or EVT 2.1; evt3.py and evt21.py are the other two).  EVT 2.0 is an ASCII
header (lines starting with '%') followed by little-endian 32-bit words, type in the top four bits:

    0x0 CD_OFF / 0x1 CD_ON   [27:22] t[5:0]   [21:11] x   [10:0] y       one event, polarity = the type
    0x8 EVT_TIME_HIGH        [27:0]  t[33:6]                             the time base of the words behind it
    0xA EXT_TRIGGER, 0xE OTHERS, 0xF CONTINUED                            skipped here

    t (us) = (loops << 34) | (time_high << 6) | t[5:0];   a loop = the 28-bit field falls back by more than 2^27 (4.8 hours)

`Evt2Decoder` evaluates the state machine for a whole buffer at once (forward fill of "the last TIME_HIGH word at or before i"),
the shape the device kernels have (csrc/xmaps_evt2.hpp: three scan launches).  PARITY: unpinned against Metavision (closed, no
recording ships with the reference); pinned by hand-derived word sequences and an independent word-by-word state machine
(oracle/evt2_oracle.py, tests/test_evt2.py) and by the round trip through the encoder below.
"""
from __future__ import annotations

import numpy as np

from .evt3 import DeviceEvtDecoder, _ffill_index, raw_format, read_raw_chunks, split_raw_header  # noqa: F401 (a name of this module too)
from .synthetic import EVENT_CD_DTYPE

T_CD_OFF, T_CD_ON, T_TIME_HIGH = 0x0, 0x1, 0x8
_FORMAT_NAMES = ("2.0", "2", "EVT2", "EVT2.0")


class Evt2Decoder:
    """Streaming decoder: feed chunks of words, get EventCD arrays; the time base and the loop count carry over."""

    def __init__(self, wait_for_time_base: bool = False):
        self.t_high = 0
        self.t_loops = 0
        self.wait_for_time_base = bool(wait_for_time_base)  # CD words in front of the stream's first EVT_TIME_HIGH are not emitted (evt3.py)
        self.have_time = False

    def decode(self, words: np.ndarray) -> np.ndarray:
        w = np.ascontiguousarray(words, dtype="<u4").astype(np.int64)
        n = len(w)
        if n == 0:
            return np.zeros(0, EVENT_CD_DTYPE)
        typ = w >> 28
        is_hi = typ == T_TIME_HIGH
        ih = _ffill_index(is_hi)
        hi_words = np.nonzero(is_hi)[0]
        th_seq = w[hi_words] & 0x0fffffff
        prev = np.concatenate(([self.t_high], th_seq[:-1])) if len(th_seq) else th_seq
        wraps = np.cumsum((prev - th_seq) > (1 << 27)) if len(th_seq) else np.zeros(0, np.int64)
        loops_at = np.full(n, self.t_loops, np.int64)
        if len(hi_words):
            loops_at = np.where(ih >= 0, self.t_loops + wraps[np.searchsorted(hi_words, np.maximum(ih, 0))], self.t_loops)
        t_high = np.where(ih >= 0, w[np.maximum(ih, 0)] & 0x0fffffff, self.t_high)
        cd = np.nonzero(typ <= T_CD_ON)[0]
        if self.wait_for_time_base and not self.have_time:
            cd = cd[ih[cd] >= 0]
        self.have_time = self.have_time or len(hi_words) > 0
        out = np.zeros(len(cd), EVENT_CD_DTYPE)
        wc = w[cd]
        out["x"] = (wc >> 11) & 0x7ff
        out["y"] = wc & 0x7ff
        out["p"] = wc >> 28
        out["t"] = (loops_at[cd] << 34) | (t_high[cd] << 6) | ((wc >> 22) & 0x3f)
        self.t_high, self.t_loops = int(t_high[-1]), int(loops_at[-1])
        return out


def decode_evt2(words: np.ndarray, wait_for_time_base: bool = False) -> np.ndarray:
    return Evt2Decoder(wait_for_time_base).decode(words)


def encode_evt2(evs: np.ndarray, time_high_every_us: int = 0) -> np.ndarray:
    """EventCD (time-ordered) -> EVT 2.0 words, vectorised: EVT_TIME_HIGH in front of every event whose t >> 6 differs from its
    predecessor's (and of the first one), then the CD word.  time_high_every_us > 0 additionally repeats the current EVT_TIME_HIGH
    in front of events that are that far from the last one written -- cameras send it periodically, events or not."""
    n = len(evs)
    if n == 0:
        return np.zeros(0, "<u4")
    x, y, p, t = (evs[k].astype(np.int64) for k in ("x", "y", "p", "t"))
    hi, lo = (t >> 6) & 0x0fffffff, t & 0x3f
    c_hi = np.ones(n, bool)
    c_hi[1:] = hi[1:] != hi[:-1]
    if time_high_every_us > 0:
        c_hi[1:] |= (t[1:] // time_high_every_us) != (t[:-1] // time_high_every_us)
    per = c_hi.astype(np.int64) + 1
    end = np.cumsum(per)
    words = np.zeros(int(end[-1]), np.int64)
    words[end - 1] = ((p & 1) << 28) | (lo << 22) | ((x & 0x7ff) << 11) | (y & 0x7ff)
    words[(end - 2)[c_hi]] = ((T_TIME_HIGH << 28) | hi)[c_hi]
    return words.astype("<u4")


def _is_evt2(fields: dict) -> bool:
    return raw_format(fields) in _FORMAT_NAMES


def read_raw(path: str, chunk_words: int = 1 << 22):
    """Yields EventCD packets of a .raw file (EVT 2.0)."""
    dec = Evt2Decoder()
    for w in read_raw_words(path, chunk_words):
        ev = dec.decode(w)
        if len(ev):
            yield ev


def read_raw_words(path: str, chunk_words: int = 1 << 20):
    """Yields the EVT 2.0 words of a .raw file chunk by chunk, undecoded: for DeviceEvt2Decoder / process_evt2_words."""
    return read_raw_chunks(path, _FORMAT_NAMES, "<u4", chunk_words)


def write_raw(path: str, evs: np.ndarray, width: int = 640, height: int = 480):
    hdr = f"% evt 2.0\n% format EVT2;height={height};width={width}\n% geometry {width}x{height}\n% end\n".encode("ascii")
    with open(path, "wb") as f:
        f.write(hdr)
        f.write(encode_evt2(evs).tobytes())


class DeviceEvt2Decoder(DeviceEvtDecoder):
    """The same decoder as three kernels (csrc/xmaps_evt2.hpp): the words cross PCIe as the recording stores them (4-8 bytes per
    event), the records stay on the device.  Same interface as evt3.DeviceEvt3Decoder (push: xm_ingest_push_evt2)."""

    _dtype, _create, _decode, _push = "<u4", "xm_evt2_create", "xm_evt2_decode", "xm_ingest_push_evt2"
