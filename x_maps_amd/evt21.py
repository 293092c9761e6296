"""Prophesee EVT 2.1 RAW decoder ("next" row N4): the 64-bit vectorised one of the three public RAW encodings.

Gen4 / IMX636 cameras can be set to it (evt2.py and evt3.py are the other two).  An ASCII header (lines starting with '%'), then
little-endian 64-bit words, type in the top four bits:

    0x0 EVT_NEG / 0x1 EVT_POS   [59:54] t[5:0]   [53:43] x_base   [42:32] y   [31:0] valid
                                bit n of valid set -> one event at (x_base + n, y), polarity = the type, in ascending n
    0x8 EVT_TIME_HIGH           [59:32] t[33:6]  ([31:0] ignored)            the time base of the words behind it
    0xA EXT_TRIGGER, 0xE OTHERS, 0xF CONTINUED, anything else                 skipped here

    t (us) = (loops << 34) | (time_high << 6) | t[5:0];   loops, the initial state and wait_for_time_base exactly as EVT 2.0

x_base is documented as a multiple of 32; x_base + n is decoded whatever it is (at most 2047 + 31).  Half order: "endianness=legacy"
in the header's format line means every word is stored as two 32-bit little-endian halves with the HIGH half first; the decoders
take that as an option (`legacy_halves`) and put the halves back where they load a word.  A header that names neither is read as little.

`Evt21Decoder` evaluates the state machine for a whole buffer at once (EVT 2.0's forward fill, then the masks expanded by their
popcounts), the shape the device kernels have (csrc/xmaps_evt21.hpp: three scan launches; its two emit kernels, by word and by
output slot, are timed in profiles/evt21.md).
PARITY: unpinned against Metavision (closed, no recording ships with the reference); pinned by hand-derived word sequences and an
independent word-by-word state machine (tests/evt21_ref.py, tests/test_evt21.py) and by the round trip through the encoder below.
"""
from __future__ import annotations

import numpy as np

from .evt3 import DeviceEvtDecoder, _ffill_index, raw_format, read_raw_chunks, split_raw_header  # noqa: F401 (names of this module too)
from .synthetic import EVENT_CD_DTYPE

T_EVT_NEG, T_EVT_POS, T_TIME_HIGH = 0x0, 0x1, 0x8
_FORMAT_NAMES = ("2.1", "EVT21", "EVT2.1")
_U = np.uint64


def swap_halves(words: np.ndarray) -> np.ndarray:
    """little <-> legacy: the two 32-bit halves of every 64-bit word exchanged"""
    w = np.ascontiguousarray(words, dtype="<u8")
    return ((w << _U(32)) | (w >> _U(32))).astype("<u8")


def header_legacy_halves(fields: dict) -> bool:
    """the half order a RAW header's format line names: '% format EVT21;...;endianness=legacy' (absent or 'little': False)"""
    for part in fields.get("format", "").split(";")[1:]:
        k, _, v = part.partition("=")
        if k.strip().lower() == "endianness":
            return v.strip().lower() == "legacy"
    return False


class Evt21Decoder:
    """Streaming decoder: feed chunks of words, get EventCD arrays; the time base and the loop count carry over."""

    def __init__(self, wait_for_time_base: bool = False, legacy_halves: bool = False):
        self.t_high = 0
        self.t_loops = 0
        self.wait_for_time_base = bool(wait_for_time_base)  # events in front of the stream's first EVT_TIME_HIGH are not emitted (evt3.py)
        self.legacy_halves = bool(legacy_halves)
        self.have_time = False

    def decode(self, words: np.ndarray) -> np.ndarray:
        w = np.ascontiguousarray(words, dtype="<u8")
        n = len(w)
        if n == 0:
            return np.zeros(0, EVENT_CD_DTYPE)
        if self.legacy_halves:
            w = swap_halves(w)
        top = (w >> _U(32)).astype(np.int64)  # type, t[5:0], x_base, y where EVT 2.0 has them in its 32-bit word
        typ = top >> 28
        is_hi = typ == T_TIME_HIGH
        ih = _ffill_index(is_hi)
        hi_words = np.nonzero(is_hi)[0]
        th_seq = top[hi_words] & 0x0fffffff
        prev = np.concatenate(([self.t_high], th_seq[:-1])) if len(th_seq) else th_seq
        wraps = np.cumsum((prev - th_seq) > (1 << 27)) if len(th_seq) else np.zeros(0, np.int64)
        loops_at = np.full(n, self.t_loops, np.int64)
        if len(hi_words):
            loops_at = np.where(ih >= 0, self.t_loops + wraps[np.searchsorted(hi_words, np.maximum(ih, 0))], self.t_loops)
        t_high = np.where(ih >= 0, top[np.maximum(ih, 0)] & 0x0fffffff, self.t_high)
        cd = np.nonzero(typ <= T_EVT_POS)[0]
        if self.wait_for_time_base and not self.have_time:
            cd = cd[ih[cd] >= 0]
        self.have_time = self.have_time or len(hi_words) > 0
        # the masks expanded: row r of `bits` is word cd[r], column b its bit b; np.nonzero walks them in word order, ascending bit
        bits = np.unpackbits((w[cd] & _U(0xffffffff)).astype("<u4").view(np.uint8).reshape(-1, 4), axis=1, bitorder="little")
        r, b = np.nonzero(bits)
        src = cd[r]
        out = np.zeros(len(src), EVENT_CD_DTYPE)
        ws = top[src]
        out["x"] = ((ws >> 11) & 0x7ff) + b
        out["y"] = ws & 0x7ff
        out["p"] = ws >> 28
        out["t"] = (loops_at[src] << 34) | (t_high[src] << 6) | ((ws >> 22) & 0x3f)
        self.t_high, self.t_loops = int(t_high[-1]), int(loops_at[-1])
        return out


def decode_evt21(words: np.ndarray, wait_for_time_base: bool = False, legacy_halves: bool = False) -> np.ndarray:
    return Evt21Decoder(wait_for_time_base, legacy_halves).decode(words)


def encode_evt21(evs: np.ndarray, use_vectors: bool = True, time_high_every_us: int = 0) -> np.ndarray:
    """EventCD (time-ordered) -> EVT 2.1 words (little), vectorised.  use_vectors: a run of consecutive events that share
    (t, y, p, x >> 5) and whose columns rise becomes ONE word (x_base = the columns' multiple of 32, one bit each); otherwise one
    bit per word.  EVT_TIME_HIGH in front of every word whose t >> 6 differs from its predecessor's (and of the first one);
    time_high_every_us > 0 additionally repeats it in front of words that are that far from the last one written, as encode_evt2."""
    n = len(evs)
    if n == 0:
        return np.zeros(0, "<u8")
    x, y, p, t = (evs[k].astype(np.int64) for k in ("x", "y", "p", "t"))
    first = np.ones(n, bool)
    if use_vectors:
        first[1:] = (t[1:] != t[:-1]) | (y[1:] != y[:-1]) | (p[1:] != p[:-1]) | ((x[1:] >> 5) != (x[:-1] >> 5)) | (x[1:] <= x[:-1])
    g = np.nonzero(first)[0]  # every word's first event
    mask = np.bitwise_or.reduceat(np.left_shift(1, x & 31), g)
    tg, hi, lo = t[g], (t[g] >> 6) & 0x0fffffff, t[g] & 0x3f
    m = len(g)
    c_hi = np.ones(m, bool)
    c_hi[1:] = hi[1:] != hi[:-1]
    if time_high_every_us > 0:
        c_hi[1:] |= (tg[1:] // time_high_every_us) != (tg[:-1] // time_high_every_us)
    end = np.cumsum(c_hi.astype(np.int64) + 1)
    words = np.zeros(int(end[-1]), np.uint64)
    top = ((p[g] & 1) << 28) | (lo << 22) | (((x[g] >> 5 << 5) & 0x7ff) << 11) | (y[g] & 0x7ff)
    words[end - 1] = (top.astype(np.uint64) << _U(32)) | mask.astype(np.uint64)
    words[(end - 2)[c_hi]] = (((T_TIME_HIGH << 28) | hi)[c_hi]).astype(np.uint64) << _U(32)
    return words.astype("<u8")


def _is_evt21(fields: dict) -> bool:
    return raw_format(fields) in _FORMAT_NAMES


def raw_legacy_halves(path: str) -> bool:
    """the half order the header of a .raw file names"""
    with open(path, "rb") as f:
        fields, _ = split_raw_header(f.read(1 << 16))
    return header_legacy_halves(fields)


def read_raw(path: str, chunk_words: int = 1 << 22):
    """Yields EventCD packets of a .raw file (EVT 2.1, either half order)."""
    dec = Evt21Decoder(legacy_halves=raw_legacy_halves(path))
    for w in read_raw_words(path, chunk_words):
        ev = dec.decode(w)
        if len(ev):
            yield ev


def read_raw_words(path: str, chunk_words: int = 1 << 20):
    """Yields the EVT 2.1 words of a .raw file chunk by chunk, undecoded and as the file stores them (raw_legacy_halves says in
    which half order): for DeviceEvt21Decoder / process_evt21_words."""
    return read_raw_chunks(path, _FORMAT_NAMES, "<u8", chunk_words)


def write_raw(path: str, evs: np.ndarray, width: int = 640, height: int = 480, use_vectors: bool = True, legacy_halves: bool = False):
    order = "legacy" if legacy_halves else "little"
    hdr = (f"% evt 2.1\n% format EVT21;height={height};width={width};endianness={order}\n% geometry {width}x{height}\n"
           f"% end\n").encode("ascii")
    words = encode_evt21(evs, use_vectors)
    with open(path, "wb") as f:
        f.write(hdr)
        f.write((swap_halves(words) if legacy_halves else words).tobytes())


class DeviceEvt21Decoder(DeviceEvtDecoder):
    """The same decoder as three kernels (csrc/xmaps_evt21.hpp): the words cross PCIe as the recording stores them (8 bytes for up
    to 32 events), the records stay on the device.  Same interface as evt3.DeviceEvt3Decoder (push: xm_ingest_push_evt21);
    max_events = 0 means 4 * max_words.  legacy_halves: the words are stored HIGH half first; the kernels put them back."""

    _dtype, _create, _decode, _push = "<u8", "xm_evt21_create", "xm_evt21_decode", "xm_ingest_push_evt21"

    def __init__(self, engine, max_words: int = 1 << 20, max_events: int = 0, wait_for_time_base: bool = False, legacy_halves: bool = False):
        super().__init__(engine, max_words, max_events, wait_for_time_base)
        self.set_legacy_halves(legacy_halves)

    def set_legacy_halves(self, on: bool):
        self._N.check(self._lib.xm_evt21_set_legacy_halves(self._d, int(bool(on))))
