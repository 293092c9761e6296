"""TEST INFRASTRUCTURE ONLY (never imported by the product): independent decoders of the three RAW encodings that also return the
EXT_TRIGGER words, word by word.

Written from the format descriptions, not from x_maps_amd: one plain loop per format over the words, the decoder's state in a
few variables, events and triggers appended as they come.  They share no code and no structure with the product's host form
(NumPy forward fills over a marker stream) or its device form (scans).

    EVT 3.0 (16 bit): 0x0 ADDR_Y y[10:0] | 0x2 ADDR_X x[10:0] p[11] | 0x3 VECT_BASE_X x[10:0] p[11] | 0x4 VECT_12 | 0x5 VECT_8 |
                      0x6 TIME_LOW t[11:0] | 0x8 TIME_HIGH t[23:12] | 0xA EXT_TRIGGER id[11:8] value[0]
                      a TIME_HIGH more than 0x800 below the previous one = one more 24-bit wrap; a TIME_HIGH that changes the field
                      sets the low field to 0
    EVT 2.0 (32 bit): 0x0 / 0x1 CD t[27:22] x[21:11] y[10:0] | 0x8 TIME_HIGH t[27:0] | 0xA EXT_TRIGGER t[27:22] id[12:8] value[0]
    EVT 2.1 (64 bit): 0x0 / 0x1 CD t[59:54] x_base[53:43] y[42:32] valid[31:0] | 0x8 TIME_HIGH t[59:32] |
                      0xA EXT_TRIGGER t[59:54] id[44:40] value[32]; legacy halves: stored HIGH half first
                      a TIME_HIGH more than 2^27 below the previous one = one more loop of the 34-bit clock
    wait_for_time_base: nothing is emitted in front of the stream's first TIME_HIGH word, neither event nor trigger
    a trigger's event_index = the events emitted for this feed() call in front of it
"""
import numpy as np

EVENT_CD = np.dtype({"names": ["x", "y", "p", "t"], "formats": ["<u2", "<u2", "<i2", "<i8"], "offsets": [0, 2, 4, 8], "itemsize": 16})
TRIGGER = np.dtype({"names": ["t", "event_index", "id", "value", "reserved"], "formats": ["<i8", "<u4", "u1", "u1", "<u2"],
                    "offsets": [0, 8, 12, 13, 14], "itemsize": 16})


def _arrays(events, triggers):
    ev = np.zeros(len(events), EVENT_CD)
    for i, (x, y, p, t) in enumerate(events):
        ev[i] = (x, y, p, t)
    tr = np.zeros(len(triggers), TRIGGER)
    for i, (t, idx, ident, value) in enumerate(triggers):
        tr[i] = (t, idx, ident, value, 0)
    return ev, tr


class Evt3Machine:
    def __init__(self, wait_for_time_base=False):
        self.row = self.base = self.pol = self.low = self.high = self.wraps = 0
        self.wait, self.have_high = bool(wait_for_time_base), False

    def feed(self, words):
        events, triggers = [], []
        for w in np.asarray(words, dtype="<u2").tolist():
            kind, live = w >> 12, not (self.wait and not self.have_high)
            now = (self.wraps << 24) | (self.high << 12) | self.low
            if kind == 0x0:
                self.row = w & 0x7FF
            elif kind == 0x2:
                if live:
                    events.append((w & 0x7FF, self.row, (w >> 11) & 1, now))
            elif kind == 0x3:
                self.base, self.pol = w & 0x7FF, (w >> 11) & 1
            elif kind in (0x4, 0x5):
                width = 12 if kind == 0x4 else 8
                for bit in range(width):
                    if live and (w >> bit) & 1:
                        events.append(((self.base + bit) & 0xFFFF, self.row, self.pol, now))
                self.base += width
            elif kind == 0x6:
                self.low = w & 0xFFF
            elif kind == 0x8:
                value = w & 0xFFF
                if self.high - value > 0x800:
                    self.wraps += 1
                if value != self.high:
                    self.low = 0
                self.high, self.have_high = value, True
            elif kind == 0xA and live:
                triggers.append((now, len(events), (w >> 8) & 0xF, w & 1))
        return _arrays(events, triggers)


class Evt2Machine:
    def __init__(self, wait_for_time_base=False):
        self.high = self.loops = 0
        self.wait, self.have_high = bool(wait_for_time_base), False

    def feed(self, words):
        events, triggers = [], []
        for w in np.asarray(words, dtype="<u4").tolist():
            kind, live = w >> 28, not (self.wait and not self.have_high)
            now = (self.loops << 34) | (self.high << 6) | ((w >> 22) & 0x3F)
            if kind == 0x8:
                value = w & 0x0FFFFFFF
                if self.high - value > (1 << 27):
                    self.loops += 1
                self.high, self.have_high = value, True
            elif kind in (0x0, 0x1) and live:
                events.append(((w >> 11) & 0x7FF, w & 0x7FF, kind, now))
            elif kind == 0xA and live:
                triggers.append((now, len(events), (w >> 8) & 0x1F, w & 1))
        return _arrays(events, triggers)


class Evt21Machine:
    def __init__(self, wait_for_time_base=False, legacy_halves=False):
        self.high = self.loops = 0
        self.wait, self.have_high, self.legacy = bool(wait_for_time_base), False, bool(legacy_halves)

    def feed(self, words):
        events, triggers = [], []
        for w in np.asarray(words, dtype="<u8").tolist():
            if self.legacy:
                w = ((w & 0xFFFFFFFF) << 32) | (w >> 32)
            kind, live = w >> 60, not (self.wait and not self.have_high)
            now = (self.loops << 34) | (self.high << 6) | ((w >> 54) & 0x3F)
            if kind == 0x8:
                value = (w >> 32) & 0x0FFFFFFF
                if self.high - value > (1 << 27):
                    self.loops += 1
                self.high, self.have_high = value, True
            elif kind in (0x0, 0x1) and live:
                m = w & 0xFFFFFFFF
                while m:  # the set bits, ascending
                    events.append((((w >> 43) & 0x7FF) + (m & -m).bit_length() - 1, (w >> 32) & 0x7FF, kind, now))
                    m &= m - 1
            elif kind == 0xA and live:
                triggers.append((now, len(events), (w >> 40) & 0x1F, (w >> 32) & 1))
        return _arrays(events, triggers)


def machine(fmt, wait_for_time_base=False, legacy_halves=False):
    if fmt == 3:
        return Evt3Machine(wait_for_time_base)
    if fmt == 2:
        return Evt2Machine(wait_for_time_base)
    return Evt21Machine(wait_for_time_base, legacy_halves)


def decode(words, fmt, wait_for_time_base=False, legacy_halves=False):
    return machine(fmt, wait_for_time_base, legacy_halves).feed(words)
