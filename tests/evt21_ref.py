"""TEST INFRASTRUCTURE ONLY (never imported by the product): an independent EVT 2.1 decoder, word by word.

Written from the format description (64-bit little-endian words, type in bits 63..60), not from x_maps_amd/evt21.py: a plain loop
over the words with the decoder's state in three variables; only the expansion of a word's validity mask into its events is
vectorised.  It shares no code and no structure with the product's two decoders (the NumPy forward fills, the device scans).

    type 0x0 EVT_NEG, 0x1 EVT_POS : bits 59..54 = t & 63, bits 53..43 = x_base, bits 42..32 = y, bits 31..0 = valid;
                                    one event at (x_base + n, y) per set bit n, ascending n, polarity = type
    type 0x8 EVT_TIME_HIGH         : bits 59..32 = t >> 6
    anything else                  : no event, no state change
    a TIME_HIGH value more than 2^27 below the previous one = the 34-bit clock has wrapped once more
    legacy halves: the word is stored as two 32-bit little-endian halves, the HIGH half first
"""
import numpy as np

EVENT_CD = np.dtype({"names": ["x", "y", "p", "t"], "formats": ["<u2", "<u2", "<i2", "<i8"], "offsets": [0, 2, 4, 8], "itemsize": 16})
_BITS = np.arange(32, dtype=np.int64)


class Evt21StateMachine:
    def __init__(self, wait_for_time_base=False, legacy_halves=False):
        self.time_high = 0
        self.loops = 0
        self.wait = bool(wait_for_time_base)
        self.legacy = bool(legacy_halves)
        self.have_high = False

    def feed(self, words):
        xs, ys, ps, ts = [], [], [], []
        for w in np.asarray(words, dtype="<u8").tolist():
            if self.legacy:
                w = ((w & 0xFFFFFFFF) << 32) | (w >> 32)
            kind = w >> 60
            if kind == 0x8:
                value = (w >> 32) & 0x0FFFFFFF
                if self.time_high - value > (1 << 27):
                    self.loops += 1
                self.time_high = value
                self.have_high = True
            elif kind in (0x0, 0x1) and not (self.wait and not self.have_high):
                valid = w & 0xFFFFFFFF
                cols = _BITS[((valid >> _BITS) & 1) == 1]  # (the mask expansion: the one vectorised step)
                t = (self.loops << 34) | (self.time_high << 6) | ((w >> 54) & 0x3F)
                xs.append(((w >> 43) & 0x7FF) + cols)
                ys.append(np.full(len(cols), (w >> 32) & 0x7FF, np.int64))
                ps.append(np.full(len(cols), kind, np.int64))
                ts.append(np.full(len(cols), t, np.int64))
        n = sum(len(a) for a in xs)
        evs = np.zeros(n, EVENT_CD)
        if n:
            evs["x"], evs["y"], evs["p"], evs["t"] = np.concatenate(xs), np.concatenate(ys), np.concatenate(ps), np.concatenate(ts)
        return evs


def decode(words, wait_for_time_base=False, legacy_halves=False):
    return Evt21StateMachine(wait_for_time_base, legacy_halves).feed(words)
