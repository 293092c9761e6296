"""TEST INFRASTRUCTURE ONLY (never imported by the product): an independent DAT (version 2, CD) decoder, record by record.

Written from the format description, not from x_maps_amd/dat.py: the bytes are unpacked with `struct`, the state is two
variables in a plain loop.

    record = u32 ts, u32 data (little-endian);  x = data & 0x3FFF, y = (data >> 14) & 0x3FFF, p = data >> 28
    ts more than 2^31 below the record before it = the 32-bit clock has wrapped once more; t = (loops << 32) | ts
"""
import struct

import numpy as np

EVENT_CD = np.dtype({"names": ["x", "y", "p", "t"], "formats": ["<u2", "<u2", "<i2", "<i8"], "offsets": [0, 2, 4, 8], "itemsize": 16})


class DatStateMachine:
    def __init__(self):
        self.last_ts = 0
        self.loops = 0

    def feed(self, records):
        raw = np.ascontiguousarray(records).tobytes()
        out = []
        for ts, data in struct.iter_unpack("<II", raw):
            if self.last_ts - ts > (1 << 31):
                self.loops += 1
            self.last_ts = ts
            out.append((data & 0x3FFF, (data >> 14) & 0x3FFF, data >> 28, (self.loops << 32) | ts))
        evs = np.zeros(len(out), EVENT_CD)
        if out:
            a = np.array(out, dtype=np.int64)
            evs["x"], evs["y"], evs["p"], evs["t"] = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
        return evs


def decode(records):
    return DatStateMachine().feed(records)
