"""Prophesee DAT reader (version 2, CD events): the other container the reference's --input takes (".raw, .dat").

The reference reads its recordings through Metavision's closed readers (python/bias_events_iterator.py:53-96).  A DAT file is
ASCII header lines starting with '%' ("% Version 2", "% Height 480", "% Width 640", "% Date ..."), then two bytes -- the event
type, which must be 0x0C (CD), and the event size, which must be 8 -- and then 8-byte little-endian records:

    u32 ts (us)     u32 data:  [13:0] x   [27:14] y   [31:28] p            every record is one event

    t (us) = (loops << 32) | ts;   a loop = ts falls back by more than 2^31 against the record before it (smaller steps
    backwards are kept as they are)

`DatDecoder` evaluates that for a whole buffer at once, the shape the device kernels have (csrc/xmaps_dat.hpp: three scan launches,
the emit elementwise).  "% Version 1", another event type or another event size is a ValueError that names the file and the field.
PARITY: unpinned against Metavision (closed, no recording ships with the reference); pinned by hand-derived records and an
independent record-by-record checker (tests/dat_ref.py, tests/test_dat.py) and by the round trip through the encoder below.
"""
from __future__ import annotations

import numpy as np

from .evt3 import DeviceEvtDecoder, split_raw_header
from .synthetic import EVENT_CD_DTYPE

DAT_DTYPE = np.dtype([("ts", "<u4"), ("data", "<u4")])
EVENT_TYPE_CD, EVENT_SIZE = 0x0C, 8


def as_records(records) -> np.ndarray:
    """a chunk as DAT_DTYPE records, from that dtype or from the same 8 bytes viewed as '<u8' (ts in the low half)"""
    a = np.asarray(records)
    if a.dtype == DAT_DTYPE:
        return np.ascontiguousarray(a)
    return np.ascontiguousarray(a, dtype="<u8").view(DAT_DTYPE)


def split_dat_header(blob: bytes, path: str = "<buffer>") -> tuple[dict, int]:
    """-> (the header's fields, offset of the first record); ValueError for what this reader does not read"""
    fields, off = split_raw_header(blob)
    version = fields.get("Version", "").strip()
    if version != "2":
        raise ValueError(f"{path}: DAT Version {version or '(none)'!s} is not supported (field 'Version' must be 2)")
    if len(blob) < off + 2:
        raise ValueError(f"{path}: the file ends in front of the event type and event size bytes")
    if blob[off] != EVENT_TYPE_CD:
        raise ValueError(f"{path}: event type 0x{blob[off]:02X} is not supported (field 'event type' must be 0x0C, CD events)")
    if blob[off + 1] != EVENT_SIZE:
        raise ValueError(f"{path}: event size {blob[off + 1]} is not supported (field 'event size' must be 8)")
    return fields, off + 2


def is_dat(path: str, fields: dict | None = None) -> bool:
    """a .dat suffix, or the header fields a DAT file has and a RAW file has not"""
    if path.lower().endswith(".dat"):
        return True
    if fields is None:
        with open(path, "rb") as f:
            fields, _ = split_raw_header(f.read(1 << 16))
    return "Version" in fields and "evt" not in fields and "format" not in fields


class DatDecoder:
    """Streaming decoder: feed chunks of records, get EventCD arrays; the last stamp and the loop count carry over."""

    def __init__(self, wait_for_time_base: bool = False):  # (the option of the RAW decoders: nothing to wait for in this format)
        self.last_ts = 0
        self.t_loops = 0

    def decode(self, records) -> np.ndarray:
        r = as_records(records)
        if len(r) == 0:
            return np.zeros(0, EVENT_CD_DTYPE)
        ts, data = r["ts"].astype(np.int64), r["data"].astype(np.int64)
        prev = np.concatenate(([self.last_ts], ts[:-1]))
        loops = self.t_loops + np.cumsum((prev - ts) > (1 << 31))
        out = np.zeros(len(r), EVENT_CD_DTYPE)
        out["x"] = data & 0x3fff
        out["y"] = (data >> 14) & 0x3fff
        out["p"] = data >> 28
        out["t"] = (loops << 32) | ts
        self.last_ts, self.t_loops = int(ts[-1]), int(loops[-1])
        return out


def decode_dat(records, wait_for_time_base: bool = False) -> np.ndarray:
    return DatDecoder().decode(records)


def encode_dat(evs: np.ndarray) -> np.ndarray:
    """EventCD -> DAT records, vectorised: one record per event, the low 32 bits of its stamp"""
    out = np.zeros(len(evs), DAT_DTYPE)
    x, y, p, t = (evs[k].astype(np.int64) for k in ("x", "y", "p", "t"))
    out["ts"] = t & 0xffffffff
    out["data"] = (x & 0x3fff) | ((y & 0x3fff) << 14) | ((p & 0xf) << 28)
    return out


def read_raw(path: str, chunk_words: int = 1 << 22):
    """Yields EventCD packets of a .dat file."""
    dec = DatDecoder()
    for r in read_raw_words(path, chunk_words):
        ev = dec.decode(r)
        if len(ev):
            yield ev


def read_raw_words(path: str, chunk_words: int = 1 << 20):
    """Yields the records of a .dat file chunk by chunk, undecoded: for DeviceDatDecoder / process_dat_records."""
    with open(path, "rb") as f:
        blob = f.read()
    _, off = split_dat_header(blob, path)
    recs = np.frombuffer(blob, dtype=DAT_DTYPE, offset=off, count=(len(blob) - off) // DAT_DTYPE.itemsize)
    for a in range(0, len(recs), chunk_words):
        yield recs[a:a + chunk_words]


def write_raw(path: str, evs: np.ndarray, width: int = 640, height: int = 480):
    hdr = f"% Data file containing CD events.\n% Version 2\n% Height {height}\n% Width {width}\n".encode("ascii")
    with open(path, "wb") as f:
        f.write(hdr)
        f.write(bytes([EVENT_TYPE_CD, EVENT_SIZE]))
        f.write(encode_dat(evs).tobytes())


class DeviceDatDecoder(DeviceEvtDecoder):
    """The same decoder as three kernels (csrc/xmaps_dat.hpp): the records cross PCIe as the file stores them, the EventCD records
    stay on the device.  Same interface as evt3.DeviceEvt3Decoder (push: xm_ingest_push_dat); max_events = 0 means max_words."""

    _dtype, _create, _decode, _push = "<u8", "xm_dat_create", "xm_dat_decode", "xm_ingest_push_dat"

    def _as_words(self, records) -> np.ndarray:
        return as_records(records).view("<u8")
