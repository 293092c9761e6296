"""The packets of the device ingest's edge cases -- built once, shared by tests/test_ingest_edge_streams_cpu.py (which pins, with the
CPU oracle alone, the properties that take each case past a first trip of the kernels' loops) and tests/test_gpu_ingest_edges.py
(which feeds the very same packets to DeviceIngest).  Nothing here touches the GPU.

Numbers the cases are built around (x_maps_amd/csrc/xmaps_ingest.hpp): a block is ING_EPB = 512 packet events, ing_scan_blocks walks
the block records ING_THREADS = 256 at a time and finds a block's predecessor inside its wave of 64 blocks or through
group_last[], a packet has at most ING_MAX_BLOCKS = 4096 blocks, ing_find_trigger searches the pause ring 256 pairs at a time."""
from functools import lru_cache

import numpy as np

import ingest_oracle as IO
from x_maps_amd import synthetic as S

from ingest_helpers import (_cpu_chain, _dense_stream, _period_packets, _shifted, _sparse_stretch, _tiny_stream,
                            _with_negative_run)

EPB, MAX_BLOCKS = 512, 4096
T0 = 2_000_000


def n_blocks(packet):
    return (len(packet) + EPB - 1) // EPB


def _run_at(first_block, rest):
    """index at which a negative run starts so that `first_block` is the first block it empties and the run begins `rest` events
    before that block"""
    return first_block * EPB - rest


# ---- a. second trip of the block scan ------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def dense_packets(lead_us=1000):
    """7 frames of 140 000 + 520 events in packets of one period: every packet but the last has more than 256 blocks"""
    return tuple(_period_packets(_dense_stream(7, 140_000, seed=101), lead_us=lead_us))


@lru_cache(maxsize=None)
def dense_chain(lead_us=1000):
    return _cpu_chain(dense_packets(lead_us))


# ---- b. predecessor across groups and trips ------------------------------------------------------------------------------------------
RUN_GROUP, RUN_TWO_GROUPS, RUN_TRIP = 33_000, 70_000, 135_000  # > 64, > 128, > 256 blocks of 512


def _gap_index(packet, frame):
    """index of the first event of frame `frame` in the packet (the event behind the frame gap)"""
    return int(np.searchsorted(packet["t"], T0 + frame * 16_600))


@lru_cache(maxsize=None)
def negative_run_packets():
    """dense_packets() with runs of negative events (copies of the event they stand in front of):
      packet 0 (the stream's first: no tail): 33 000 at its very start; 33 000 inside frame 0
      packet 1: 33 000 (+ what aligns the next run) at its very start (predecessor: the stream's tail); 33 000 in the gap in front of frame 2
      packet 2: 135 000 inside frame 2; 70 000 in the gap in front of frame 3
      packet 3: 70 000 inside frame 3; 135 000 in the gap in front of frame 4
    A run inside a frame has events less than 40 us apart on both sides (no pause at the boundary); a run in a frame gap sits between
    the two events of the pause the trigger finder cuts at.  The runs of 33 000 start 100 events in front of a block whose number is
    no multiple of 64, so that they empty exactly 64 blocks."""
    pk = list(dense_packets())
    p = _with_negative_run(pk[0], 0, RUN_GROUP)
    pk[0] = _with_negative_run(p, _run_at(101, 100), RUN_GROUP)
    g = _gap_index(pk[1], 2)
    lead = RUN_GROUP + (-(g + RUN_GROUP) - 100) % EPB  # the gap run then starts 100 events in front of a block
    p = _with_negative_run(pk[1], 0, lead)
    pk[1] = _with_negative_run(p, _gap_index(p, 2), RUN_GROUP)
    p = _with_negative_run(pk[2], _run_at(37, 100), RUN_TRIP)
    pk[2] = _with_negative_run(p, _gap_index(p, 3), RUN_TWO_GROUPS)
    p = _with_negative_run(pk[3], _run_at(150, 100), RUN_TWO_GROUPS)
    pk[3] = _with_negative_run(p, _gap_index(p, 4), RUN_TRIP)
    return tuple(pk)


# ---- c. trigger search past 256 and 512 pauses ---------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def stretch_packets(n_stretch, frame_behind=True):
    """a sparse stretch of n_stretch events, 45 us behind it four (negative form: six) frames of 2600 + 520 positive events.
    frame_behind: the first packet runs from the stretch to 500 us into the second frame, so the first plausible pair of pauses
    is the n_stretch-th; else the first packet is the stretch and one more event alone: n_stretch pauses, none plausible, and the
    second runs to 500 us into the third frame (a buffer that starts with a frame holds two pauses only then).  Behind them packets
    of 900."""
    frames = _dense_stream(4 if frame_behind else 6, 2600, seed=103, neg=0)
    if frame_behind:
        stream = np.concatenate((_sparse_stretch(n_stretch, T0 - 45 * n_stretch), frames))
        first = int(np.searchsorted(stream["t"], T0 + 16_600 + 500))
        head = (stream[:first],)
    else:
        stream = np.concatenate((_sparse_stretch(n_stretch + 1, T0 - 45 * (n_stretch + 1)), frames))
        first = int(np.searchsorted(stream["t"], T0 + 2 * 16_600 + 500))
        head = (stream[:n_stretch + 1], stream[n_stretch + 1:first])
    return head + tuple(stream[a:a + 900] for a in range(first, len(stream), 900))


# ---- d. pause ring wrap ----------------------------------------------------------------------------------------------------------
PAUSE_CAP = dict(capacity_events=1 << 12, max_packet_events=1 << 11)  # pcap = 2 * capacity = 8192; room: one packet (ahead = 0)


@lru_cache(maxsize=None)
def pause_wrap_packets():
    """frames, 6000 pauses, frames, 6000 pauses, frames, 6000 pauses, frames: the pause ring of 8192 entries wraps twice.  The frames
    have ~1400 events, all positive (a negative one on the 25 us comb of so thin a frame would leave a pause inside it): more than the
    finder's 1000, and two packets of them fit a ring of 4096 while one stays within what the room rule leaves, 2048.  Stretches in
    packets of 2000 events, frames in packets of one period."""
    pk, t = [], T0
    for k in range(4):
        n_frames = 8 if k == 3 else 5
        pk += _period_packets(_shifted(_tiny_stream(n_frames, seed=110 + k, per_frame=900, neg=0, gap_noise=0), t - T0), t0=t)
        t += n_frames * 16_600
        if k < 3:
            s = _sparse_stretch(6000, t)
            pk += [s[a:a + 2000] for a in range(0, len(s), 2000)]
            t += 6000 * 45 + 45
            t += (-(t - T0)) % 16_600  # (frames stay on the 16 600 us grid: nothing depends on it)
    return tuple(pk)


# ---- e. a frame longer than the mirror -----------------------------------------------------------------------------------------------
MIRROR_CAP = dict(capacity_events=1 << 14, max_packet_events=1 << 11)  # mirror 8192; ahead = 2: room 3 * 2048


@lru_cache(maxsize=None)
def long_frame_packets():
    """14 frames at _tiny_stream's rate, the seventh replaced by one of 9500 + 520 events (~9000 positive: longer than the mirrored
    half of a ring of 16 384), in packets of one period cut into pieces of at most 2000 events"""
    tiny = _tiny_stream(14, seed=120, gap_noise=0)
    a, b = T0 + 6 * 16_600, T0 + 7 * 16_600
    big = _dense_stream(1, 9500, seed=121, t0=a)
    stream = np.concatenate((tiny[tiny["t"] < a], big, tiny[tiny["t"] >= b]))
    return tuple(p[a:a + 2000] for p in _period_packets(stream) for a in range(0, len(p), 2000))


# ---- f. activity filter on large packets ---------------------------------------------------------------------------------------------
def lattice_packet(n, seed, span_us, support=0.015, sort=True, start=1_000_000):
    """n positive events over span_us on C_TINY: most of them on the pixels with x % 3 == y % 3 == 0, which are no neighbours of one
    another, the rest (`support`) on the pixels between them.  An event on the lattice is kept only if one of the few supporting
    events hit a neighbour recently enough: about half of the flags are set, whatever the packet's density."""
    cfg = S.C_TINY
    rng = np.random.default_rng(seed)
    ev = np.zeros(n, S.EVENT_CD_DTYPE)
    t = rng.integers(0, span_us, n)
    ev["t"] = start + (np.sort(t) if sort else t)
    x, y = rng.integers(0, (cfg.cam_w + 2) // 3, n) * 3, rng.integers(0, cfg.cam_h // 3, n) * 3
    sup = rng.random(n) < support
    off = rng.integers(1, 9, n)  # one of the 8 cells of the 3 x 3 tile that are not its lattice pixel
    x = np.where(sup, np.minimum(x + off % 3, cfg.cam_w - 1), x)
    y = np.where(sup, y + off // 3, y)
    ev["x"], ev["y"], ev["p"] = x, y, 1
    return ev


@lru_cache(maxsize=None)
def backwards_packets():
    """dense_packets(1200) whose first packet (300 blocks) has the stamps of its second half 20 000 us earlier: more than a bucket
    of the default threshold, so the packet is judged sequentially, block after block"""
    pk = list(dense_packets(1200))
    bad = pk[0].copy()
    bad["t"][len(bad) // 2:] -= 20_000
    pk[0] = bad
    return tuple(pk)


def activity_chain(packets, thresh=int(1e6 / 60)):
    return _cpu_chain(packets, act=IO.ActivityFilterC(S.C_TINY.cam_w, S.C_TINY.cam_h, thresh))


# ---- g. the limit ------------------------------------------------------------------------------------------------------------------------
LIMIT = MAX_BLOCKS * EPB


@lru_cache(maxsize=None)
def limit_packets():
    """one packet of exactly 2 097 152 events, then packets of 900: six frames of 2600 + 520 positive events; those up to 500 us into
    the fourth frame go into the large packet, in pieces (cut at even steps and at the frame gaps) that start at blocks spread evenly
    over the packet -- the first in block 0, the last ends with the packet -- with negative events (copies of the positive one behind
    them) in between"""
    stream = _dense_stream(6, 2600, seed=130, neg=0)
    n = int(np.searchsorted(stream["t"], T0 + 3 * 16_600 + 500))
    pos = stream[:n]
    cuts = sorted(set(np.linspace(0, n, 10).astype(int).tolist()) | {_gap_index(pos, f) for f in (1, 2, 3)})
    where = np.zeros(n, np.int64)
    for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        first = (k * (MAX_BLOCKS - 2) // (len(cuts) - 2)) * EPB if k < len(cuts) - 2 else LIMIT - (b - a)
        where[a:b] = first + np.arange(b - a)
    src = np.minimum(np.searchsorted(where, np.arange(LIMIT), side="left"), n - 1)  # the positive event at or behind each place
    big = pos[src]
    big["p"] = 0
    big[where] = pos
    return (big,) + tuple(stream[a:a + 900] for a in range(n, len(stream), 900))
