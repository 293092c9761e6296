"""Frames for the frame -> EVT 3.0 entry (xm_frames_to_evt3_words, the ingest's record stage) and the rule itself, restated.

The oracle of every test is the host encoder, x_maps_amd.evt3.encode_evt3 (use_vectors off: encode_evt3_singles).  `restate` is the
parallel form of the rule as include/xmaps.h spells it (links -> chains -> run starts -> the words in front of a run start): NumPy on
whole arrays, with one walk per chain head like the kernel's.  tests/test_evt3_record_cases_cpu.py holds the two against each other
and shows that every case below reaches what its name claims; tests/test_gpu_evt3_record.py runs the cases on the device.

Kernel geometry the cases cross (csrc/xmaps_evt3enc.hpp, csrc/xmaps_frameacc.hpp): 64 events per word count (one wave
instruction), 1 024 events per block and trip of the chunk loops, 32 frames per launch sequence, and 1 024 threads in the scan
block, each taking ceil(segments / 1 024) consecutive 64-event counts."""
import functools

import numpy as np

from x_maps_amd import evt3
from x_maps_amd.synthetic import EVENT_CD_DTYPE

SEGMENT, CHUNK, GROUP, SCAN_BLOCK = 64, 1024, 32, 1024
RUN_COLS = 12
STAT_FIELDS = ("n_events", "n_words", "n_vector_runs", "n_out_of_range", "t_first", "t_last")
# the scan block's threads take more than one count each from SCAN_BLOCK * SEGMENT + 1 = 65 537 events on: this frame has 1 028
# counts, two per thread (the last threads none), the last count of 37 events
BIG_FRAME_EVENTS = SCAN_BLOCK * SEGMENT + 3 * SEGMENT + 37


def events(x, y, p, t):
    x = np.asarray(x)
    ev = np.zeros(len(x), EVENT_CD_DTYPE)
    ev["x"], ev["y"], ev["p"], ev["t"] = x, y, p, t
    return ev


def concat(frames, lead=0):
    """(one record array with `lead` foreign records in front, u64 offsets [n + 1] into it)"""
    offs = np.zeros(len(frames) + 1, np.uint64)
    offs[1:] = np.cumsum([len(f) for f in frames])
    offs += np.uint64(lead)
    evs = np.zeros(int(offs[-1]), EVENT_CD_DTYPE)
    evs[:lead] = events(np.arange(lead) % 7, 3, 1, 5)
    for f, a in zip(frames, offs[:-1]):
        evs[int(a):int(a) + len(f)] = f
    return evs, offs


def oracle(evs, use_vectors=True):
    """the host encoder's words and the statistics they imply"""
    words = evt3.encode_evt3(evs, True) if use_vectors else evt3.encode_evt3_singles(evs)
    x, y, p, t = (evs[k].astype(np.int64) for k in ("x", "y", "p", "t"))
    oor = (x > 2047) | (y > 2047) | ((p != 0) & (p != 1)) | (t < 0)
    st = dict(n_events=len(evs), n_words=len(words), n_vector_runs=int(((words >> 12) == evt3.T_VECT_BASE_X).sum()),
              n_out_of_range=int(oor.sum()), t_first=int(t[0]) if len(evs) else 0, t_last=int(t[-1]) if len(evs) else 0)
    return words.astype(np.uint16), st


# ---- the rule in its parallel form ----------------------------------------------------------------------------------------------

def links(evs, use_vectors=True):
    """linked[i]: event i >= 1 is linked to event i - 1"""
    x, y, p, t = (evs[k].astype(np.int64) for k in ("x", "y", "p", "t"))
    out = np.zeros(len(evs), bool)
    if use_vectors and len(evs) > 1:
        out[1:] = (t[1:] == t[:-1]) & (y[1:] == y[:-1]) & (p[1:] == p[:-1]) & (x[1:] > x[:-1])
    return out


def run_starts(evs, use_vectors=True):
    """(start[i], bits[i]): is event i a run start, and its run's VECT_12 bits (bit 0 = the start itself)"""
    n = len(evs)
    x = evs["x"].astype(np.int64)
    linked = links(evs, use_vectors)
    start, bits = np.zeros(n, bool), np.zeros(n, np.int64)
    for head in np.nonzero(~linked)[0]:  # one walk per chain, as one lane per chain head
        cur = int(head)
        while True:
            start[cur], bits[cur] = True, 1
            j = cur + 1
            while j < n and linked[j] and x[j] - x[cur] < RUN_COLS:
                bits[cur] |= 1 << int(x[j] - x[cur])
                j += 1
            assert j <= cur + RUN_COLS
            if j >= n or not linked[j]:
                break
            cur = j  # next(cur)
    return start, bits


def restate(evs, use_vectors=True):
    """the frame's words from the parallel form: per-event word counts, an exclusive scan, every word placed by its event"""
    n = len(evs)
    if n == 0:
        return np.zeros(0, np.uint16)
    x, y, p, t = (evs[k].astype(np.int64) for k in ("x", "y", "p", "t"))
    hi, lo = (t >> 12) & 0xfff, t & 0xfff
    start, bits = run_starts(evs, use_vectors)
    first = np.arange(n) == 0
    w_hi = start & (first | (hi != np.roll(hi, 1)))
    w_lo = start & (w_hi | (lo != np.roll(lo, 1)))
    w_y = start & (first | (y != np.roll(y, 1)))
    vect = start & (bits != 1)
    per = w_hi.astype(np.int64) + w_lo + w_y + start + vect
    off = np.cumsum(per) - per
    words = np.zeros(int(per.sum()), np.int64)
    pos = off.copy()
    for mask, val in ((w_hi, (evt3.T_TIME_HIGH << 12) | hi), (w_lo, (evt3.T_TIME_LOW << 12) | lo), (w_y, (evt3.T_ADDR_Y << 12) | (y & 0x7ff))):
        words[pos[mask]] = val[mask]
        pos = pos + mask
    xp = ((p & 1) << 11) | (x & 0x7ff)
    single = start & ~vect
    words[pos[single]] = ((evt3.T_ADDR_X << 12) | xp)[single]
    words[pos[vect]] = ((evt3.T_VECT_BASE_X << 12) | xp)[vect]
    words[pos[vect] + 1] = ((evt3.T_VECT_12 << 12) | bits)[vect]
    return words.astype(np.uint16)


# ---- the cases ------------------------------------------------------------------------------------------------------------------

def _filler(n, seed, t0=5_000_000):
    """n unlinked events: the stamp grows by one per event"""
    rng = np.random.default_rng(seed)
    return events(rng.integers(0, 640, n), rng.integers(0, 480, n), 1, t0 + np.arange(n))


def _row(x, y=7, p=1, t=6_000_000):
    return events(x, y, p, t)


def _cat(*parts):
    return concat(list(parts))[0]


def clustered(rng, n, t0=3_000_000, wide=False):
    """a random stream in which links, chains and runs of every length occur: stamps that mostly repeat, a few rows, column
    steps of -2 .. 13 (wide: fields beyond the format's range as well)"""
    t = t0 + np.cumsum(rng.choice([0, 0, 0, 0, 1, 4096, 1 << 24], n, p=[.3, .2, .2, .1, .15, .04, .01]))
    y = (np.cumsum(rng.random(n) < 0.15) * 7) % 480  # the row changes now and then
    step = rng.choice([-2, 0, 1, 1, 1, 2, 3, 5, 11, 12, 13], n)
    x = np.cumsum(step) % (4096 if wide else 640)
    p = np.where(rng.random(n) < 0.1, 0, 1)
    if wide:
        p = np.where(rng.random(n) < 0.05, rng.integers(-3, 4, n), p)
        y = np.where(rng.random(n) < 0.05, y + 2048, y)
        t = np.where(rng.random(n) < 0.02, -t, t)
    return events(x, y, p, t)


@functools.lru_cache(maxsize=None)
def cases():
    """{name: frame}; what each is for is asserted in tests/test_evt3_record_cases_cpu.py"""
    c = {}
    c["empty"] = events([], [], [], [])
    for n in (1, 63, 64, 65):
        c[f"n{n}"] = _filler(n, n)
    c["run1"] = _row([5])
    c["run2"] = _row([5, 6])
    c["run12"] = _row(np.arange(100, 112))
    c["gap11"] = _row([30, 41])          # the same run: bit 11
    c["gap12"] = _row([30, 42])          # a new run
    c["equal_x"] = _row([9, 9, 10])
    c["decreasing_x"] = _row([9, 8, 7, 20])
    c["break_p"] = events([1, 2, 3, 4], 7, [1, 1, 0, 0], 6_000_000)
    c["break_y"] = events([1, 2, 3, 4], [7, 7, 8, 8], 1, 6_000_000)
    c["break_t1"] = events([1, 2, 3, 4], 7, 1, [50, 50, 51, 51])
    c["break_t24"] = events([1, 2, 3, 4], 7, 1, [50, 50, 50 + (1 << 24), 50 + (1 << 24)])  # not linked, and no time word between them
    c["hi_change_lo_equal"] = events([1, 2, 300], 7, 1, [(3 << 12) | 77, (4 << 12) | 77, (4 << 12) | 77])
    # a chain of 310 consecutive columns (26 runs) from event 874 on: it straddles the 64-event counts at 896, 960, ... and the
    # block boundary at event 1 024
    c["long_chain"] = _cat(_filler(874, 11), _row(np.arange(200, 510)), _filler(90, 12, t0=7_000_000))
    # a chain that ends on event 63, the last of its count; the next count starts with an unlinked event in the same row
    c["chain_ends_segment"] = _cat(_filler(58, 13), _row(np.arange(40, 46)), _row([3], t=6_000_001), _filler(20, 14, t0=7_000_000))
    # a run that straddles two counts (events 60 .. 67)
    c["run_straddles_segment"] = _cat(_filler(60, 15), _row(np.arange(40, 48)), _filler(30, 16, t0=7_000_000))
    c["out_of_range"] = events([2047, 2048, 4000, 65535, 5, 6, 7, 8], [1, 1, 2047, 2048, 65535, 3, 3, 3], [1, 1, 1, 1, 1, 2, -1, 1],
                               [10, 10, 10, 10, 10, 10, 10, -5])
    c["wide_random"] = clustered(np.random.default_rng(21), 700, wide=True)
    c["random_3572"] = clustered(np.random.default_rng(22), 3572)  # four blocks, or (XM_ENC_MAX_BLOCKS = 1) four trips of one
    for v in c.values():
        v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def big_frame():
    """BIG_FRAME_EVENTS events: the per-frame scan's threads take two counts each"""
    ev = clustered(np.random.default_rng(23), BIG_FRAME_EVENTS)
    ev.setflags(write=False)
    return ev


def group(n_frames):
    """(names, frames): n_frames frames drawn from the cases in turn (the empty frame among them)"""
    names = [k for k in cases() if k != "random_3572"]
    pick = [names[(5 * i + 3) % len(names)] for i in range(n_frames)]
    return pick, [cases()[k] for k in pick]
