"""The streams, chunkings and CPU chain of the triggered frames' two filters (tests/test_gpu_trigger_filters.py,
tests/test_gpu_trigger_frame_filters.py, tests/test_gpu_trigger_pipe_filters.py); pinned without a GPU by
tests/test_trigger_filter_cases_cpu.py.

Expected = the word-by-word checker (ext_trigger_ref.machine) -> p == 1 on the sensor -> the activity rule over the WHOLE stream
(oracle/ingest_oracle.py: ActivityFilterOracle, or its C form for long streams) -> ext_trigger.keep_where -> TriggerFrameCutter.

Stream A is the recipe of tests/test_gpu_trigger_pipe.py::_stream: six frames of the 64 x 48 synthetic rig, a fifth of the events
negative, a trigger in front of every frame and behind the last."""
import functools

import numpy as np

import ext_trigger_ref as R
import ingest_oracle as IO
from x_maps_amd import evt2, evt21, evt3
from x_maps_amd import ext_trigger as X
from x_maps_amd import synthetic as S

CFG = S.C_TINY
ENCODE = {3: evt3.encode_evt3, 2: evt2.encode_evt2, 21: evt21.encode_evt21}
N_EVENTS = (3000, 2600, 800, 3400, 2900, 3100)  # per frame, both polarities
N_POSITIVE = 12_671
ACT_NB = 8                                      # xmaps_ingest.hpp: buckets of T + 1 us a chunk may span on the parallel path
MIN_EVENTS = 1000                               # the pipe's MIN_EVENTS_PER_FRAME
# T -> (kept of the whole stream, positive kept per frame, frames shown, frames skipped); None where the issue states nothing
TABLE = {16_666: (12_150, None, None, None),
         500: (9_586, (1876, 1514, 236, 2228, 1804, 1928), 5, 1),
         200: (None, (1285, 991, 127, 1594, 1228, 1320), 4, 2)}


@functools.lru_cache(maxsize=None)
def stream_a(fmt):
    """-> (words, the events as encoded)"""
    parts = [S.make_events(CFG, frame=f, n=n, p_zero_fraction=0.2, t0=5_000_000 + f * 16_600) for f, n in enumerate(N_EVENTS)]
    evs = np.zeros(sum(N_EVENTS), S.EVENT_CD_DTYPE)
    starts = np.concatenate(([0], np.cumsum(N_EVENTS)))
    for a, p in zip(starts, parts):
        evs[a:a + len(p)] = p
    at, ids, vals = [], [], []
    for a in starts:
        at += [int(a), int(a), int(min(a + 500, len(evs)))]
        ids += [1, 0, 0]      # another channel's pulse, THE trigger, its falling edge
        vals += [1, 1, 0]
    return X.insert_ext_triggers(ENCODE[fmt](evs), fmt, at, ids, vals), evs


def one_chunk(words):
    return [words]


def uneven_chunks(words):
    """the five uneven chunks of tests/test_gpu_trigger_pipe.py (one of them holds several closing triggers)"""
    cuts = [0, len(words) // 7, len(words) // 3, len(words) // 3 + 1, len(words) // 2, len(words)]
    return [words[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


def chunks_spanning_under(words, fmt, span_us, piece=32):
    """consecutive pieces of `piece` words, merged greedily for as long as the chunk's decoded records span less than span_us (a
    piece of its own that spans more stays alone: the caller asserts what it needs)"""
    dec = X.ExtTriggerExtractor(fmt)
    out, cur_a, t_first, t_last = [], 0, None, None
    for a in range(0, len(words), piece):
        ev, _ = dec.extract(words[a:a + piece])
        if len(ev):
            lo, hi = int(ev["t"].min()), int(ev["t"].max())
            if t_first is not None and max(hi, t_last) - min(lo, t_first) >= span_us:
                out.append(words[cur_a:a])
                cur_a, t_first, t_last = a, None, None
            t_first = lo if t_first is None else min(t_first, lo)
            t_last = hi if t_last is None else max(t_last, hi)
    out.append(words[cur_a:])
    return [c for c in out if len(c)]


def takes_sequential_path(ev, thresh_us) -> bool:
    """k_act_first's proviso (xmaps_ingest.hpp), restated: a chunk of decoded records `ev` (ALL of them, whatever their polarity)
    stays on the parallel path iff no stamp lies in front of the chunk's first, all lie inside ACT_NB buckets of thresh_us + 1 us
    counted from it, and the bucket numbers never fall along the chunk"""
    if len(ev) == 0:
        return False
    t = ev["t"].astype(np.int64)
    d = t - t[0]
    w = int(thresh_us) + 1
    if (d < 0).any() or (d >= w * ACT_NB).any():
        return True
    b = d // w
    return bool((np.diff(b) < 0).any())


def act_mask(oracle, ev, cam_w=CFG.cam_w, cam_h=CFG.cam_h):
    """the keep mask of a chunk's records under the stateful `oracle` (ActivityFilterOracle / ActivityFilterC): p == 1, on the
    sensor, kept by the rule.  The oracle returns events, not flags: the records go in 32 767 at a time with their index in `p`,
    which the rule does not read."""
    mask = np.zeros(len(ev), bool)
    idx = np.nonzero((ev["p"] == 1) & (ev["x"] < cam_w) & (ev["y"] < cam_h))[0]
    for a in range(0, len(idx), 32767):
        part = idx[a:a + 32767]
        sub = np.zeros(len(part), S.EVENT_CD_DTYPE)
        sub[:] = ev[part]
        sub["p"] = np.arange(len(part))
        kept = oracle.process(sub)
        mask[part[kept["p"].astype(np.int64)]] = True
    return mask, len(idx)


def decoded_chunks(fmt, chunks):
    """[(events, triggers)] of the chunks, by the word-by-word checker"""
    ref = R.machine(fmt)
    return [ref.feed(c) for c in chunks]


class Chain:
    """The CPU chain, chunk by chunk: feed(events, triggers) of the checker -> the cutter's ready count; drain() -> the frames that
    became ready, released.  thresh_us None: polarity only (today's chain)."""

    def __init__(self, thresh_us, include_self=False, c_form=False, cam=(CFG.cam_w, CFG.cam_h), **cut_cfg):
        self.cut = X.TriggerFrameCutter(**cut_cfg)
        self.cam = cam
        self.thresh, self.include_self, self.c_form = thresh_us, include_self, c_form
        self.n_positive = self.n_active = self.n_sequential = 0
        self.kept = []  # per chunk: (kept events, remapped triggers)
        self.reset_history()

    def reset_history(self):
        self.oracle = None
        if self.thresh is not None:
            self.oracle = (IO.ActivityFilterC if self.c_form else IO.ActivityFilterOracle)(self.cam[0], self.cam[1], self.thresh, self.include_self)

    def feed(self, ev, tr) -> int:
        if self.oracle is None:
            mask = ev["p"] == 1
        else:
            mask, _ = act_mask(self.oracle, ev, *self.cam)
            self.n_positive += int((ev["p"] == 1).sum())
            self.n_active += int(mask.sum())
            self.n_sequential += takes_sequential_path(ev, self.thresh)
        kept, trk = X.keep_where(ev, tr, mask)
        self.kept.append((kept, trk))
        return self.cut.push(kept, trk, n_in=len(ev))

    def drain(self):
        got = []
        while True:  # (a skipped frame ends a run)
            more = self.cut.ready()
            if not more:
                return got
            self.cut.release(len(more))
            got += more


def expected(decoded, thresh_us, include_self=False, c_form=False, **cut_cfg):
    """The CPU chain over decoded chunks [(events, triggers)] -> dict(frames=[(events, opening trigger)], per_chunk=[frames closed],
    kept, n_positive, n_active, n_sequential, cutter)"""
    ch = Chain(thresh_us, include_self, c_form, **cut_cfg)
    frames, per_chunk = [], []
    for ev, tr in decoded:
        ch.feed(ev, tr)
        got = ch.drain()
        frames += got
        per_chunk.append(len(got))
    return dict(frames=frames, per_chunk=per_chunk, kept=ch.kept, n_positive=ch.n_positive, n_active=ch.n_active,
                n_sequential=ch.n_sequential, cutter=ch.cut)
