"""-m gpu: a slot handed from one way in to the next.  With n_slots = 2 every slot's key frame and state are used in turn by eager
frames (the slot's own stream), groups (a stream per group, in rotation) and graph replays (the graphs' origin stream); the only
thing that keeps them apart is the slot's ordering record (x_maps_amd/csrc/host/xm_slot_order.hpp) -- a missing wait is a race
between two of them.  Nothing synchronises between the steps; every frame's depth and BGR equal the CPU oracle bit for bit.
Also what xm_graph_create leaves behind: a slot's last-frame record as it was before the capture, and offsets that decrease
refused as xm_process_batch refuses them."""
import numpy as np
import pytest

from conftest import xm_option

import xmaps_oracle as O
from x_maps_amd import XMapsEngine
from x_maps_amd import synthetic as S

pytestmark = pytest.mark.gpu

CFG = S.C_TINY
N_FRAMES = 9  # 2 eager, a group of 2, a graph of 2, 1 eager, a group of 2
SHUFFLED = 2  # the group's first frame, for the run that shuffles one


def _oracle(tb, cols):
    x, y, t = cols
    return O.process_ev_frame(tb, x.astype(np.int64), y.astype(np.int64), t)


@pytest.fixture(scope="module")
def rig():
    tb = S.make_tables(CFG)
    frames = [S.to_soa(S.make_events(CFG, frame=f, n=4000 + 13 * f))[:3] for f in range(N_FRAMES)]  # (lengths differ: last_frame_stats)
    perm = np.random.default_rng(17).permutation(len(frames[SHUFFLED][2]))
    shuffled = tuple(np.ascontiguousarray(c[perm]) for c in frames[SHUFFLED])
    assert shuffled[2][0] != shuffled[2].min() and shuffled[2][-1] != shuffled[2].max()  # (the shortcut cannot hold)
    return tb, frames, [_oracle(tb, c) for c in frames], shuffled, _oracle(tb, shuffled)


class _Batch:
    """frames as device columns, one after the other, + their outputs"""

    def __init__(self, eng, frames):
        self.eng, self.n = eng, [len(c[2]) for c in frames]
        self.offs = np.concatenate([[0], np.cumsum(self.n)]).astype(np.uint64)
        self.x, self.y, self.t = (eng.to_device(np.concatenate([c[k] for c in frames])) for k in range(3))
        self.px = eng.out_h * eng.out_w
        self.depth, self.bgr = eng.dev_alloc(len(frames) * self.px * 4), eng.dev_alloc(len(frames) * self.px * 3)
        eng.dev_upload(self.depth, np.full(len(frames) * self.px, -1.0, np.float32))
        eng.dev_upload(self.bgr, np.full(len(frames) * self.px * 3, 7, np.uint8))

    def ptrs(self, f):
        a = int(self.offs[f])
        return self.x + 2 * a, self.y + 2 * a, self.t + 8 * a, self.depth + 4 * f * self.px, self.bgr + 3 * f * self.px

    def eager(self, f):
        x, y, t, d, b = self.ptrs(f)
        self.eng.process_frame_device(x, y, t, None, self.n[f], d, b)

    def group_args(self, f0, n):
        x, y, t, d, b = self.ptrs(f0)
        return x, y, t, None, self.offs[f0:f0 + n + 1] - self.offs[f0], d, b

    def results(self):
        e = self.eng
        depth, bgr = np.empty((len(self.n), e.out_h, e.out_w), np.float32), np.empty((len(self.n), e.out_h, e.out_w, 3), np.uint8)
        e.dev_download(depth, self.depth)
        e.dev_download(bgr, self.bgr)
        return depth, bgr

    def free(self):
        for p in (self.x, self.y, self.t, self.depth, self.bgr):
            self.eng.dev_free(p)


@pytest.mark.parametrize("variant", ["plain", "launch_workers", "one_frame_shuffled"])
def test_eager_frames_groups_and_graph_replays_share_two_slots(rig, variant):
    tb, frames, refs, shuffled, shuffled_ref = rig
    if variant == "one_frame_shuffled":
        frames, refs = list(frames), list(refs)
        frames[SHUFFLED], refs[SHUFFLED] = shuffled, shuffled_ref
    with XMapsEngine(tb, n_slots=2, launch_workers=variant == "launch_workers") as eng:
        b = _Batch(eng, frames)
        b.eager(0)
        b.eager(1)
        eng.process_batch_device(*b.group_args(2, 2))
        g = eng.graph_create(*b.group_args(4, 2))
        g.launch()
        g.launch()
        b.eager(6)
        eng.process_batch_device(*b.group_args(7, 2))
        st = eng.last_frame_stats()
        eng.sync()
        depth, bgr = b.results()
        fallbacks = eng.sorted_fallbacks()
        g.close()
        b.free()
    assert st.n_events == len(frames[8][2]) and st.n_inliers == int(refs[8]["mask"].sum())
    for f in range(N_FRAMES):
        assert np.array_equal(depth[f], refs[f]["depth"]) and np.array_equal(bgr[f], refs[f]["bgr"]), f
    assert fallbacks == (1 if variant == "one_frame_shuffled" else 0)


def _failing_frames_then_sorted_ones(tb, frames, refs, capture_between):
    """four shuffled eager frames on ONE slot, then two sorted ones: -> path_counts, all results equal the oracle"""
    with XMapsEngine(tb, n_slots=1) as eng:
        b = _Batch(eng, frames)
        for f in range(len(frames)):
            b.eager(f)
            if f == 0:
                assert eng.path_counts()["cols"] == 1  # (the frames are dense enough for the column tiles)
            if capture_between and f < 4:  # a capture between a frame and the verdict on it
                eng.graph_create(*b.group_args(5, 1)).close()
        eng.sync()
        depth, bgr = b.results()
        pc = eng.path_counts()
        b.free()
    for f in (0, 1, 2, 3, 4):  # (frame 5's outputs: the graph was never launched, the eager frame wrote them last)
        assert np.array_equal(depth[f], refs[f]["depth"]) and np.array_equal(bgr[f], refs[f]["bgr"]), f
    assert np.array_equal(depth[5], refs[5]["depth"]) and np.array_equal(bgr[5], refs[5]["bgr"])
    return pc


def test_graph_create_leaves_the_slots_last_frame_record_alone():
    """A frame that failed on the column tiles counts against the compact paths when its verdict is read (resolve_prev reads the
    slot's last-frame record: did it take a compact path?).  A capture between the frame and its verdict must not change that:
    four failures in a row pause the compact paths with or without captures in between, so the sorted frames that follow take
    the same path in both runs.  (The capture's own frame is counted once per capture, under "general": path_counts counts
    frames enqueued, captured ones too.)"""
    xm_option("XM_COLS", "2")
    tb = S.make_tables(CFG)
    rng = np.random.default_rng(5)
    frames = []
    for f in range(6):
        cols = S.to_soa(S.make_events(CFG, frame=20 + f, n=6000))[:3]
        if f < 4:
            perm = rng.permutation(6000)
            cols = tuple(np.ascontiguousarray(c[perm]) for c in cols)
        frames.append(cols)
    refs = [_oracle(tb, c) for c in frames]
    base = _failing_frames_then_sorted_ones(tb, frames, refs, False)
    assert base["cols"] == 4 and base["general"] == 4 and base["sorted_key64"] + base["key32"] == 2  # (paused: no tiles for the last two)
    with_capture = _failing_frames_then_sorted_ones(tb, frames, refs, True)
    assert with_capture == dict(base, general=base["general"] + 4)


def test_graph_create_refuses_offsets_that_decrease(rig):
    tb, frames, _, _, _ = rig
    with XMapsEngine(tb, n_slots=2) as eng:
        b = _Batch(eng, frames[:2])
        x, y, t, d, bg = b.ptrs(0)
        with pytest.raises(ValueError, match="non-decreasing"):
            eng.graph_create(x, y, t, None, [0, 10, 5], d, bg)
        b.free()
