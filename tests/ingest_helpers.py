"""What the device-ingest test modules share: the synthetic camera stream, its packets, the processor's parameters, a window
that keeps what it is shown, and the frame-by-frame comparison with the CPU oracle."""
import numpy as np

import xmaps_oracle as O
from x_maps_amd import synthetic as S


class Window:
    """the processor's window: appends every frame it is shown to `shown` (the frame itself, never a copy)"""

    def __init__(self, shown):
        self.shown = shown

    def should_close(self):
        return False

    def show_async(self, img):
        self.shown.append(img)


def _packets(stream, packet_us):
    edges = np.arange(stream["t"][0], stream["t"][-1] + packet_us, packet_us)
    cuts = np.searchsorted(stream["t"], edges)
    return [stream[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


def _tiny_stream(n_frames, seed, per_frame=2600, neg=0.1, gap_noise=3):
    cfg = S.C_TINY
    rng = np.random.default_rng(seed)
    chunks = []
    for f in range(n_frames):
        start = 2_000_000 + f * 16_600
        tt = np.unique(np.concatenate((np.sort(rng.integers(0, 13_000, per_frame)) + start, np.arange(start, start + 13_000, 25))))
        ev = np.zeros(len(tt), S.EVENT_CD_DTYPE)
        ev["t"] = tt
        ev["x"] = np.clip((tt - start) / 13_000 * cfg.cam_w + rng.normal(0, 1.5, len(tt)), 0, cfg.cam_w - 1).astype(np.uint16)
        ev["y"] = rng.integers(0, cfg.cam_h, len(tt))
        ev["p"] = rng.random(len(tt)) >= neg
        parts = [ev]
        if gap_noise and f % gap_noise == gap_noise - 1:
            nz = np.zeros(1, S.EVENT_CD_DTYPE)
            nz["t"], nz["x"], nz["y"], nz["p"] = start + 14_500, 5, 5, 1
            parts.append(nz)
        chunks.append(np.concatenate(parts))
    return np.concatenate(chunks)


def _frame_events(cfg, rng, tt, start, neg):
    """events at the stamps `tt` of the frame that starts at `start`: the column follows the scan, rows anywhere, a share negative"""
    ev = np.zeros(len(tt), S.EVENT_CD_DTYPE)
    ev["t"] = tt
    ev["x"] = np.clip((tt - start) / 13_000 * cfg.cam_w + rng.normal(0, 1.5, len(tt)), 0, cfg.cam_w - 1).astype(np.uint16)
    ev["y"] = rng.integers(0, cfg.cam_h, len(tt))
    ev["p"] = rng.random(len(tt)) >= neg
    return ev


def _dense_stream(n_frames, per_frame, seed, neg=0.1, t0=2_000_000):
    """_tiny_stream's frames without its limit of one event per microsecond: `per_frame` random stamps in 13 000 us (equal stamps
    allowed) plus the 25 us comb, so no pause inside a frame; frame starts 16 600 us apart, nothing between the frames"""
    cfg = S.C_TINY
    rng = np.random.default_rng(seed)
    chunks = []
    for f in range(n_frames):
        start = t0 + f * 16_600
        tt = np.sort(np.concatenate((rng.integers(0, 13_000, per_frame) + start, np.arange(start, start + 13_000, 25))))
        chunks.append(_frame_events(cfg, rng, tt, start, neg))
    return np.concatenate(chunks)


def _period_packets(stream, lead_us=1000, t0=2_000_000):
    """packets of one period of a stream whose frames start at t0 + k * 16 600, each ending `lead_us` into the next frame (the last
    one takes what is left).  Packets aligned to the frame starts, or of 2/3 or 1/2 a period, make the reference's finder lose lock
    on such a stream and cut nothing."""
    edges = np.arange(t0 + 16_600 + lead_us, stream["t"][-1] + 1, 16_600)
    cuts = np.concatenate(([0], np.searchsorted(stream["t"], edges), [len(stream)]))
    return [stream[a:b] for a, b in zip(cuts[:-1], cuts[1:]) if b > a]


def _with_negative_run(packet, at, n):
    """the packet with `n` negative events in front of event `at` (copies of it, same stamp: the stream stays sorted); they are
    events at + 0 .. at + n - 1 of the result"""
    run = packet[at:at + 1].repeat(n)
    run["p"] = 0
    return np.concatenate((packet[:at], run, packet[at:]))


def _sparse_stretch(n, t0, step_us=45):
    """`n` positive events `step_us` apart from t0 on: every gap is a pause, and no two consecutive pauses are half a period apart"""
    cfg = S.C_TINY
    ev = np.zeros(n, S.EVENT_CD_DTYPE)
    i = np.arange(n)
    ev["t"] = t0 + i * step_us
    ev["x"], ev["y"], ev["p"] = i % cfg.cam_w, (i // cfg.cam_w) % cfg.cam_h, 1
    return ev


def _shifted(stream, dt):
    out = stream.copy()
    out["t"] += dt
    return out


def _block_kept(packet, epb=512):
    """positive events per block of `epb` packet events (what k_ing_count's blocks keep with the polarity filter alone)"""
    pos = (packet["p"] == 1).astype(np.int64)
    pad = (-len(pos)) % epb
    return np.concatenate((pos, np.zeros(pad, np.int64))).reshape(-1, epb).sum(axis=1)


def _empty_runs(packet, min_blocks=1, epb=512):
    """[(index of the first block behind the run, the run's length in blocks)] for every run of >= min_blocks blocks that keep
    nothing (a run at the packet's end has no block behind it: its index is the block count)"""
    kept = _block_kept(packet, epb)
    out, b = [], 0
    while b < len(kept):
        if kept[b]:
            b += 1
            continue
        e = b
        while e < len(kept) and not kept[e]:
            e += 1
        if e - b >= min_blocks:
            out.append((e, e - b))
        b = e
    return out


def _pause_indices(evs, pause_us=40):
    """the trigger finder's pauses in a buffer of (positive) events"""
    return np.nonzero(np.diff(evs["t"]) >= pause_us)[0]


def _first_plausible_pair(evs, fps=60, pause_us=40):
    """index (into the buffer's pauses) of the first pair of consecutive pauses more than half a period apart, -1: none; and the
    number of pauses"""
    p = _pause_indices(evs, pause_us)
    gaps = evs["t"][p[1:]] - evs["t"][p[:-1]]
    hit = np.nonzero(gaps > 1e6 / fps / 2)[0]
    return (int(hit[0]) if len(hit) else -1), len(p)


def _cpu_chain(packets, fps=60, act=None):
    """the CPU chain over the very packets the device gets: (the finder, its buffer's length behind every packet, the positive --
    with `act`: kept -- events)"""
    import ingest_oracle as IO
    tf = IO.TriggerFinderOracle(fps)
    live, n_kept = [], 0
    for p in packets:
        kept = IO.polarity_filter(p)
        if act is not None:
            kept = act.process(kept)
        n_kept += len(kept)
        tf.process_events(kept)
        live.append(0 if tf.buf is None else len(tf.buf))
    return tf, live, n_kept


def _check_frames(tb, got, want_frames, camera=False, overflow=None):
    """overflow: what every frame's `overflow` must say, frame by frame (default: nothing was dropped)"""
    assert len(got) == len(want_frames), (len(got), len(want_frames))
    overflow = [0] * len(got) if overflow is None else overflow
    for fr, evs, ovf in zip(got, want_frames, overflow):
        assert (fr.n_events, fr.t_first, fr.t_last) == (len(evs), int(evs["t"][0]), int(evs["t"][-1])), (fr.seq, fr.lost, fr.overflow)
        x, y, t, _ = S.to_soa(evs)
        ref = O.process_ev_frame(tb, x.astype(np.int64), y.astype(np.int64), t, camera_perspective=camera)
        assert fr.n_inliers == int(ref["mask"].sum()) and fr.n_index_errors == 0 and not fr.lost and fr.overflow == ovf, (fr.seq, fr.overflow, ovf)
        assert np.array_equal(fr.depth, ref["depth"]) and np.array_equal(fr.bgr, ref["bgr"]), fr.seq


def _processor_params(tb, cfg=S.C_TINY, **kw):
    from x_maps_amd.depth_reprojection_processor import RuntimeParams
    args = dict(camera_width=cfg.cam_w, camera_height=cfg.cam_h, projector_width=cfg.proj_w, projector_height=cfg.proj_h,
                projector_fps=60, z_near=0.1, z_far=1.2, calib=None, projector_time_map=None, no_frame_dropping=True,
                camera_perspective=False, tables=tb)
    args.update(kw)
    return RuntimeParams(**args)
