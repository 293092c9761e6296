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


def _check_frames(tb, got, want_frames, camera=False):
    assert len(got) == len(want_frames), (len(got), len(want_frames))
    for fr, evs in zip(got, want_frames):
        assert (fr.n_events, fr.t_first, fr.t_last) == (len(evs), int(evs["t"][0]), int(evs["t"][-1])), (fr.seq, fr.lost, fr.overflow)
        x, y, t, _ = S.to_soa(evs)
        ref = O.process_ev_frame(tb, x.astype(np.int64), y.astype(np.int64), t, camera_perspective=camera)
        assert fr.n_inliers == int(ref["mask"].sum()) and fr.n_index_errors == 0 and not fr.lost and fr.overflow == 0
        assert np.array_equal(fr.depth, ref["depth"]) and np.array_equal(fr.bgr, ref["bgr"]), fr.seq


def _processor_params(tb, cfg=S.C_TINY, **kw):
    from x_maps_amd.depth_reprojection_processor import RuntimeParams
    args = dict(camera_width=cfg.cam_w, camera_height=cfg.cam_h, projector_width=cfg.proj_w, projector_height=cfg.proj_h,
                projector_fps=60, z_near=0.1, z_far=1.2, calib=None, projector_time_map=None, no_frame_dropping=True,
                camera_perspective=False, tables=tb)
    args.update(kw)
    return RuntimeParams(**args)
