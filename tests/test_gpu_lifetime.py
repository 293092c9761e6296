"""-m gpu: what a create / destroy cycle of every object of the library leaves behind on the device.

One process creates and destroys, N times over and through the public API in the documented order: an engine on the C-1M rig and
one on the owner-tile rig (projector view), an ingest with the activity filter on, an EVT 3.0 decoder in front of it, and a graph
batch; each gets a few packets / frames pushed through.  The device's free memory after cycle 2 is compared with the one after
cycle N: the first cycles pay for what stays for the life of the process on purpose (the HIP runtime's own pools, the code
objects, the ingest's per-device stream set), the later ones must not add to it.

What it cannot see: torch.cuda.mem_get_info reports device memory at the allocator's page granularity, so a leak of a few bytes
per cycle shows only once it crosses a page (hence N = 100), and leaked events, streams or pinned host memory do not show at
all.  Those are guarded by construction (every such resource is a member with a destructor: csrc/host/xm_res.hpp), not by this test."""
import time

import numpy as np
import pytest

from x_maps_amd import XMapsEngine, evt3
from x_maps_amd import synthetic as S
from x_maps_amd.ingest import DeviceIngest

pytestmark = pytest.mark.gpu

N_CYCLES = 100  # a cycle was measured at 0.06 s on an MI355X (the first one, which loads the code objects, at 0.3 s): about 6 s
# Bytes of free device memory that cycles 3 .. N may take.  The library as it was before its resources had owners (raw pointers,
# released field by field in the destroy functions) showed a drift of 0 bytes in this test, with this N -- so must this one.
MAX_DRIFT_BYTES = 0


def _tiny_stream(n_frames, seed):
    """frames of a 60 Hz projector: a 13 ms scan (an event at least every 25 us), 3.6 ms of silence, 10 % negative events"""
    cfg = S.C_TINY
    rng = np.random.default_rng(seed)
    chunks = []
    for f in range(n_frames):
        start = 2_000_000 + f * 16_600
        tt = np.unique(np.concatenate((np.sort(rng.integers(0, 13_000, 2600)) + start, np.arange(start, start + 13_000, 25))))
        ev = np.zeros(len(tt), S.EVENT_CD_DTYPE)
        ev["t"] = tt
        ev["x"] = np.clip((tt - start) / 13_000 * cfg.cam_w + rng.normal(0, 1.5, len(tt)), 0, cfg.cam_w - 1).astype(np.uint16)
        ev["y"] = rng.integers(0, cfg.cam_h, len(tt))
        ev["p"] = rng.random(len(tt)) >= 0.1
        chunks.append(ev)
    return np.concatenate(chunks)


def _packets(stream, packet_us):
    cuts = np.searchsorted(stream["t"], np.arange(stream["t"][0], stream["t"][-1] + packet_us, packet_us))
    return [stream[a:b] for a, b in zip(cuts[:-1], cuts[1:]) if b > a]


def _cycle(torch, work):
    # 1. engines: column tiles (C-1M) and owner tiles (several time columns per frame cell), projector view, a group of frames each
    for tables, frames, mode in ((work["tb_1m"], work["ev_1m"], "cols"), (work["tb_own"], work["ev_own"], "own")):
        with XMapsEngine(tables, n_slots=len(frames), device=0) as eng:
            out = eng.process_event_frames(frames)
            assert eng.cols_info()["mode"] == mode and len(out) == len(frames)
            depth, _, st = eng.process_events(frames[0])
            assert st.n_inliers > 0 and depth.shape == (tables["proj_h"], tables["proj_w"])
    # 2. the ingest with the activity filter on: records pushed packet by packet
    with XMapsEngine(work["tb_tiny"], device=0) as eng, \
            DeviceIngest(eng, 60, activity_filter=True, capacity_events=1 << 16, max_packet_events=1 << 13, result_ring=16) as ing:
        for p in work["packets"]:
            ing.push(p)
        ing.flush()
        n_records = len(ing.poll())
    assert n_records >= 4
    # 3. the EVT 3.0 decoder in front of an ingest: the same stream as raw words
    with XMapsEngine(work["tb_tiny"], device=0) as eng:
        ing = DeviceIngest(eng, 60, activity_filter=True, capacity_events=1 << 16, max_packet_events=1 << 13, result_ring=16)
        with evt3.DeviceEvt3Decoder(eng, max_words=max(len(c) for c in work["chunks"])) as dec:
            for words, p in zip(work["chunks"], work["packets"]):
                assert dec.push(ing, words) == len(p)
            ing.flush()
            assert len(ing.poll()) == n_records
        ing.close()
    # 4. a graph batch: captured, replayed twice, destroyed before its engine
    F, cfg = 4, S.C_TINY
    x, y, t, _ = S.to_soa(np.concatenate([S.make_events(cfg, frame=f) for f in range(F)]))
    dev = torch.device("cuda", 0)
    X, Y, T = (torch.from_numpy(a).to(dev) for a in (x.view(np.int16), y.view(np.int16), t))
    depth = torch.zeros((F, cfg.proj_h, cfg.proj_w), dtype=torch.float32, device=dev)
    bgr = torch.zeros((F, cfg.proj_h, cfg.proj_w, 3), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    offs = np.arange(F + 1, dtype=np.uint64) * cfg.n_events
    with XMapsEngine(work["tb_tiny"], n_slots=F, default_priority_streams=True, device=0) as eng:
        g = eng.graph_create(X.data_ptr(), Y.data_ptr(), T.data_ptr(), None, offs, depth.data_ptr(), bgr.data_ptr())
        for _ in range(2):
            g.launch()
            eng.sync()
        assert float(depth.max()) > 0
        g.close()
    del X, Y, T, depth, bgr


def _free_bytes(torch):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()  # (the test's own tensors go back to the device: only the library's allocations remain)
    return torch.cuda.mem_get_info(0)[0]


def test_create_destroy_cycles_leave_no_device_memory_behind():
    torch = pytest.importorskip("torch")
    stream = _tiny_stream(8, seed=3)
    packets = _packets(stream, int(1e6 / 60 / 4))  # a quarter of a period per packet, like a camera's
    work = {
        "tb_1m": S.make_tables(S.C_1M), "ev_1m": [S.make_events(S.C_1M, frame=f, n=200_000) for f in (1, 2)],
        "tb_own": S.make_tables_shared_cells(), "ev_own": [S.make_events(S.C_SHARED, frame=f) for f in (1, 2)],
        "tb_tiny": S.make_tables(S.C_TINY), "packets": packets, "chunks": [evt3.encode_evt3(p) for p in packets],
    }
    free = []
    for c in range(N_CYCLES):
        t0 = time.perf_counter()
        _cycle(torch, work)
        free.append(_free_bytes(torch))
        if c < 3 or (c + 1) % 10 == 0:
            print(f"[lifetime] cycle {c + 1}: {time.perf_counter() - t0:.2f} s, free {free[-1]} bytes "
                  f"({free[-1] - free[0]:+d} against cycle 1)")
    drift = free[1] - free[-1]  # > 0: cycles 3 .. N took memory that never came back
    print(f"[lifetime] drift after cycle 2 .. after cycle {N_CYCLES}: {drift} bytes")
    assert drift <= MAX_DRIFT_BYTES, free
