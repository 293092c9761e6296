"""What the *_time.py tools share: the box's clock state, one timer and the rendered time surfaces.  Imported by the tools (tools/ is
the script's directory, so `import _timing` finds it); no tool imports another tool."""
from __future__ import annotations

import collections
import subprocess
import time

import numpy as np

Timing = collections.namedtuple("Timing", "ev ev_min ev_max host host_min host_max")  # ms: medians and extremes over the repeats


def clock_state() -> str:
    """what the box says about its clocks (read-only query); 'unknown' when the tool is not there"""
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--showperflevel"], capture_output=True, text=True, timeout=30)
        lines = [" ".join(ln.split()) for ln in r.stdout.splitlines() if "GPU[0]" in ln and ("sclk" in ln or "mclk" in ln or "Performance" in ln)]
        return "; ".join(lines) if lines else "unknown (no clock lines in the query's output)"
    except Exception as e:  # noqa: BLE001
        return f"unknown ({type(e).__name__})"


def timed(fn, repeats, warmup=3) -> Timing:
    """fn ends in a device synchronise.  After `warmup` calls, `repeats` calls: each between two device events, with the host clock
    around the call alone -- the events are recorded outside the host's interval, so a tool that reports only the host clock reads
    what it read without them."""
    import torch
    for _ in range(warmup):
        fn()
    ev, host = [], []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        t0 = time.perf_counter()
        fn()
        host.append((time.perf_counter() - t0) * 1e3)
        b.record()
        b.synchronize()
        ev.append(a.elapsed_time(b))
    ev, host = np.array(ev), np.array(host)
    return Timing(float(np.median(ev)), float(ev.min()), float(ev.max()), float(np.median(host)), float(host.min()), float(host.max()))


def render_surfaces(cp, tables, n_distinct):
    """n_distinct float32 time surfaces (microsecond stamps, 0 = no event), each another rendering of x_maps_amd/rig.py's scene"""
    from x_maps_amd import rig
    base = []
    for k in range(n_distinct):
        evs, _ = rig.render_events(cp, tables, row_stride=3, scan_upwards=False, seed=k)
        s = np.zeros((cp.camera_height, cp.camera_width), np.float32)
        s[evs["y"], evs["x"]] = (evs["t"] - evs["t"].min() + 1).astype(np.float32)  # (the last event of a pixel stays)
        base.append(s)
    return base


def cycle(base, n):
    """a contiguous group of n surfaces that cycles through `base`"""
    return np.ascontiguousarray(np.stack([base[i % len(base)] for i in range(n)]))
