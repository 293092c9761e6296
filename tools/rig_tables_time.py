#!/usr/bin/env python3
"""Time the table builders with their maps in NumPy on the host (maps_on_device=False: the yardstick) and on the device (True).

    python tools/rig_tables_time.py [--out profiles/rig_tables.md] [--repeats 5] [--device 0]

Two rigs from tests/golden/g6_esl_calib.npz: the live rig (640 x 480 camera, 1080 x 1920 projector, rect 1760 x 1320, scanning
upwards, replicate border) and the evaluation rig (rect 3240 x 5760 = 3 x projector).  For each, build_tables, build_eval_tables
and build_esl_init_tables: one warm-up call, then the median and the spread (min .. max) of `--repeats` calls, wall clock, one
process.  The per-kernel times are the library's own, from HIP events around each launch (kernel_ms of the entries).  The device
results are compared with the host's before anything is reported.  Writes a Markdown table."""
import argparse
import os
import platform
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cpu_model() -> str:
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.lower().startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or platform.machine()


def timed(fn, repeats):
    t0 = time.perf_counter()
    result = fn()
    warm = time.perf_counter() - t0
    runs = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        runs.append(time.perf_counter() - t0)
    return result, warm, statistics.median(runs), min(runs), max(runs)


def same(a: dict, b: dict) -> bool:
    if set(a) != set(b):
        return False
    for k, v in a.items():
        if isinstance(v, np.ndarray):
            w = b[k]
            if v.dtype != w.dtype or v.shape != w.shape or v.tobytes() != w.tobytes():
                return False
    return True


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rig_tables.md"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    try:  # torch first when it is there; the library needs none
        import torch
        if torch.cuda.is_available():
            torch.cuda.init()
    except ImportError:
        pass
    from x_maps_amd import calibration as C
    from x_maps_amd import esl_init, rig, rig_maps

    npz = os.path.join(ROOT, "tests", "golden", "g6_esl_calib.npz")
    g = np.load(npz)
    live = rig.esl_like_params(npz)
    ev = C.CamProjCalibrationParams(640, 480, 1080, 1920, 3240, 5760, g["camera_K"], g["camera_D"].ravel(), g["projector_K"],
                                    g["projector_D"].ravel(), g["R"], g["T"])
    rigs = [("live", live, f"rect {live.rect_image_width} x {live.rect_image_height}"),
            ("eval", ev, f"rect {ev.rect_image_width} x {ev.rect_image_height}")]
    builders = [("build_tables", lambda cp, on: C.build_tables(cp, device=a.device, maps_on_device=on)),
                ("build_eval_tables", lambda cp, on: C.build_eval_tables(cp, device=a.device, maps_on_device=on)),
                ("build_esl_init_tables", lambda cp, on: esl_init.build_esl_init_tables(cp, maps_on_device=on, device=a.device))]
    rows, slower, differ = [], [], []
    with np.errstate(all="ignore"):
        for rname, cp, shape in rigs:
            for bname, fn in builders:
                host = timed(lambda: fn(cp, False), a.repeats)
                dev = timed(lambda: fn(cp, True), a.repeats)
                if not same(host[0], dev[0]):
                    differ.append(f"{bname} on the {rname} rig")
                if dev[2] > host[2]:
                    slower.append(f"{bname} on the {rname} rig")
                rows.append((rname, shape, bname, host[1:], dev[1:]))
                print(f"{rname:5s} {bname:22s} host {host[2] * 1e3:9.1f} ms   device {dev[2] * 1e3:9.1f} ms", flush=True)
        # the kernels alone (HIP events around each launch): the chain of build_tables, and ESL-init's three maps
        kernels = []
        for rname, cp, shape in rigs:
            size = (cp.rect_image_width, cp.rect_image_height)
            R1, R2, P1, P2, _ = C.stereo_rectify(cp.projector_K, cp.projector_D, cp.camera_K, cp.camera_D, size, cp.cam2proj_R, cp.cam2proj_T)
            xw = cp.projector_width
            ms = [rig_maps.build_xmaps_tables(cp, R1, R2, P1, P2, scan_upwards=rname == "live", zero_undistort_proj_map=rname == "eval",
                                              time_map_border="replicate" if rname == "live" else "constant", x_map_width=xw,
                                              t_px_scale=xw - 1, x_offset=4242, device=a.device)["kernel_ms"] for _ in range(a.repeats + 1)][1:]
            for i, name in enumerate(("k_rig_forward_map (projector, remap of the linear time map only)", "k_build_x_map_sorted",
                                      "k_rig_inverse_map (camera: f32 + int16 maps)", "k_rig_inverse_map (projector: int16 pair)")):
                kernels.append((rname, name, statistics.median(m[i] for m in ms)))
            fwd = [rig_maps.forward_map(cp.camera_K, cp.camera_D, R1, P1, size, want_maps=False, want_pair=True, device=a.device)["kernel_ms"]
                   for _ in range(a.repeats + 1)][1:]
            kernels.append((rname, "k_rig_forward_map (camera, int16 pair only: ESL-init's cam_to_rect_map)", statistics.median(fwd)))
            fwd2 = [rig_maps.forward_map(cp.camera_K, cp.camera_D, R1, P1, size, device=a.device)["kernel_ms"] for _ in range(a.repeats + 1)][1:]
            kernels.append((rname, "k_rig_forward_map (camera, both f32 maps)", statistics.median(fwd2)))

    fmt = lambda t: f"{t[0] * 1e3:.1f} | {t[1] * 1e3:.1f} | {t[2] * 1e3:.1f} .. {t[3] * 1e3:.1f}"
    lines = ["# Table builders: maps in NumPy on the host vs on the device", "",
             "Written by `tools/rig_tables_time.py` on an MI355X; wall clock of the whole Python call (maps, X-map, copies back into the",
             f"dict), one process, one warm-up call then {a.repeats} timed calls.  `maps_on_device=False` is the yardstick: that path is",
             "the one every earlier commit runs.  Times in ms.", "",
             f"Host CPU: {cpu_model()} (NumPy {np.__version__}).", "",
             "| rig | builder | host warm-up | host median | host min .. max | device warm-up | device median | device min .. max | host / device |",
             "|---|---|---|---|---|---|---|---|---|"]
    for rname, shape, bname, h, d in rows:
        lines.append(f"| {rname} ({shape}) | `{bname}` | {fmt(h)} | {fmt(d)} | {h[1] / d[1]:.1f} x |")
    lines += ["", "The kernels alone, from HIP events around each launch (median, ms):", "", "| rig | kernel | ms |", "|---|---|---|"]
    for rname, name, ms in kernels:
        lines.append(f"| {rname} | {name} | {ms:.3f} |")
    lines += ["", "Every device-built dict was compared with the host-built one, byte for byte: " +
              ("all equal." if not differ else "DIFFERENT for " + ", ".join(differ) + "."),
              "The device path is " + ("not slower than the NumPy path in any row." if not slower else
                                       "SLOWER than the NumPy path for " + ", ".join(slower) + "."), ""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
