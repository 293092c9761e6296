#!/usr/bin/env python3
"""Time the projector time-map calibration: 64 camera time surfaces 640 x 480 -> a 1080 x 1920 projector time map.

    python tools/time_cal_time.py [--out profiles/time_cal.md] [--repeats 5] [--device 0] [--no-oracle]

The surfaces are rendered (tests/time_cal_cases.render: a white frame seen through a perspective quadrilateral, 20 % of the pixels
dropped per surface, float32).  Per kernel the library's own time from HIP events around each launch (xm_timecal_kernel_ms), the
median of `--repeats` runs after one warm-up; the whole chain's wall clock from host arrays; and beside them the NumPy oracle of
tests/time_cal_cases.py on the same box, run once.  The device's map is compared with the oracle's, bit for bit, before anything is
reported.  No threshold.  Writes a Markdown table."""
import argparse
import os
import platform
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

CAM, PROJ, N_SURF = (640, 480), (1080, 1920), 64
QUAD = ((70, 52), (560, 80), (600, 430), (45, 400))


def cpu_model() -> str:
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.lower().startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or platform.machine()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_cal.md"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--no-oracle", action="store_true", help="skip the NumPy oracle (its fill is a Python loop over 2 M pixels)")
    a = ap.parse_args(argv)
    import time_cal_cases as T
    from x_maps_amd.time_map_calibration import TimeMapCalibrator

    surf = T.render(CAM, PROJ, QUAD, T.curved_time(PROJ), N_SURF, dtype=np.float32, bases=[1000.0 * k for k in range(N_SURF)],
                    span=13_000.0, drop=0.2, seed=1)
    runs, wall = [], []
    with TimeMapCalibrator(CAM, device=a.device) as cal:
        for r in range(a.repeats + 1):
            cal.reset()
            t0 = time.perf_counter()
            cal.add_surfaces(surf)
            cal.mean(0.5)
            got, st = cal.solve(PROJ)
            wall.append(time.perf_counter() - t0)
            runs.append(cal.kernel_ms())
        corners, counts = st.corners, (st.n_valid, st.n_core, st.n_missing, st.n_unfilled)
    runs, wall = runs[1:], wall[1:]
    verdict, t_oracle = "not compared (--no-oracle)", None
    if not a.no_oracle:
        t0 = time.perf_counter()
        o = T.Oracle(CAM)
        o.add(surf)
        t_acc = time.perf_counter() - t0
        want = T.solve(o, T.min_count_for(0.5, o.n_used), PROJ)
        t_oracle = time.perf_counter() - t0
        same = want["time_map"].tobytes() == got.tobytes() and list(corners) == want["corners"]
        verdict = "equal, bit for bit" if same else "DIFFERENT"
    lines = ["# Projector time-map calibration: kernel times", "",
             f"Written by `tools/time_cal_time.py` on an MI355X: {N_SURF} float32 camera time surfaces {CAM[0]} x {CAM[1]} (one call) -> the",
             f"{PROJ[0]} x {PROJ[1]} projector time map; one warm-up run, then the median of {a.repeats}.  Kernel times are the library's own, from",
             "HIP events around each launch.  The arithmetic is this build's definition (include/xmaps.h).  No threshold.", "",
             f"Host CPU: {cpu_model()} (NumPy {np.__version__}).", "", "| kernel | ms (median) | min .. max |", "|---|---|---|"]
    for k in TimeMapCalibrator.KERNELS:
        v = [r[k] for r in runs]
        lines.append(f"| `{k}` | {statistics.median(v):.3f} | {min(v):.3f} .. {max(v):.3f} |")
    total = [sum(r.values()) for r in runs]
    lines += [f"| all six | {statistics.median(total):.3f} | {min(total):.3f} .. {max(total):.3f} |", "",
              f"The whole chain from host arrays (upload of {surf.nbytes / 1e6:.0f} MB, three calls, the host's 8 x 8 solve, the map back): "
              f"{statistics.median(wall) * 1e3:.1f} ms (min {min(wall) * 1e3:.1f}, max {max(wall) * 1e3:.1f}).",
              f"Corners {list(corners)}; valid {counts[0]}, core {counts[1]}, missing before the fill {counts[2]}, unfilled rows {counts[3]}.", ""]
    if t_oracle is not None:
        lines += [f"The NumPy oracle (`tests/time_cal_cases.py`) on the same box, once: {t_oracle * 1e3:.0f} ms, of which accumulate {t_acc * 1e3:.0f} ms "
                  "(its fill is a Python loop per missing pixel: a yardstick for the arithmetic, not a tuned host version).",
                  f"The device's map against the oracle's: {verdict}.", ""]
    else:
        lines += [f"The device's map against the oracle's: {verdict}.", ""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 1 if verdict == "DIFFERENT" else 0


if __name__ == "__main__":
    sys.exit(main())
