"""What tools/frame_surfaces_time.py, tools/frame_clouds_time.py and tools/evt3_record_time.py share: the child-step runner, the
ingest pass loop with the stage alternating off / on, and the pieces of the markdown they write.  Imported by the three tools
(tools/ is the script's directory, so `import _frame_stage` finds it); no tool imports another tool."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HBM_BYTES_PER_S = 6.29e12  # measured streaming rate of an MI355X (float4 copy)
GROUP = 32
TRIED = "## Notes\n"
FRAMES_NOTE = "rendered from rig.py's ESL-like stand-in, as bench.py --esl renders them; NOT the ESL recordings"


def gpu():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device and has no fallback")
    torch.cuda.init()
    return torch


def add_arguments(ap, parent_lib_help):
    ap.add_argument("--md", help="write the profile (markdown) here")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--passes", type=int, default=7, help="timed passes of the stream per setting")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--parent-lib", help=parent_lib_help)
    ap.add_argument("--step-timeout", type=float, default=240.0)
    ap.add_argument("--step", help=argparse.SUPPRESS)  # (internal: one step in this process)


def run_steps(script, tag, steps, a, res):
    """steps: (name in res, --step value, XM_LIB or None).  Each in a fresh child process of `script` under a.step_timeout; its
    result is the last line of its output that starts with `tag`.  No further step is started after one that failed or ran out of
    time.  Sets res["complete"], prints res, returns whether every step gave a result."""
    ok = True
    for name, step, lib in steps:
        env = dict(os.environ)
        env.pop("XM_LIB", None)
        if lib:
            env["XM_LIB"] = lib
        cmd = [sys.executable, os.path.abspath(script), "--step", step, "--repeats", str(a.repeats), "--passes", str(a.passes),
               "--device", str(a.device)]
        try:
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            res[name] = {"error": f"no result within {a.step_timeout} s"}
            ok = False
            break
        line = [ln for ln in r.stdout.splitlines() if ln.startswith(tag)]
        if r.returncode != 0 or not line:
            res[name] = {"error": f"exit status {r.returncode}", "stderr_tail": r.stderr[-1500:]}
            ok = False
            break
        res[name] = json.loads(line[-1][len(tag):])
    res["complete"] = ok
    print(json.dumps(res, indent=1))
    return ok


def write_md(path, res, markdown):
    """markdown(res, notes) -> path; the hand-written section of an earlier profile stays"""
    notes = ""
    if os.path.exists(path):
        old = open(path).read()
        if TRIED in old:
            notes = old.split(TRIED, 1)[1]
    with open(path, "w") as f:
        f.write(markdown(res, notes))


def ingest_passes(passes, device, new_symbols, set_stage, after_pass=None):
    """The ESL-like stream (48 frames, quarter-period packets of pinned records, activity filter on, BGR frames out) through ONE
    DeviceIngest, whole passes (push everything, flush, poll, reset) alternating stage off / on; the result dict of the step.
    set_stage(ing, on) switches the stage; after_pass(ing, frames, on) looks at a pass's frames outside the timed window.
    set_stage None: the stage is absent (the parent commit's build through XM_LIB, which does not export `new_symbols` -- entries
    this step then never calls): stage-off passes only."""
    gpu()
    with_stage = set_stage is not None
    if not with_stage:
        from x_maps_amd import _native as N
        for name in new_symbols:
            N.SYMBOLS.pop(name, None)
    from x_maps_amd import XMapsEngine, rig
    from x_maps_amd import synthetic as S
    from x_maps_amd.ingest import DeviceIngest
    cp, tables, _, _ = rig.make_esl_like(row_stride=13, device=device)
    n_mean = int(np.mean([len(rig.render_events(cp, tables, row_stride=13, seed=f)[0]) for f in range(8)]))
    n_frames = 48
    stream, _ = rig.render_stream(cp, tables, n_frames=n_frames, row_stride=13, seed=9)
    res = {"events": int(len(stream)), "frames_rendered": n_frames}
    with XMapsEngine(tables, device=device, n_slots=4) as eng:
        pin = eng.host_empty((len(stream),), S.EVENT_CD_DTYPE)
        pin[:] = stream
        packet = int(1e6 / 60 / 4)
        cuts = np.searchsorted(pin["t"], np.arange(pin["t"][0], pin["t"][-1] + packet, packet))
        packets = [pin[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
        with DeviceIngest(eng, 60, capacity_events=1 << 21, max_packet_events=1 << 18, expected_events_per_frame=n_mean,
                          result_ring=n_frames + 2, want_depth=False, want_bgr=True, activity_filter=True) as ing:
            def one_pass(on):
                if with_stage:
                    set_stage(ing, on)
                c0 = time.perf_counter()
                for pk in packets:
                    ing.push_pinned(pk)
                ing.flush()
                got = ing.poll(copy=False)
                dt = time.perf_counter() - c0
                if with_stage and after_pass:
                    after_pass(ing, got, on)
                ing.reset()
                return dt, len(got)
            modes = [False, True] if with_stage else [False]
            for on in modes * 2:  # warm-up: both settings twice (the first on-pass allocates the stage's ring)
                one_pass(on)
            times = {m: [] for m in modes}
            cut = None
            for k in range(passes * len(modes)):  # alternating, in one process
                on = modes[k % len(modes)]
                dt, n = one_pass(on)
                times[on].append(dt)
                cut = n if cut is None else cut
                assert n == cut, "the passes cut different numbers of frames"
            res["frames_cut"] = cut
            for on, v in times.items():
                med = float(np.median(v))
                res["stage_on" if on else "stage_off"] = {"Mevents_per_s": round(len(stream) / med / 1e6, 1), "ms_per_pass_median": round(med * 1e3, 3),
                                                          "passes_ms": [round(x * 1e3, 3) for x in v]}
    return res


def run_rows(runs):
    """the rows of the ingest table: (setting, one stage_off / stage_on result)"""
    return "\n".join(f"| {k} | {v['Mevents_per_s']} | {v['ms_per_pass_median']} | {v['passes_ms']} |" for k, v in runs)


def md_head(title, tool, clock):
    return f"""# {title}: times on the ESL-like stream

Written by `tools/{tool}` on an MI355X.  **The frames are rendered** from `x_maps_amd/rig.py`'s ESL-like stand-in
(640 x 480 camera, the frames `bench.py --esl` renders), not the ESL recordings.  Every step in a process of its own.
Clock state of the box, queried idle before the first launch: {clock}.

**Nothing was measured before this**: the parent commit has no such entry.  These are first numbers, not a bar.
"""


def md_ingest(r, entry, extra, rows, ratio_note, notes):
    i = r["ingest"]
    off, on = i["stage_off"], i["stage_on"]
    return f"""## The ingest's stage (`{entry}`)

The ESL-like stream ({i['events']} events, {i['frames_rendered']} frames rendered, {i['frames_cut']} cut), quarter-period packets of
pinned records, activity filter on, BGR frames out; whole passes (push everything, flush, poll) alternating stage off / on in one
process, {r['passes']} timed passes each, the median reported{extra}.

| setting | Mev/s | ms / pass (median) | passes, ms |
|---|---|---|---|
{rows}

Stage on / off: {on['Mevents_per_s'] / off['Mevents_per_s']:.3f} of the rate.  {ratio_note}

{TRIED}
{notes.strip() or "(written by hand below this heading; kept when the tool rewrites the file)"}
"""
