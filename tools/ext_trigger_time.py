#!/usr/bin/env python3
"""Time the EXT_TRIGGER extraction and the frames cut at the triggers (x_maps_amd/ext_trigger.py).

    python tools/ext_trigger_time.py [--md profiles/ext_trigger.md] [--parent-lib libxmaps_parent.so] [--repeats 20] [--passes 7]

NOT the benchmark (bench.py measures the flagship workload); this gives the numbers of profiles/ext_trigger.md.  The streams
are tools/evt21_time.py's (the ESL-like stream, rendered; the dense EVT 2.1 words, synthetic): no real triggered recording
exists beside this project.  The parent process never opens the GPU: every step runs in a fresh child process under its own
time limit, and no further step is started after one that failed or ran out of time.
  decode   per stream and format, decode_device (pageable words in, synchronous), the median of --repeats calls:
             (a) --parent-lib, the parent commit's build, three runs (three child processes): their spread is the margin;
             (b) this build, extraction off, on the same words;
             (c) this build on the words with one trigger per 16.7 ms of stream (one per rendered frame; the dense stream: one per
                 1/16 of its words), extraction off and on in alternating rounds: the cost of the two launches and the download.
  chain    the ESL-like stream (rig.render_stream, as benchmodes/esl.py renders it) with a trigger per frame as EVT 3.0 words in
           period chunks through DepthReprojectionPipe with frame_sync = "ext_trigger", beside the device ingest's pause finder
           on the same stream without the trigger words: frames/s and ms per frame, whole passes.
  kernels  the two extraction launches and the append under rocprofv3 --kernel-trace --stats (a child of its own).
With --filters-md FILE the tool measures the chain's two filters instead (profiles/ext_trigger_filters.md): xm_trigframes_push with
both stages off beside three runs of --parent-lib, the activity stage on minus off and its kernels beside the ingest's, the frame
event filters' device stage against the download path per shown frame, and one pass at the reference's threshold."""
from __future__ import annotations

import argparse
import glob
import json
import os
import shutil
import sqlite3
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _frame_stage as F  # noqa: E402
from _timing import clock_state, timed  # noqa: E402

TAG = "EXTTRIG_STEP "
NEW_SYMBOLS = ("xm_evt_set_ext_triggers", "xm_evt_last_ext_triggers", "xm_trigframes_create", "xm_trigframes_destroy", "xm_trigframes_reset",
               "xm_trigframes_push", "xm_trigframes_ready", "xm_trigframes_release", "xm_trigframes_stats")
PERIOD_US = 16_600  # rig.render_stream's frame period
CHAIN_FRAMES = 24


ESL_FRAMES = 8


def esl_stream(device):
    """tools/evt21_time.py's esl stream (no tool imports another: restated)"""
    from x_maps_amd import rig
    cp, tables, _, _ = rig.make_esl_like(row_stride=13, device=device)
    stream, _ = rig.render_stream(cp, tables, n_frames=ESL_FRAMES, row_stride=13, seed=9)
    return tables, stream


def dense_words(n=1 << 18, seed=7):
    """tools/evt21_time.py's dense stream: synthetic EVT 2.1 words on a 640 x 480 sensor, a TIME_HIGH every 64 words, >= 16 events per word"""
    rng = np.random.default_rng(seed)
    mask = rng.integers(0, 1 << 32, n, dtype=np.uint64) | rng.integers(0, 1 << 32, n, dtype=np.uint64)
    mask |= np.uint64(0xFFFF) << (rng.integers(0, 2, n).astype(np.uint64) * np.uint64(16))
    i = np.arange(n, dtype=np.uint64)
    top = (rng.integers(0, 2, n).astype(np.uint64) << np.uint64(28)) | ((i % np.uint64(64)) << np.uint64(22)) \
        | ((rng.integers(0, 20, n).astype(np.uint64) * np.uint64(32)) << np.uint64(11)) | rng.integers(0, 480, n).astype(np.uint64)
    w = (top << np.uint64(32)) | mask
    is_hi = i % np.uint64(64) == 0
    w[is_hi] = (np.uint64(0x8) << np.uint64(60)) | ((i[is_hi] // np.uint64(64) + np.uint64(1000)) << np.uint64(32))
    return w.astype("<u8")


def _frame_starts(stream, n_frames):
    return np.searchsorted(stream["t"], 2_000_000 + PERIOD_US * np.arange(n_frames + 1))  # (render_stream's t_start_us)


def _words(device):
    """name -> (plain words, the same with triggers, fmt, device decoder class, events)"""
    from x_maps_amd import evt2, evt21, evt3
    from x_maps_amd import ext_trigger as X
    tables, stream = esl_stream(device)
    at = _frame_starts(stream, ESL_FRAMES)
    t = 2_000_000 + PERIOD_US * np.arange(ESL_FRAMES + 1) - 100
    out = {}
    for name, fmt, enc, cls in (("esl EVT 3.0", 3, evt3.encode_evt3, evt3.DeviceEvt3Decoder), ("esl EVT 2.0", 2, evt2.encode_evt2, evt2.DeviceEvt2Decoder),
                                ("esl EVT 2.1", 21, evt21.encode_evt21, evt21.DeviceEvt21Decoder)):
        plain = enc(stream)
        out[name] = (plain, X.insert_ext_triggers(plain, fmt, at, 0, 1, t=t), fmt, cls, len(stream))
    dense = dense_words()
    pos = (np.arange(16) * (len(dense) // 16)).astype(np.int64)
    trig = np.array([X.trigger_word(21, 0, 1, 0)] * 16, dtype="<u8")
    out["dense EVT 2.1"] = (dense, np.insert(dense, pos, trig), 21, evt21.DeviceEvt21Decoder, len(evt21.decode_evt21(dense)))
    return tables, out


def step_decode(repeats, device):
    F.gpu()
    from x_maps_amd import _native as N
    parent = bool(os.environ.get("XM_LIB"))
    if parent:
        for name in NEW_SYMBOLS:
            N.SYMBOLS.pop(name, None)
    from x_maps_amd import XMapsEngine
    from x_maps_amd import ext_trigger as X
    tables, streams = _words(device)
    res = {}
    with XMapsEngine(tables, device=device) as eng:
        for name, (plain, with_trig, fmt, cls, n_ev) in streams.items():
            _, want = X.ExtTriggerExtractor(fmt).extract(with_trig)
            row = res[name] = {"words": int(len(plain)), "words_with_triggers": int(len(with_trig)), "events": int(n_ev), "triggers": int(len(want))}
            n_max = len(with_trig)
            off = cls(eng, max_words=n_max, max_events=n_ev)
            row["off_plain_ms"] = round(timed(lambda: (off.reset(), off.decode_device(plain)), repeats).ev, 4)
            if not parent:
                on = cls(eng, max_words=n_max, max_events=n_ev)
                on.set_ext_triggers(4096)
                on.decode_device(with_trig)
                assert on.last_ext_triggers().tobytes() == want.tobytes() and len(want) >= 9, name
                rounds = {"off": [], "on": []}
                for _ in range(2):  # alternating rounds in one process
                    for k, dec in (("off", off), ("on", on)):
                        rounds[k].append(timed(lambda d=dec: (d.reset(), d.decode_device(with_trig)), max(3, repeats // 2)).ev)
                row["off_trig_ms"], row["on_trig_ms"] = round(min(rounds["off"]), 4), round(min(rounds["on"]), 4)
                row["rounds_ms"] = {k: [round(x, 4) for x in v] for k, v in rounds.items()}
                on.close()
            off.close()
    print(TAG + json.dumps(res), flush=True)


def _chain_stream(device):
    from x_maps_amd import evt3, rig
    from x_maps_amd import ext_trigger as X
    cp, tables, _, _ = rig.make_esl_like(row_stride=13, device=device)
    stream, _ = rig.render_stream(cp, tables, n_frames=CHAIN_FRAMES, row_stride=13, seed=9)
    cuts = np.searchsorted(stream["t"], np.arange(stream["t"][0], stream["t"][-1] + PERIOD_US, PERIOD_US))
    packets = [stream[a:b] for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
    plain = [evt3.encode_evt3(pk) for pk in packets]  # (the encoder insert_ext_triggers uses: like for like)
    # a trigger in front of every rendered frame, in the dark gap 100 us before it, and one behind the last
    with_trig = []
    t_trig = 2_000_000 + PERIOD_US * np.arange(CHAIN_FRAMES + 1) - 100
    for pk, w in zip(packets, plain):
        tt = t_trig[(t_trig >= pk["t"][0] - 200) & (t_trig <= pk["t"][-1])] if len(with_trig) else t_trig[t_trig <= pk["t"][-1]]
        t_trig = t_trig[t_trig > pk["t"][-1]]
        with_trig.append(X.insert_ext_triggers(w, 3, np.searchsorted(pk["t"], tt), 0, 1, t=tt) if len(tt) else w)
    with_trig[-1] = np.concatenate((with_trig[-1], X.insert_ext_triggers(np.zeros(0, "<u2"), 3, [0] * len(t_trig), 0, 1, t=t_trig))) if len(t_trig) else with_trig[-1]
    return tables, stream, plain, with_trig


def step_chain(passes, device):
    F.gpu()
    from x_maps_amd.depth_reprojection_processor import DepthReprojectionProcessor, RuntimeParams
    tables, stream, plain, with_trig = _chain_stream(device)
    res = {"events": int(len(stream)), "frames_rendered": CHAIN_FRAMES, "chunks": len(plain)}

    class Window:
        n = 0

        def should_close(self):
            return False

        def show_async(self, img):
            Window.n += 1

    for name, chunks, kw in (("ext_trigger", with_trig, {"frame_sync": "ext_trigger"}), ("pauses (device ingest)", plain, {"activity_filter": False})):
        params = RuntimeParams(camera_width=640, camera_height=480, projector_width=1080, projector_height=1920, projector_fps=60, z_near=0.1,
                               z_far=1.2, calib=None, tables=tables, device=device, **kw)
        with DepthReprojectionProcessor(params, window=Window()) as proc:
            def one_pass():
                Window.n = 0
                c0 = time.perf_counter()
                for w in chunks:
                    proc.process_evt3_words(w)
                proc.flush()
                dt = time.perf_counter() - c0
                n = Window.n
                proc._pipe.reset()
                for d in proc._pipe._raw_dev.values():
                    d.reset()
                return dt, n
            one_pass(), one_pass()
            ts, shown = [], None
            for _ in range(passes):
                dt, n = one_pass()
                ts.append(dt)
                shown = n if shown is None else shown
                assert n == shown, "the passes showed different numbers of frames"
            med = float(np.median(ts))
            res[name] = {"frames_shown": shown, "ms_per_pass_median": round(med * 1e3, 3), "ms_per_frame": round(med * 1e3 / max(shown, 1), 4),
                         "frames_per_s": round(shown / med, 1), "passes_ms": [round(x * 1e3, 3) for x in ts]}
            if proc._pipe._trig is not None:
                res[name]["counters"] = proc._pipe._trig.stats()
    print(TAG + json.dumps(res), flush=True)


def step_kernels_child(device):
    """what the kernel trace looks at: decodes with extraction on and pushes with positive_only, on the esl EVT 3.0 words"""
    F.gpu()
    from x_maps_amd import XMapsEngine
    from x_maps_amd import ext_trigger as X
    tables, streams = _words(device)
    _, with_trig, _, cls, n_ev = streams["esl EVT 3.0"]
    with XMapsEngine(tables, device=device) as eng, cls(eng, max_words=len(with_trig), max_events=n_ev) as dec:
        dec.set_ext_triggers(4096)
        with X.TriggeredFrames(eng, cap_events=4 * n_ev, positive_only=True) as tf:
            for _ in range(20):
                dec.reset(), tf.reset()
                tf.push(dec, with_trig)
    print(TAG + json.dumps({"words": int(len(with_trig)), "events": int(n_ev)}), flush=True)


def step_kernels(a):
    """-> per kernel {calls, avg_us, min_us, max_us} from rocprofv3 --kernel-trace --stats of the child above"""
    prof = shutil.which("rocprofv3")
    if prof is None:
        return {"error": "rocprofv3 not found"}
    tmp = tempfile.mkdtemp(prefix="exttrig_")
    try:
        cmd = [prof, "--kernel-trace", "--stats", "-d", tmp, "-o", "trig", "--", sys.executable, os.path.abspath(__file__), "--step", "kernels_child",
               "--device", str(a.device)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith(TAG)]
        if r.returncode != 0 or not line:
            return {"error": f"exit status {r.returncode}", "stderr_tail": r.stderr[-1500:]}
        out = dict(json.loads(line[-1][len(TAG):]), kernels={})
        for db in glob.glob(os.path.join(tmp, "**", "*.db"), recursive=True):
            c = sqlite3.connect(db)
            for name, d in c.execute("select name, end - start from kernels"):
                short = name.split("(")[0].replace("void ", "").replace("xm::", "")
                if "trig" in short or short.startswith("k_evt3_"):
                    out["kernels"].setdefault(short, []).append(d)
        out["kernels"] = {k: {"calls": len(v), "avg_us": round(sum(v) / len(v) / 1e3, 2), "min_us": round(min(v) / 1e3, 2), "max_us": round(max(v) / 1e3, 2)}
                          for k, v in sorted(out["kernels"].items())}
        return out if out["kernels"] else dict(out, error="no kernel rows in the trace")
    except (subprocess.TimeoutExpired, sqlite3.Error) as e:
        return {"error": repr(e)}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


# ---- the chain's two filters (--filters-md): xm_trigframes_set_activity / xm_trigframes_set_frame_filter ---------------------------
FILTER_SYMBOLS = ("xm_trigframes_set_activity", "xm_trigframes_filter_stats", "xm_trigframes_set_frame_filter", "xm_trigframes_ready_filtered")
ACT_T = int(1e6 / 60)  # the reference's threshold at 60 Hz


def step_push(repeats, device, off_only=False):
    """xm_trigframes_push over the chain stream's period chunks, whole passes (reset, every chunk), the median of `repeats` passes
    after two: both stages off (what the parent's build can run; this build: off_only, the same process shape as the parent's runs)
    or, on this build, alternating with the activity stage on"""
    F.gpu()
    from x_maps_amd import _native as N
    parent = bool(os.environ.get("XM_LIB"))
    off_only = off_only or parent
    if parent:
        for name in FILTER_SYMBOLS:
            N.SYMBOLS.pop(name, None)
    from x_maps_amd import XMapsEngine, evt3
    from x_maps_amd import ext_trigger as X
    tables, stream, _, chunks = _chain_stream(device)
    res = {"events": int(len(stream)), "chunks": len(chunks)}
    with XMapsEngine(tables, device=device) as eng, evt3.DeviceEvt3Decoder(eng, max_words=max(len(c) for c in chunks)) as dec:
        dec.set_ext_triggers(4096)
        with X.TriggeredFrames(eng, cap_events=1 << 22, min_events=1000, positive_only=True) as tf:
            def one_pass():
                dec.reset(), tf.reset()
                c0 = time.perf_counter()
                for w in chunks:
                    tf.push(dec, w)
                    tf.release(len(tf.ready(64)[1]) - 1)
                return time.perf_counter() - c0
            modes = ["off"] if off_only else ["off", "activity"]
            times = {m: [] for m in modes}
            for k in range((repeats + 2) * len(modes)):  # alternating, in one process; the first two rounds are warm-up
                m = modes[k % len(modes)]
                if not off_only:
                    tf.set_activity(ACT_T if m == "activity" else None)
                dt = one_pass()
                if k >= 2 * len(modes):
                    times[m].append(dt)
            for m, v in times.items():
                res[m] = {"ms_per_chunk": round(float(np.median(v)) * 1e3 / len(chunks), 4), "ms_per_pass_median": round(float(np.median(v)) * 1e3, 3),
                          "ms_per_pass_min_max": [round(min(v) * 1e3, 3), round(max(v) * 1e3, 3)]}
            if not off_only:  # one pass at the reference's T on the period chunks, counted on its own
                tf.set_activity(None), tf.set_activity(ACT_T)
                before = tf.filter_stats()
                one_pass()
                after, st = tf.filter_stats(), tf.stats()
                res["one_pass_at_T"] = {"thresh_us": ACT_T, "chunks_sequential": after["chunks_sequential"] - before["chunks_sequential"],
                                        "events_positive": after["events_positive"] - before["events_positive"],
                                        "events_active": after["events_active"] - before["events_active"], "frames_cut_total": st["frames_cut"]}
    print(TAG + json.dumps(res), flush=True)


def step_frame_filters(passes, device):
    """the chain per shown frame with a frame event filter selected: device stage against download path, alternating passes"""
    F.gpu()
    from x_maps_amd.depth_reprojection_processor import DepthReprojectionProcessor, RuntimeParams
    tables, stream, _, chunks = _chain_stream(device)
    res = {"events": int(len(stream)), "chunks": len(chunks)}

    class Window:
        n = 0

        def should_close(self):
            return False

        def show_async(self, img):
            Window.n += 1

    for label, presses in (("LastEventPerXY", 3), ("FirstEventPerYT", 1)):
        procs = {}
        for mode in ("download", "device"):
            params = RuntimeParams(camera_width=640, camera_height=480, projector_width=1080, projector_height=1920, projector_fps=60, z_near=0.1,
                                   z_far=1.2, calib=None, tables=tables, device=device, frame_sync="ext_trigger", device_frame_filters=mode == "device")
            procs[mode] = DepthReprojectionProcessor(params, window=Window()).__enter__()
            for _ in range(presses):
                procs[mode]._pipe.select_next_frame_event_filter()
        assert type(procs["device"]._pipe.ev_filter_proc.selected_filter()).__name__.startswith(label)

        def one_pass(proc):
            Window.n = 0
            c0 = time.perf_counter()
            for w in chunks:
                proc.process_evt3_words(w)
            dt = time.perf_counter() - c0
            proc._pipe.reset()
            return dt, Window.n
        times = {m: [] for m in procs}
        shown = None
        for k in range((passes + 2) * 2):
            m = ("download", "device")[k % 2]
            dt, n = one_pass(procs[m])
            shown = n if shown is None else shown
            assert n == shown, "the two paths showed different numbers of frames"
            if k >= 4:
                times[m].append(dt)
        res[label] = {"frames_shown": shown, "filter_stats": procs["device"]._pipe._trig.filter_stats()}
        for m, v in times.items():
            res[label][m] = {"ms_per_frame": round(float(np.median(v)) * 1e3 / max(shown, 1), 4), "passes_ms": [round(x * 1e3, 2) for x in v]}
        for p in procs.values():
            p.__exit__(None, None, None)
    print(TAG + json.dumps(res), flush=True)


def step_filter_kernels_child(device, which):
    """what the two kernel traces look at: pushes with the activity stage on (`trig`), or the same chunks' positive events as packets
    through the activity filter alone, the ingest's kernels (`alone`)"""
    F.gpu()
    from x_maps_amd import XMapsEngine, evt3
    from x_maps_amd import ext_trigger as X
    tables, stream, _, chunks = _chain_stream(device)
    with XMapsEngine(tables, device=device) as eng:
        if which == "trig":
            with evt3.DeviceEvt3Decoder(eng, max_words=max(len(c) for c in chunks)) as dec:
                dec.set_ext_triggers(4096)
                with X.TriggeredFrames(eng, cap_events=1 << 22, positive_only=True, activity_thresh_us=ACT_T) as tf:
                    for _ in range(3):
                        dec.reset(), tf.reset()
                        for w in chunks:
                            tf.push(dec, w)
                            tf.release(len(tf.ready(64)[1]) - 1)
        else:
            from x_maps_amd.activity_filter import ActivityNoiseFilterAlgorithm
            ext = X.ExtTriggerExtractor(3)
            packets = [ext.extract(w)[0] for w in chunks]
            packets = [p[p["p"] == 1] for p in packets]
            flt = ActivityNoiseFilterAlgorithm(eng, ACT_T)
            for _ in range(3):
                flt.reset()
                for p in packets:
                    flt.process_events(p)
    print(TAG + json.dumps({"events": int(len(stream)), "chunks": len(chunks)}), flush=True)


def step_filter_kernels(a, which):
    prof = shutil.which("rocprofv3")
    if prof is None:
        return {"error": "rocprofv3 not found"}
    tmp = tempfile.mkdtemp(prefix="trigflt_")
    try:
        cmd = [prof, "--kernel-trace", "--stats", "-d", tmp, "-o", "trig", "--", sys.executable, os.path.abspath(__file__), "--step", "filter_kernels_" + which,
               "--device", str(a.device)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith(TAG)]
        if r.returncode != 0 or not line:
            return {"error": f"exit status {r.returncode}", "stderr_tail": r.stderr[-1500:]}
        rows = {}
        for db in glob.glob(os.path.join(tmp, "**", "*.db"), recursive=True):
            c = sqlite3.connect(db)
            for name, d in c.execute("select name, end - start from kernels"):
                short = name.split("(")[0].replace("void ", "").replace("xm::", "")
                if short.startswith(("k_act_", "k_trigact_", "k_trig_keep")):
                    rows.setdefault(short, []).append(d)
        rows = {k: {"calls": len(v), "avg_us": round(sum(v) / len(v) / 1e3, 2), "min_us": round(min(v) / 1e3, 2), "max_us": round(max(v) / 1e3, 2)}
                for k, v in sorted(rows.items())}
        return rows or {"error": "no kernel rows in the trace"}
    except (subprocess.TimeoutExpired, sqlite3.Error) as e:
        return {"error": repr(e)}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def filters_markdown(r, notes="") -> str:
    parents = [r[k] for k in ("parent_1", "parent_2", "parent_3") if k in r and "error" not in r[k]]
    p, pa = r["push"], [q["off"]["ms_per_chunk"] for q in parents]
    offs = [r[k] for k in ("off_1", "off_2", "off_3") if k in r and "error" not in r[k]]
    mine = float(np.median([q["off"]["ms_per_chunk"] for q in offs]))
    inside = ("inside" if min(pa) <= mine <= max(pa) else
              f"OUTSIDE ({mine / (sum(pa) / len(pa)):.3f} of the parent's mean)") if pa else "not measured (no --parent-lib)"
    one = p["one_pass_at_T"]
    ff = r["frame_filters"]
    ff_rows = "\n".join(f"| {k} | {v['frames_shown']} | {v['download']['ms_per_frame']} | {v['device']['ms_per_frame']} | "
                        f"{v['device']['ms_per_frame'] / v['download']['ms_per_frame']:.3f} | {v['download']['passes_ms']} | {v['device']['passes_ms']} |"
                        for k, v in ff.items() if isinstance(v, dict))

    def ktable(k):
        if "error" in k:
            return f"Not measured in this run: {k['error']}."
        return "| kernel | calls | avg us | min us | max us |\n|---|---|---|---|---|\n" + "\n".join(
            f"| `{n}` | {v['calls']} | {v['avg_us']} | {v['min_us']} | {v['max_us']} |" for n, v in k.items())
    return f"""# The triggered chain's two filters: times

Written by `tools/ext_trigger_time.py --filters-md` on an MI355X.  **No real triggered recording exists beside this project: the
stream is rendered** -- the ESL-like stream of `profiles/ext_trigger.md` ({p['events']} events, {CHAIN_FRAMES} frames, a trigger 100 us in
front of every frame) as EVT 3.0 words in {p['chunks']} period chunks.  Every step in a process of its own, all in one call.
Clock state of the box, queried idle before the first launch: {r['clock_state']}.

## 1. Stages off against the parent commit's library

`xm_trigframes_push` (+ ready / release) over the chunks, whole passes, the median of {r['repeats']} passes after two.  The parent's
build three times (three processes): its own spread is the margin.  This build with both stages off three times too, in processes of
the same shape, the two builds taking turns (parent, this, parent, this, ...): a box's rate drifts from process to process by more
than the two builds differ.  Compared: the median of this build's three runs.

| build | ms / chunk | ms / pass (median) | pass min .. max, ms |
|---|---|---|---|
{chr(10).join(f"| parent, run {i + 1} | {q['off']['ms_per_chunk']} | {q['off']['ms_per_pass_median']} | {q['off']['ms_per_pass_min_max']} |" for i, q in enumerate(parents))}
{chr(10).join(f"| this build, both stages off, run {i + 1} | {q['off']['ms_per_chunk']} | {q['off']['ms_per_pass_median']} | {q['off']['ms_per_pass_min_max']} |" for i, q in enumerate(offs))}

In the order they ran: {", ".join(f"{k} {r[k]['off']['ms_per_chunk']}" for k in ("parent_1", "off_1", "parent_2", "off_2", "parent_3", "off_3") if k in r and "error" not in r[k])}.
This build (median {mine:.4f} ms / chunk) lies **{inside}** the parent's spread{f" ({min(pa)} .. {max(pa)} ms / chunk)" if pa else ""}.

## 2. The activity stage on minus off

The same passes alternating off / on (T = {ACT_T} us) in one process: off {p['off']['ms_per_chunk']} ms / chunk, on
{p['activity']['ms_per_chunk']} ms / chunk: **{p['activity']['ms_per_chunk'] - p['off']['ms_per_chunk']:+.4f} ms per chunk**
({p['activity']['ms_per_chunk'] / p['off']['ms_per_chunk']:.3f} x).

The stage's kernels, `rocprofv3 --kernel-trace --stats` of three passes in a process of its own:

{ktable(r['kernels_trig'])}

Beside them the ingest's activity kernels (`xm_activity_process`: `k_act_first`, `k_act_mark`, `k_act_update`) on the same chunks'
positive events, a trace of its own:

{ktable(r['kernels_alone'])}

## 3. Frame event filter: device stage against download path

The chain through `DepthReprojectionPipe` with the filter selected, ms per shown frame, the median of {r['passes']} whole passes
after two, the two paths alternating in one process.  Reported, not gated: the stream stays on the device either way.

| filter | frames shown | download path, ms / frame | device stage, ms / frame | device / download | download passes, ms | device passes, ms |
|---|---|---|---|---|---|---|
{ff_rows}

## 4. One pass at the reference's T = {one['thresh_us']} us on period chunks

`chunks_sequential` = **{one['chunks_sequential']}** (must be 0: a period chunk of 16.6 ms is one bucket of T + 1 us);
{one['events_active']} of {one['events_positive']} positive events kept.

{F.TRIED}{notes}"""


def markdown(r, notes="") -> str:
    d, parents = r["decode"], [r[k] for k in ("parent_1", "parent_2", "parent_3") if k in r and "error" not in r[k]]
    rows = []
    for name, v in d.items():
        pa = [p[name]["off_plain_ms"] for p in parents]
        spread = f"{min(pa)} .. {max(pa)}" if pa else "not measured"
        inside = ("yes" if min(pa) <= v["off_plain_ms"] <= max(pa) else f"no ({v['off_plain_ms'] / (sum(pa) / len(pa)):.3f} of the parent's mean)") if pa else "-"
        rows.append(f"| {name} | {v['words']} | {v['events']} | {v['triggers']} | {pa} | {spread} | {v['off_plain_ms']} | {inside} | {v['off_trig_ms']} | "
                    f"{v['on_trig_ms']} | {v['on_trig_ms'] - v['off_trig_ms']:+.4f} ({v['on_trig_ms'] / v['off_trig_ms']:.3f} x) | {v['rounds_ms']} |")
    c = r["chain"]
    chain_rows = "\n".join(f"| {k} | {v['frames_shown']} | {v['frames_per_s']} | {v['ms_per_frame']} | {v['ms_per_pass_median']} | {v['passes_ms']} |"
                           for k, v in c.items() if isinstance(v, dict))
    k = r.get("kernels", {})
    if "kernels" in k and k["kernels"]:
        krows = "\n".join(f"| `{n}` | {v['calls']} | {v['avg_us']} | {v['min_us']} | {v['max_us']} |" for n, v in k["kernels"].items())
        ktxt = (f"`rocprofv3 --kernel-trace --stats` of 20 pushes of the esl EVT 3.0 words ({k['words']} words, {k['events']} events, positive_only) "
                f"into a TriggeredFrames, in a process of its own; the decoder's three kernels beside the new ones.\n\n"
                f"| kernel | calls | avg us | min us | max us |\n|---|---|---|---|---|\n{krows}")
    else:
        ktxt = f"Not measured in this run: {k.get('error', 'the step did not run')}."
    return f"""# Frames cut at external trigger events: times

Written by `tools/ext_trigger_time.py` on an MI355X.  **No real triggered recording exists beside this project: the streams are
rendered** (`x_maps_amd/rig.py`'s ESL-like stand-in, 640 x 480 camera; the dense EVT 2.1 words are synthetic) and the trigger words
were put in by `insert_ext_triggers`, one per rendered frame (16.6 ms).  Every step in a process of its own.
Clock state of the box, queried idle before the first launch: {r['clock_state']}.

## Decode rate with and without extraction

`decode_device`: one chunk per call (copy through the pinned staging buffer, the launches, the count back, synchronous), the decoder
reset before every call; after warm-up the median of {r['repeats']} calls, each between two device events.  (a) the parent commit's
build, three runs in three processes; (b) this build with extraction off on the same words -- `evt3_run` issues the same three
launches, the two new ones sit behind `if (ext)` with `ext = ext && d->max_triggers`; (c) the words with the trigger words in them,
extraction off and on in alternating rounds of half the calls, the faster round of each.

| stream | words | events | triggers | (a) parent, ms | spread | (b) off, ms | inside (a)? | (c) off, ms | (c) on, ms | on - off | rounds, ms |
|---|---|---|---|---|---|---|---|---|---|---|---|
{chr(10).join(rows)}

## The triggered chain beside the pause finder

The ESL-like stream ({c['events']} events, {c['frames_rendered']} frames rendered) as EVT 3.0 words in {c['chunks']} period chunks through
`DepthReprojectionPipe.process_evt3_words`, whole passes (every chunk, flush, reset), the median of {r['passes']} after two warm-up
passes.  `ext_trigger`: the words hold a trigger 100 us in front of every frame; decode + extraction, p == 1 compaction into the
device buffer, the frames' group launches, BGR back, synchronous per chunk.  `pauses`: the same words without the triggers through
the device ingest (activity filter off, to compare like with like: the triggered chain has none).  The two cut different frames by
construction (trigger-to-trigger spans against pause-to-pause spans): the figure is the cost per shown frame, not an identity.

| frame_sync | frames shown | frames / s | ms / frame | ms / pass (median) | passes, ms |
|---|---|---|---|---|---|
{chain_rows}

## Kernel times

{ktxt}

{F.TRIED}{notes}"""


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    F.add_arguments(ap, "the parent commit's libxmaps_hip.so: (a) of the decode table; with --filters-md the three parent runs of its first table")
    ap.add_argument("--filters-md", help="measure the chain's two filters instead (profiles/ext_trigger_filters.md) and write the profile here")
    a = ap.parse_args(argv)
    if a.step in ("push", "push_off"):
        return step_push(a.repeats, a.device, off_only=a.step == "push_off")
    if a.step == "frame_filters":
        return step_frame_filters(a.passes, a.device)
    if a.step in ("filter_kernels_trig", "filter_kernels_alone"):
        return step_filter_kernels_child(a.device, a.step.rsplit("_", 1)[1])
    if a.filters_md:
        res = {"clock_state": clock_state(), "repeats": a.repeats, "passes": a.passes}
        steps = []
        for i in (1, 2, 3):  # (the box's rate drifts from process to process: the two builds take turns)
            steps += [(f"parent_{i}", "push", a.parent_lib)] if a.parent_lib else []
            steps += [(f"off_{i}", "push_off", None)]
        steps += [("push", "push", None), ("frame_filters", "frame_filters", None)]
        if F.run_steps(__file__, TAG, steps, a, res):
            res["kernels_trig"] = step_filter_kernels(a, "trig")
            res["kernels_alone"] = step_filter_kernels(a, "alone") if "error" not in res["kernels_trig"] else {"error": "not started: the trace in front of it failed"}
            print(json.dumps({k: res[k] for k in ("kernels_trig", "kernels_alone")}, indent=1))
            F.write_md(a.filters_md, res, filters_markdown)
        return res
    if a.step == "decode":
        return step_decode(a.repeats, a.device)
    if a.step == "chain":
        return step_chain(a.passes, a.device)
    if a.step == "kernels_child":
        return step_kernels_child(a.device)
    res = {"clock_state": clock_state(), "repeats": a.repeats, "passes": a.passes}
    steps = [(f"parent_{i}", "decode", a.parent_lib) for i in (1, 2, 3)] if a.parent_lib else []
    steps += [("decode", "decode", None), ("chain", "chain", None)]
    ok = F.run_steps(__file__, TAG, steps, a, res)
    if ok:
        res["kernels"] = step_kernels(a)
        print(json.dumps(res["kernels"], indent=1))
        if a.md:
            F.write_md(a.md, res, markdown)
    return res


if __name__ == "__main__":
    main()
