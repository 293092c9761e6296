#!/usr/bin/env python3
"""Time the frame -> EVT 3.0 entry and the ingest's record stage on the ESL-like stream.

    python tools/evt3_record_time.py [--md profiles/evt3_record.md] [--repeats 20] [--parent-lib PATH]

NOT the benchmark (bench.py measures the flagship workload); this gives the numbers of profiles/evt3_record.md.  The frames are
the ones `bench.py --esl` renders (x_maps_amd/rig.py's ESL-like stand-in: the reference's calibration numbers, a rendered scene) --
the ESL recordings are not available here, and the output says so.

The parent process never opens the GPU: every step runs in a fresh child process under its own time limit (--step-timeout), and no
further step is started after one that failed or ran out of time.
  group    xm_frames_to_evt3_words on a group of 32 frames, device-resident (records in, words out, the final synchronise), with
           vector words and without: after warm-up the median of --repeats calls, each between two device events
           (tools/_timing.py); words and bytes per event; evt3.encode_evt3_singles (NumPy) on the same group, host clock.  Every
           frame's words are compared with the host encoder's (vectors: evt3.encode_evt3 on the first frame, the loop encoder).
           A third row: the same group with the stamps rounded down to 32 us, so that vector runs exist.
  ingest   the ESL-like stream (48 frames, quarter-period packets of pinned records, activity filter on, BGR frames out) through
           one DeviceIngest, whole passes alternating stage off / on in ONE process, the median pass of each reported; with
           --parent-lib (a build of the parent commit's library, XM_LIB) the same stage-off passes on that build in processes of
           their own, alternating with this build's: this, parent, this, parent."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _frame_stage as F  # noqa: E402
from _frame_stage import GROUP, HBM_BYTES_PER_S  # noqa: E402
from _timing import clock_state, timed  # noqa: E402

MAX_WORDS = 1 << 21
NEW_SYMBOLS = ("xm_frames_to_evt3_words", "xm_ingest_set_record_output", "xm_ingest_copy_record")


def step_group(repeats, device):
    F.gpu()
    import ctypes as C

    import evt3_record_cases as K
    from x_maps_amd import XMapsEngine, evt3, rig
    from x_maps_amd import _native as N
    cp, tables, _, _ = rig.make_esl_like(row_stride=13, device=device)
    frames = [rig.render_events(cp, dict(tables), row_stride=13, seed=f)[0] for f in range(GROUP)]
    evs, offs = K.concat(frames)
    res = {"frames": GROUP, "events_per_frame": int(len(evs)) // GROUP}
    t0 = time.perf_counter()
    singles = [evt3.encode_evt3_singles(f) for f in frames]
    res["numpy_singles_ms_per_group"] = round((time.perf_counter() - t0) * 1e3, 2)
    t0 = time.perf_counter()
    first_vect = evt3.encode_evt3(frames[0], True)
    res["python_loop_encoder_ms_per_frame"] = round((time.perf_counter() - t0) * 1e3, 1)
    with XMapsEngine(tables, device=device) as eng:
        d_ev = eng.to_device(evs)
        d_out = eng.dev_alloc(max(len(evs), 1) * 8)
        op = offs.ctypes.data_as(C.POINTER(C.c_uint64))
        # the rendered frames' stamps are all different, so no two events are linked and vector words never occur; the same frames
        # with the stamps rounded down to 32 us and the events of a stamp in raster order have chains and runs
        coarse = []
        for f in frames:
            c = f.copy()
            c["t"] = c["t"] // 32 * 32
            coarse.append(c[np.lexsort((c["x"], c["y"], c["t"]))])
        for name, vec in (("vectors", True), ("singles", False), ("vectors_coarse_stamps", True)):
            if name == "vectors_coarse_stamps":
                frames = coarse
                evs, offs = K.concat(frames)
                op = offs.ctypes.data_as(C.POINTER(C.c_uint64))
                eng.dev_upload(d_ev, evs)
            words, stats = eng.frames_to_evt3_words(frames, use_vectors=vec)
            if name == "vectors":
                assert np.array_equal(words[0], first_vect), "the first frame's words differ from encode_evt3's"
            elif name == "singles":
                assert all(np.array_equal(w, s) for w, s in zip(words, singles)), "words differ from encode_evt3_singles'"
            else:
                ref = evt3.encode_evt3(frames[0][:12000], True)[:-8]  # (a prefix of the frame: all but the words of its last runs)
                assert np.array_equal(words[0][:len(ref)], ref), "coarse stamps: words differ from encode_evt3's"
            n_words = sum(len(w) for w in words)

            def call():
                N.check(eng._lib.xm_frames_to_evt3_words(eng._h, C.c_void_p(d_ev), op, GROUP, int(vec), N.XM_MEM_DEVICE, C.c_void_p(d_out), None))
                eng.sync()
            t = timed(call, repeats)
            # what the passes move: the record of every event up to three times in R0 (itself, its predecessor, its successor: the
            # last two from the cache) and once in R3, the 2-byte code written and read twice, the words, the counts and offsets
            moved = len(evs) * (32 + 6) + n_words * 2 + (len(evs) // 64) * 16
            res[name] = {
                "ms_per_group_device_events": round(t.ev, 4), "min_max_ms": [round(t.ev_min, 4), round(t.ev_max, 4)],
                "ms_per_group_host_clock": round(t.host, 4), "us_per_frame": round(t.ev / GROUP * 1e3, 2),
                "Gevents_per_s": round(len(evs) / (t.ev * 1e-3) / 1e9, 3), "words_per_event": round(n_words / len(evs), 3),
                "bytes_per_event": round(2 * n_words / len(evs), 3), "vector_runs_per_frame": sum(s.n_vector_runs for s in stats) // GROUP,
                "event_stream_share_of_hbm_rate": round(len(evs) * 16 / HBM_BYTES_PER_S / (t.ev * 1e-3), 4),
                "bytes_moved_per_group": int(moved), "moved_share_of_hbm_rate": round(moved / HBM_BYTES_PER_S / (t.ev * 1e-3), 4)}
        t = timed(lambda: eng.frames_to_evt3_words(frames), max(3, repeats // 4))
        res["ms_per_group_from_host_memory"] = round(t.host, 3)
        eng.dev_free(d_out)
        eng.dev_free(d_ev)
    print("ENC_STEP " + json.dumps(res), flush=True)


def step_ingest(passes, device, with_stage):
    def check(ing, got, on):  # the stage ran for the pass's frames, or for none of them
        held = [ing.record(fr.seq) for fr in got]
        assert all((h is not None and h[0] is not None and len(h[0]) == h[1].n_words > 0 and h[1].n_events == fr.n_events) if on else h is None
                   for h, fr in zip(held, got))
    set_stage = (lambda ing, on: ing.set_record_output(on, True, MAX_WORDS)) if with_stage else None
    print("ENC_STEP " + json.dumps(F.ingest_passes(passes, device, NEW_SYMBOLS, set_stage, check)), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    F.add_arguments(ap, "a build of the parent commit's library: its stage-off passes, in processes of their own")
    a = ap.parse_args(argv)
    if a.step == "group":
        return step_group(a.repeats, a.device)
    if a.step in ("ingest", "ingest_off_only"):
        return step_ingest(a.passes, a.device, a.step == "ingest")
    res = {"frames": F.FRAMES_NOTE, "clock_state": clock_state(), "repeats": a.repeats, "passes": a.passes}
    steps = [("group", "group", None), ("ingest", "ingest", None)]
    if a.parent_lib:
        lib = os.path.abspath(a.parent_lib)
        steps += [("ingest_parent_build", "ingest_off_only", lib), ("ingest_again", "ingest", None), ("ingest_parent_build_again", "ingest_off_only", lib)]
    if F.run_steps(__file__, "ENC_STEP ", steps, a, res) and a.md:
        F.write_md(a.md, res, markdown)
    return res


def markdown(r, notes="") -> str:
    g, i = r["group"], r["ingest"]
    off, on = i["stage_off"], i["stage_on"]
    runs = [("this build, stage off", off), ("this build, stage on", on)]
    par = [r[k]["stage_off"] for k in ("ingest_parent_build", "ingest_parent_build_again") if k in r]
    if par:
        runs += [("parent commit's build (stage absent), run 1", par[0]), ("this build, stage off, run 2", r["ingest_again"]["stage_off"]),
                 ("this build, stage on, run 2", r["ingest_again"]["stage_on"]), ("parent commit's build, run 2", par[1])]
        mine = np.mean([off["Mevents_per_s"], r["ingest_again"]["stage_off"]["Mevents_per_s"]])
        theirs = np.mean([p["Mevents_per_s"] for p in par])
        par_note = (f"Stage off against the parent's build, means of the two alternating runs: {mine:.1f} / {theirs:.1f} = {mine / theirs:.3f} "
                    f"(the README states a +-6 % run-to-run spread for this stream).")
    else:
        par_note = "The parent commit's build was not timed in this run (--parent-lib)."

    def row(name, d):
        return (f"| {name} | {d['ms_per_group_device_events']} ({d['min_max_ms'][0]} .. {d['min_max_ms'][1]}) | {d['us_per_frame']} | {d['Gevents_per_s']} | "
                f"{d['words_per_event']} | {d['bytes_per_event']} | {d['vector_runs_per_frame']} | {d['bytes_moved_per_group'] / 1e6:.1f} | {d['moved_share_of_hbm_rate']} |")
    n_ev = g["frames"] * g["events_per_frame"]
    return F.md_head("Frames of events -> EVT 3.0 words", "evt3_record_time.py", r["clock_state"]) + f"""
## The group entry (`xm_frames_to_evt3_words`)

A group of {g['frames']} frames of {g['events_per_frame']} events, records and words device-resident, four launches and the final
synchronise.  Median of {r['repeats']} calls after warm-up, each between two device events.

| words | ms / group (min .. max) | us / frame | Gev/s | words / event | bytes / event | vector runs / frame | MB moved / group | moved bytes at 6.29 TB/s |
|---|---|---|---|---|---|---|---|---|
{row("vectors on", g['vectors'])}
{row("vectors off", g['singles'])}
{row("vectors on, stamps rounded to 32 us", g['vectors_coarse_stamps'])}

Host clock around the vectors-on call: {g['vectors']['ms_per_group_host_clock']} ms.  From host memory (records up, valid words and
statistics back, synchronous): {g['ms_per_group_from_host_memory']} ms / group.  On the host of the same box,
`evt3.encode_evt3_singles` (NumPy) takes {g['numpy_singles_ms_per_group']} ms for the group
({n_ev / max(g['numpy_singles_ms_per_group'], 1e-9) / 1e6:.4f} Gev/s) and the loop encoder `evt3.encode_evt3`
{g['python_loop_encoder_ms_per_frame']} ms for ONE frame.  An EventCD record is 16 bytes.

The rendered frames' stamps are all different: no two events are linked, vector words never occur, and the first two rows write
the same words.  The third row is the same group with every stamp rounded down to 32 us and the events of a stamp in raster
order, so that chains and runs exist and R0's walk has work to do.

"Moved" counts what the four passes move: every record read in R0 (with its neighbours, which come from the cache) and in R3, the
2-byte code written once and read twice, the words, and the 64-event counts and offsets.  A group this small lies inside the
Infinity Cache, and its four launches are a visible part of the time.

""" + F.md_ingest(r, "xm_ingest_set_record_output", f"; max_words = {MAX_WORDS}, vector words on", F.run_rows(runs), par_note, notes)


if __name__ == "__main__":
    main()
