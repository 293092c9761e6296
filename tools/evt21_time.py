#!/usr/bin/env python3
"""Time the EVT 2.1 and DAT decoders: the NumPy decoder, Device*Decoder.decode_device with both EVT 2.1 emit kernels, push into
the ingest -- and, in the same run, the same events as EVT 2.0 and EVT 3.0 words through the existing decoders.

    python tools/evt21_time.py [--md profiles/evt21.md] [--repeats 20] [--passes 7]

NOT the benchmark (bench.py measures the flagship workload); this gives the numbers of profiles/evt21.md.  Two streams:
  esl     the ESL-like stream (x_maps_amd/rig.py's stand-in: the reference's calibration numbers, a rendered scene, 8 frames) --
          the ESL recordings are not available here; encoded with vectors on, so a word is whatever runs the stream has
  dense   2^18 synthetic EVT 2.1 words on a 640 x 480 sensor, a TIME_HIGH every 64 words, every mask the OR of two random ones
          (>= 16 events per word is asserted): what the emit kernel was shaped for
The parent process never opens the GPU: every step runs in a fresh child process under its own time limit (--step-timeout), and no
further step is started after one that failed or ran out of time.
  decode  per stream and format: the host decoder once (host clock); decode_device (pageable words in, records device-resident,
          synchronous) after warm-up, the median of --repeats calls between two device events, in Mev/s and input GB/s.  The two
          EVT 2.1 emit kernels (the per-word loop; by output slot, "XM_EVT21_EMIT_BY_WORD" = 0) are two decoders in ONE process, timed
          in alternating rounds.  Every decoder's records are compared with the host decoder's first.
  push    the esl stream in period chunks (count left on the device) through one DeviceIngest per format, whole passes (push
          everything, flush, poll, reset), the median of --passes; the same packets as EventCD records beside them."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _frame_stage as F  # noqa: E402
from _timing import clock_state, timed  # noqa: E402

ESL_FRAMES = 8


def esl_stream(device):
    from x_maps_amd import rig
    cp, tables, _, _ = rig.make_esl_like(row_stride=13, device=device)
    stream, _ = rig.render_stream(cp, tables, n_frames=ESL_FRAMES, row_stride=13, seed=9)
    return tables, stream


def dense_words(n=1 << 18, seed=7):
    rng = np.random.default_rng(seed)
    mask = rng.integers(0, 1 << 32, n, dtype=np.uint64) | rng.integers(0, 1 << 32, n, dtype=np.uint64)
    mask |= np.uint64(0xFFFF) << (rng.integers(0, 2, n).astype(np.uint64) * np.uint64(16))  # (never fewer than 16 bits)
    i = np.arange(n, dtype=np.uint64)
    top = (rng.integers(0, 2, n).astype(np.uint64) << np.uint64(28)) | ((i % np.uint64(64)) << np.uint64(22)) \
        | ((rng.integers(0, 20, n).astype(np.uint64) * np.uint64(32)) << np.uint64(11)) | rng.integers(0, 480, n).astype(np.uint64)
    w = (top << np.uint64(32)) | mask
    is_hi = i % np.uint64(64) == 0
    w[is_hi] = (np.uint64(0x8) << np.uint64(60)) | ((i[is_hi] // np.uint64(64) + np.uint64(1000)) << np.uint64(32))
    return w.astype("<u8")


def encodings(evs, w21):
    """the same events in every format: name -> (words, host decoder factory, device decoder class)"""
    from x_maps_amd import dat, evt2, evt21, evt3
    return {"EVT 2.1": (w21, evt21.Evt21Decoder, evt21.DeviceEvt21Decoder),
            "DAT": (dat.encode_dat(evs), dat.DatDecoder, dat.DeviceDatDecoder),
            "EVT 2.0": (evt2.encode_evt2(evs), evt2.Evt2Decoder, evt2.DeviceEvt2Decoder),
            "EVT 3.0": (evt3.encode_evt3(evs) if len(evs) < 1_000_000 else evt3.encode_evt3_singles(evs), evt3.Evt3Decoder, evt3.DeviceEvt3Decoder)}


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(a[k], b[k]) for k in ("x", "y", "p", "t"))


def _rate(n_events, n_bytes, t):
    return {"ms_device_events": round(t.ev, 4), "min_max_ms": [round(t.ev_min, 4), round(t.ev_max, 4)],
            "Mevents_per_s": round(n_events / (t.ev * 1e-3) / 1e6, 1), "input_GB_per_s": round(n_bytes / (t.ev * 1e-3) / 1e9, 3)}


def step_decode(repeats, device):
    F.gpu()
    from x_maps_amd import XMapsEngine, evt21
    from x_maps_amd import _native as N
    tables, stream = esl_stream(device)
    dense = dense_words()
    dense_evs = evt21.decode_evt21(dense)
    assert len(dense_evs) >= 16 * (len(dense) - len(dense) // 64)
    res = {}
    with XMapsEngine(tables, device=device) as eng:
        for sname, evs, w21 in (("esl", stream, evt21.encode_evt21(stream)), ("dense", dense_evs, dense)):
            out = res[sname] = {"events": int(len(evs)), "formats": {}}
            for fname, (words, host_cls, dev_cls) in encodings(evs, w21).items():
                t0 = time.perf_counter()
                host = host_cls().decode(words)
                host_s = time.perf_counter() - t0
                assert _same(host, evs), (sname, fname)
                row = out["formats"][fname] = {"words": int(len(words)), "bytes": int(words.nbytes), "events_per_word": round(len(evs) / len(words), 3),
                                               "numpy_host_ms": round(host_s * 1e3, 2), "numpy_host_Mevents_per_s": round(len(evs) / host_s / 1e6, 2)}
                variants = {"by_slot": "0", "by_word": "1"} if fname == "EVT 2.1" else {"": None}
                decs = {}
                for v, opt in variants.items():
                    N.debug_option("XM_EVT21_EMIT_BY_WORD", opt)
                    decs[v] = dev_cls(eng, max_words=len(words), max_events=len(evs))
                N.debug_option("XM_EVT21_EMIT_BY_WORD", None)
                for v, dec in decs.items():
                    assert _same(dec.decode(words), evs), (sname, fname, v)
                    dec.reset()
                rounds = {v: [] for v in decs}
                for _ in range(2):  # alternating rounds in one process
                    for v, dec in decs.items():
                        rounds[v].append(timed(lambda d=dec: (d.reset(), d.decode_device(words)), max(3, repeats // 2)))
                for v, ts in rounds.items():
                    best = min(ts, key=lambda t: t.ev)
                    r = _rate(len(evs), words.nbytes, best)
                    r["rounds_ms"] = [round(t.ev, 4) for t in ts]
                    row["device" + ("_" + v if v else "")] = r
                for dec in decs.values():
                    dec.close()
    print("EVT21_STEP " + json.dumps(res), flush=True)


def step_push(passes, device):
    F.gpu()
    from x_maps_amd import XMapsEngine, evt21
    from x_maps_amd.ingest import DeviceIngest
    tables, stream = esl_stream(device)
    period = int(1e6 / 60)
    cuts = np.searchsorted(stream["t"], np.arange(stream["t"][0], stream["t"][-1] + period, period))
    packets = [stream[a:b] for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
    res = {"events": int(len(stream)), "packets": len(packets), "formats": {}}
    per = [encodings(pk, evt21.encode_evt21(pk)) for pk in packets]
    max_pk = max(len(pk) for pk in packets)
    frames = None
    with XMapsEngine(tables, device=device, n_slots=4) as eng:
        for fname in ("records", "EVT 2.1", "DAT", "EVT 2.0", "EVT 3.0"):
            with DeviceIngest(eng, 60, capacity_events=1 << 21, max_packet_events=max(1 << 18, max_pk), result_ring=ESL_FRAMES + 2,
                              want_depth=False, want_bgr=True, activity_filter=True) as ing:
                if fname == "records":
                    chunks, dec = packets, None
                    push = ing.push
                else:
                    chunks = [p[fname][0] for p in per]
                    dec = per[0][fname][2](eng, max_words=max(len(c) for c in chunks))
                    push = lambda c, d=dec: d.push(ing, c, count=False)  # noqa: E731

                def one_pass():
                    c0 = time.perf_counter()
                    for c in chunks:
                        push(c)
                    ing.flush()
                    got = ing.poll(copy=False)
                    dt = time.perf_counter() - c0
                    sums = [(f.n_events, f.t_first, f.t_last) for f in got]
                    ing.reset()
                    if dec is not None:
                        dec.reset()
                    return dt, sums
                one_pass(), one_pass()
                ts = []
                for _ in range(passes):
                    dt, sums = one_pass()
                    ts.append(dt)
                    frames = sums if frames is None else frames
                    assert sums == frames, f"{fname}: the frames differ from the first format's"
                if dec is not None:
                    dec.close()
                med = float(np.median(ts))
                res["formats"][fname] = {"Mevents_per_s": round(len(stream) / med / 1e6, 1), "ms_per_pass_median": round(med * 1e3, 3),
                                         "passes_ms": [round(x * 1e3, 3) for x in ts],
                                         "bytes_in": int(sum(c.nbytes for c in chunks)) if dec is not None else int(len(stream)) * 16}
    res["frames_cut"] = len(frames)
    print("EVT21_STEP " + json.dumps(res), flush=True)


def markdown(r, notes="") -> str:
    d, p = r["decode"], r["push"]

    def rows(s):
        out = []
        for fname, f in d[s]["formats"].items():
            for key in [k for k in f if k.startswith("device")]:
                v = f[key]
                label = fname + {"device": "", "device_by_slot": ", emit by output slot", "device_by_word": ", emit by word"}[key]
                out.append(f"| {label} | {f['words']} | {f['events_per_word']} | {f['numpy_host_Mevents_per_s']} | {v['ms_device_events']} "
                           f"({v['min_max_ms'][0]} .. {v['min_max_ms'][1]}) | {v['Mevents_per_s']} | {v['input_GB_per_s']} | {v['rounds_ms']} |")
        return "\n".join(out)

    def ratio(s):
        f = d[s]["formats"]["EVT 2.1"]
        return f["device_by_word"]["ms_device_events"] / f["device_by_slot"]["ms_device_events"]
    kept = "by output slot (`k_evt21_emit`)" if ratio("dense") >= 1.0 else "by word (`k_evt21_emit_words`)"
    push_rows = "\n".join(f"| {k} | {v['bytes_in'] / 1e6:.2f} | {v['Mevents_per_s']} | {v['ms_per_pass_median']} | {v['passes_ms']} |"
                          for k, v in p["formats"].items())
    head = ("| format | words | events / word | NumPy on the host, Mev/s | decode_device ms (min .. max) | Mev/s | input GB/s | rounds, ms |\n"
            "|---|---|---|---|---|---|---|---|\n")
    return f"""# EVT 2.1 and DAT on the device: times

Written by `tools/evt21_time.py` on an MI355X.  **The esl stream is rendered** from `x_maps_amd/rig.py`'s ESL-like stand-in (640 x 480
camera, {ESL_FRAMES} frames), not the ESL recordings; the dense stream is synthetic.  Every step in a process of its own.
Clock state of the box, queried idle before the first launch: {r['clock_state']}.

**Nothing was measured before this**: the parent commit has neither decoder.  These are first numbers, not a bar.  The EVT 2.0
and EVT 3.0 legs were measured in the same run on the **unchanged** kernels (`xmaps_evt2.hpp`, `xmaps_evt3.hpp` are textually
the parent's).

## `decode_device`: pageable words in, records device-resident

One chunk per call (copy through the pinned staging buffer, three launches, the count back, synchronous), the decoder reset before
every call.  After warm-up, {r['repeats']} calls per decoder in two alternating rounds of half that, each call between two
device events; the faster round's median is the figure, both rounds are listed.  Every decoder's records were first compared
with the host decoder's, and those with the stream.  Input GB/s is the format's own bytes over the same time.

### esl: {d['esl']['events']} events

{head}{rows('esl')}

### dense: {d['dense']['events']} events

{head}{rows('dense')}

## The emit kernel that was kept

EVT 2.1's per-word loop over by-output-slot, time ratio: **{ratio('dense'):.2f}** on the dense stream, **{ratio('esl'):.2f}** on the esl
stream (above 1: the slot kernel is faster; below: the per-word loop).  The faster one on the dense stream, the case the two
differ in: **{kept}**.  The decoder launches the per-word loop; the slot kernel stays reachable through the debug option
`XM_EVT21_EMIT_BY_WORD` = 0 so that this table can be measured again, and both are pinned by `tests/test_gpu_evt21.py`.

## `push` into the ingest

The esl stream ({p['events']} events, {p['frames_cut']} frames cut) in {p['packets']} period chunks, the count left on the device
(`count=False`), pageable words, activity filter on, BGR frames out; whole passes (push everything, flush, poll, reset), the
median of {r['passes']} after two warm-up passes; one ingest per format, one after the other in one process.  Every format's
frames (event count, first and last stamp) equal the records'.  The dense stream was not pushed: it is no projector stream.

| input | MB in / pass | Mev/s | ms / pass (median) | passes, ms |
|---|---|---|---|---|
{push_rows}

{F.TRIED}{notes}"""


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    F.add_arguments(ap, argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if a.step == "decode":
        return step_decode(a.repeats, a.device)
    if a.step == "push":
        return step_push(a.passes, a.device)
    res = {"clock_state": clock_state(), "repeats": a.repeats, "passes": a.passes}
    if F.run_steps(__file__, "EVT21_STEP ", [("decode", "decode", None), ("push", "push", None)], a, res) and a.md:
        F.write_md(a.md, res, markdown)
    return res


if __name__ == "__main__":
    main()
