"""CPU: the host side of the external-trigger frames (x_maps_amd/ext_trigger.py; include/xmaps.h states the word layouts and the cut
rule).  ExtTriggerExtractor -- the NumPy host form -- against the independent word-by-word checker (tests/ext_trigger_ref.py) on
every stream the GPU test runs (tests/ext_trigger_cases.py), events and trigger records byte for byte; insert_ext_triggers there
and back; TriggerFrameCutter on literal cases worked out by hand; and the same literals against the C++ rule
(csrc/host/xm_trigger_cut.hpp), built alone with AddressSanitizer + UBSan (tests/c_host/trigger_cut_host.cpp)."""
import os
import subprocess

import numpy as np
import pytest

import ext_trigger_cases as K
import ext_trigger_ref as R
from test_k2_live_host_cpu import FLAGS, ROOT, _gxx_with_asan
from x_maps_amd import evt2, evt21, evt3
from x_maps_amd import ext_trigger as X
from x_maps_amd.synthetic import EVENT_CD_DTYPE


def _same(a, b, what):
    assert a.dtype.itemsize == b.dtype.itemsize == 16 and len(a) == len(b), (what, len(a), len(b))
    assert a.tobytes() == b.tobytes(), what


@pytest.mark.parametrize("fmt", K.FMTS)
def test_host_form_equals_the_checker(fmt):
    n_trig = 0
    for name, f, chunks, opt in K.all_cases(fmt):
        ref, host = R.machine(f, **opt), X.ExtTriggerExtractor(f, **opt)
        for i, c in enumerate(chunks):
            ev_r, tr_r = ref.feed(c)
            ev_h, tr_h = host.extract(c)
            _same(ev_h, ev_r, (name, i, "events"))
            _same(tr_h, tr_r, (name, i, "triggers"))
            n_trig += len(tr_r)
    assert n_trig > 1000


@pytest.mark.parametrize("fmt", K.FMTS)
def test_the_cases_hold_what_they_are_for(fmt):
    cases = {name: (chunks, opt) for name, _, chunks, opt in K.all_cases(fmt)}
    big = cases["past 256 blocks"][0][0]
    assert len(big) == 2048 * 257 + 5
    t = np.nonzero(K.is_trigger(fmt, big))[0]
    assert {0, len(big) - 1, 2047, 2048, 256 * 2048 - 1, 256 * 2048, 257 * 2048} <= set(t.tolist())
    assert np.any(np.diff(t) == 1) and np.any((np.diff(t)[:-1] == 1) & (np.diff(t)[1:] == 1))  # two and three adjacent
    assert K.is_trigger(fmt, cases["triggers only"][0][0]).all() and not K.is_trigger(fmt, cases["no trigger"][0][0]).any()
    _, tr = R.decode(cases["every id, both values"][0][0], fmt)
    assert sorted(zip(tr["id"].tolist(), tr["value"].tolist())) == [(i, v) for i in range(K.N_IDS[fmt]) for v in (0, 1)]
    off = R.decode(cases["in front of the first time base, wait=False"][0][0], fmt, wait_for_time_base=False)
    on = R.decode(cases["in front of the first time base, wait=True"][0][0], fmt, wait_for_time_base=True)
    assert (len(off[0]), len(off[1]), len(on[0]), len(on[1])) == (2, 4, 1, 2)
    assert on[1]["event_index"].tolist() == [0, 1] and off[1]["event_index"].tolist() == [0, 1, 1, 2]


def test_hand_derived_evt3_records():
    ev, tr = R.decode(dict((c[0], c[2]) for c in K.small_cases(3))["trigger between VECT_BASE_X and VECT_12"][0], 3)
    t = (5 << 12) | 7
    assert [tuple(int(v) for v in e) for e in ev] == [(100, 3, 1, t), (102, 3, 1, t), (112, 3, 1, t), (113, 3, 1, t), (4, 3, 0, t)]
    assert [(int(r["t"]), int(r["event_index"]), int(r["id"]), int(r["value"])) for r in tr] == [(t, 0, 2, 1), (t, 2, 3, 0)]
    _, tr = R.decode(dict((c[0], c[2]) for c in K.small_cases(3))["trigger behind a TIME_HIGH that changed without a TIME_LOW"][0], 3)
    assert tr["t"].tolist() == [(5 << 12) | 9, 6 << 12, 6 << 12, (6 << 12) | 4]
    _, tr = R.decode(dict((c[0], c[2]) for c in K.small_cases(3))["trigger behind a 24-bit wrap"][0], 3)
    assert tr["t"].tolist() == [(0xFFF << 12) | 1, (1 << 24) | (1 << 12), (1 << 24) | (1 << 12) | 2]


@pytest.mark.parametrize("fmt", (2, 21))
def test_hand_derived_loop_records(fmt):
    _, tr = R.decode(dict((c[0], c[2]) for c in K.small_cases(fmt))["trigger behind a TIME_HIGH loop"][0], fmt)
    assert tr["t"].tolist() == [(0x0FFFFFF0 << 6) | 4, (1 << 34) | (5 << 6) | 6] and tr["event_index"].tolist() == [1, 1]


def _events(n, rng, t0=5_000_000):
    ev = np.zeros(n, EVENT_CD_DTYPE)
    ev["t"] = t0 + np.sort(rng.integers(0, 40_000, n))
    ev["x"], ev["y"], ev["p"] = rng.integers(0, 640, n), rng.integers(0, 480, n), rng.integers(0, 2, n)
    return ev


@pytest.mark.parametrize("fmt,legacy", [(3, False), (2, False), (21, False), (21, True)])
def test_insert_ext_triggers_round_trips(fmt, legacy):
    rng = np.random.default_rng(fmt)
    ev = _events(500, rng)
    enc = {3: evt3.encode_evt3, 2: evt2.encode_evt2, 21: evt21.encode_evt21}[fmt]
    words = enc(ev)
    if legacy:
        words = evt21.swap_halves(words)
    at = np.array([0, 17, 17, 100, 499, 500])
    ids = np.array([0, 1, 2, 7, 15, 3])
    vals = np.array([1, 0, 1, 1, 0, 1])
    for t in (None, np.array([4_999_000, 5_000_100, 5_000_101, 5_010_000, 5_050_000, 5_060_007])):
        out = X.insert_ext_triggers(words, fmt, at, ids, vals, t=t, legacy_halves=legacy)
        assert K.is_trigger(fmt, evt21.swap_halves(out) if legacy else out).sum() == len(at)
        for dec in (lambda w: R.decode(w, fmt, legacy_halves=legacy), X.ExtTriggerExtractor(fmt, legacy_halves=legacy).extract):
            ev2, tr = dec(out)
            assert ev2.tobytes() == ev.tobytes()
            assert tr["event_index"].tolist() == at.tolist() and tr["id"].tolist() == ids.tolist() and tr["value"].tolist() == vals.tolist()
            if t is not None:
                assert tr["t"].tolist() == t.tolist()
            else:  # the stream's time at that place: the stamp of the event in front (0 at the stream's start)
                assert tr["t"].tolist() == [0] + [int(ev["t"][a - 1]) for a in at[1:]]
    with pytest.raises(ValueError):
        X.insert_ext_triggers(words, fmt, [501], legacy_halves=legacy)


def test_keep_positive_remaps_the_indices():
    ev = np.zeros(6, EVENT_CD_DTYPE)
    ev["p"] = [1, 0, 0, 1, 1, 0]
    ev["t"] = np.arange(6)
    tr = np.zeros(4, X.EXT_TRIGGER_DTYPE)
    tr["event_index"] = [0, 2, 3, 6]
    kept, out = X.keep_positive(ev, tr)
    assert kept["t"].tolist() == [0, 3, 4] and out["event_index"].tolist() == [0, 1, 1, 3]


# ---- the cut rule: the literals of tests/c_host/trigger_cut_host.cpp against the Python mirror ----
class _Cut:
    """a TriggerFrameCutter fed with events whose t is their stream index"""

    def __init__(self, **kw):
        self.c = X.TriggerFrameCutter(**kw)
        self.n = 0

    def push(self, n, trigs):
        ev = np.zeros(n, EVENT_CD_DTYPE)
        ev["t"] = self.n + np.arange(n)
        self.n += n
        tr = np.zeros(len(trigs), X.EXT_TRIGGER_DTYPE)
        for i, (idx, ident, value) in enumerate(trigs):
            tr[i] = (1000 + idx, idx, ident, value, 0)
        return self.c.push(ev, tr)

    def frames(self):
        return [(b, e) for b, e, _ in self.c.frames]

    def stamps(self, cap=1 << 30):
        return [ev["t"].tolist() for ev, _ in self.c.ready(cap)]


def test_cutter_two_chunks_and_an_unselected_edge():
    k = _Cut(cap_events=100)
    assert k.push(10, [(3, 0, 1), (7, 0, 0), (8, 0, 1)]) == 1
    assert k.frames() == [(3, 8)] and (k.c.lo, k.c.hi) == (3, 10) and int(k.c.frames[0][2]["t"]) == 1003
    assert k.push(5, [(0, 0, 1), (5, 0, 1)]) == 3
    assert k.frames() == [(3, 8), (8, 10), (10, 15)] and k.c.run(10) == 3 and k.c.run(2) == 2
    assert k.stamps() == [[3, 4, 5, 6, 7], [8, 9], [10, 11, 12, 13, 14]]
    k.c.release(3)
    assert k.frames() == [] and k.c.open and (k.c.lo, k.c.hi, k.c.stream_pos) == (15, 15, 15)
    assert k.c.stats == dict(events_in=15, events_kept=15, triggers_seen=5, triggers_selected=4, frames_cut=3, frames_skipped=0,
                             events_before_first_trigger=3, events_dropped_open_frame=0, front_moves=0)


def test_cutter_min_events_and_runs():
    k = _Cut(cap_events=100, min_events=2)
    assert k.push(12, [(0, 0, 1), (5, 0, 1), (6, 0, 1), (8, 0, 1), (12, 0, 1)]) == 2
    assert k.frames() == [(0, 5), (8, 12)] and k.c.stats["frames_cut"] == 2 and k.c.stats["frames_skipped"] == 2
    assert k.c.run(10) == 1 and k.stamps() == [[0, 1, 2, 3, 4]]
    k.c.release(1)
    assert k.c.run(10) == 1 and k.stamps() == [[8, 9, 10, 11]] and k.c.lo == 8


def test_cutter_max_frames_ready():
    k = _Cut(cap_events=100, max_frames_ready=2)
    assert k.push(6, [(0, 0, 1), (1, 0, 1), (2, 0, 1), (3, 0, 1), (4, 0, 1)]) == 4
    assert k.c.run(10) == 2 and k.c.run(1) == 1
    k.c.release(2)
    assert k.c.run(10) == 2 and k.frames()[0] == (2, 3)
    k.c.release(2)
    assert k.c.run(10) == 0 and (k.c.lo, k.c.hi) == (4, 6)


def test_cutter_adjacent_triggers_cut_empty_frames():
    k = _Cut(cap_events=100)
    assert k.push(4, [(2, 0, 1)] * 3) == 2
    assert k.frames() == [(2, 2), (2, 2)] and k.c.run(10) == 2 and k.c.stats["events_before_first_trigger"] == 2
    assert k.stamps() == [[], []]
    s = _Cut(cap_events=100, min_events=1)
    assert s.push(4, [(2, 0, 1)] * 3) == 0 and s.c.stats["frames_skipped"] == 2


def test_cutter_channel_and_edge_selection():
    trigs = [(1, 1, 1), (2, 0, 0), (3, 1, 0), (5, 1, 0)]
    k = _Cut(cap_events=100, id=1, edge="falling")
    assert k.push(6, trigs) == 1
    assert k.frames() == [(3, 5)] and int(k.c.frames[0][2]["id"]) == 1
    assert (k.c.stats["triggers_seen"], k.c.stats["triggers_selected"], k.c.stats["events_before_first_trigger"]) == (4, 2, 3)
    b = _Cut(cap_events=100, edge="both")
    assert b.push(6, trigs) == 3 and b.frames() == [(1, 2), (2, 3), (3, 5)]


def test_cutter_front_moves_and_a_dropped_open_frame():
    k = _Cut(cap_events=10)
    k.push(6, [(4, 0, 1)])
    assert (k.c.lo, k.c.hi) == (4, 6)
    k.push(5, [(3, 0, 1)])
    assert k.frames() == [(0, 5)] and k.c.hi == 7 and k.c.stats["front_moves"] == 1 and k.stamps() == [[4, 5, 6, 7, 8]]
    k.c.release(1)
    assert k.c.lo == 5
    k.push(4, [])
    assert k.c.hi == 6 and k.c.stats["front_moves"] == 2 and k.c.buf["t"][:6].tolist() == [9, 10, 11, 12, 13, 14]
    k.push(5, [])  # 6 + 5 > 10: the open frame goes
    assert not k.c.open and k.c.stats["events_dropped_open_frame"] == 11 and k.c.hi == 0
    k.push(3, [(1, 0, 1)])
    assert k.c.stats["events_dropped_open_frame"] == 12 and k.c.open and k.c.open_pos == 1
    k.push(2, [(2, 0, 1)])
    assert k.frames() == [(1, 5)] and k.stamps() == [[21, 22, 23, 24]]
    assert k.c.stats == dict(events_in=25, events_kept=25, triggers_seen=4, triggers_selected=4, frames_cut=2, frames_skipped=0,
                             events_before_first_trigger=4, events_dropped_open_frame=12, front_moves=2)
    assert k.c.stream_pos == 25


def test_cutter_unreleased_frames_leave_no_room():
    k = _Cut(cap_events=10)
    k.push(8, [(0, 0, 1), (8, 0, 1)])
    assert k.frames() == [(0, 8)]
    with pytest.raises(ValueError):
        k.push(5, [])
    assert k.frames() == [(0, 8)]
    k.c.release(1)
    k.push(5, [(1, 0, 1)])
    assert k.c.stats["events_dropped_open_frame"] == 1 and k.c.open_pos == 1


def test_cutter_reset_and_clipped_index():
    k = _Cut(cap_events=100)
    k.push(10, [(3, 0, 1), (8, 0, 1)])
    k.c.reset()
    assert k.frames() == [] and not k.c.open and k.c.stream_pos == 0
    k.push(3, [])
    assert k.c.stats["events_before_first_trigger"] == 6 and k.c.hi == 0 and k.c.stats["frames_cut"] == 1
    c = _Cut(cap_events=100)
    c.push(4, [(0, 0, 1), (9, 0, 1)])
    assert c.frames() == [(0, 4)] and c.c.open_pos == 4


def test_cut_rule_in_cpp_under_address_and_ub_sanitizers(tmp_path):
    gxx = _gxx_with_asan(tmp_path)
    exe = tmp_path / "trigger_cut_host"
    subprocess.run([gxx] + FLAGS + [os.path.join(ROOT, "tests", "c_host", "trigger_cut_host.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip() == "ok"
