"""-m gpu: the device EVT 2.1 decoder (csrc/xmaps_evt21.hpp: the word state machine as three scan launches, either emit
kernel) against the independent word-by-word checker (tests/evt21_ref.py) and the hand-derived sequences of
tests/test_evt21.py -- x, y, p, t and the count exactly.  Every case first asserts on its words that the stream has what it is
for.  Then in front of the device ingest (== the same events as DAT records == as EventCD packets), through the processor's
methods, and a RAW / DAT file through tools/run_esl_on_arrival.py."""
import os

import numpy as np
import pytest

import evt21_ref as ER
import ingest_helpers as IH
from test_evt21 import HAND, HAND_WAIT, _same, _tuples, clustered_events, random_words, th, vec
from x_maps_amd import XMapsEngine, dat, evt21, evt3
from x_maps_amd import _native as N
from x_maps_amd import synthetic as S

pytestmark = pytest.mark.gpu
PER_BLOCK = 2048  # csrc/xmaps_evt.hpp: EVT_PER_BLOCK
ONES = 0xFFFFFFFF


@pytest.fixture(scope="module")
def eng():
    with XMapsEngine(S.make_tables(S.C_TINY)) as e:
        yield e


@pytest.fixture(params=["by_slot", "by_word"])
def emit(request):
    """both emit kernels ship (the slot kernel behind a debug option, read when a decoder is created): both are pinned"""
    N.debug_option("XM_EVT21_EMIT_BY_WORD", "1" if request.param == "by_word" else "0")
    yield request.param
    N.debug_option("XM_EVT21_EMIT_BY_WORD", None)


def _u8(words):
    return np.array(words, dtype="<u8")


def _kinds(w):
    return (w >> np.uint64(60)).astype(np.int64)


def _popcounts(w):
    return np.unpackbits((w & np.uint64(ONES)).astype("<u4").view(np.uint8).reshape(-1, 4), axis=1).sum(axis=1)


def _cat(*parts):
    out = np.zeros(sum(len(p) for p in parts), S.EVENT_CD_DTYPE)
    o = 0
    for p in parts:
        out[o:o + len(p)] = p
        o += len(p)
    return out


def test_hand_derived_sequences(eng, emit):
    for words, want in HAND:
        with evt21.DeviceEvt21Decoder(eng, max_words=64) as dec:
            assert _tuples(dec.decode(_u8(words))) == want
    for words, want_off, want_on in HAND_WAIT:
        for wait, want in ((False, want_off), (True, want_on)):
            with evt21.DeviceEvt21Decoder(eng, max_words=64, wait_for_time_base=wait) as dec:
                assert _tuples(dec.decode(_u8(words))) == want


def test_emit_trips(eng, emit):
    """block 0 emits 65 536 records (256 trips of the slot loop), block 1 none, block 2 one per word, the tail is mixed"""
    rng = np.random.default_rng(1)
    b0 = [vec(int(rng.integers(0, 2)), int(rng.integers(0, 64)), 32 * int(rng.integers(0, 40)), int(rng.integers(0, 720)), ONES) for _ in range(PER_BLOCK)]
    b1 = [th(int(v), int(rng.integers(0, 1 << 32))) for v in np.sort(rng.integers(1, 1 << 20, PER_BLOCK))]
    b2 = [vec(int(rng.integers(0, 2)), int(rng.integers(0, 64)), 32 * int(rng.integers(0, 40)), int(rng.integers(0, 720)), 1 << int(rng.integers(0, 32)))
          for _ in range(PER_BLOCK)]
    tail = [th(1 << 21), vec(1, 3, 96, 5, 0xF0F0F0F0), (0xA << 60) | ONES, vec(0, 4, 96, 5, 0), vec(0, 5, 7, 6, 0x80000001)]
    w = _u8(b0 + b1 + b2 + tail)
    pc, k = _popcounts(w), _kinds(w)
    assert len(w) == 3 * PER_BLOCK + 5
    assert (k[:PER_BLOCK] <= 1).all() and (pc[:PER_BLOCK] == 32).all()
    assert (k[PER_BLOCK:2 * PER_BLOCK] == 8).all()
    assert (k[2 * PER_BLOCK:3 * PER_BLOCK] <= 1).all() and (pc[2 * PER_BLOCK:3 * PER_BLOCK] == 1).all()
    ref = ER.decode(w)
    assert len(ref) == 65536 + PER_BLOCK + 16 + 2
    with evt21.DeviceEvt21Decoder(eng, max_words=len(w), max_events=len(ref)) as dec:
        assert _same(dec.decode(w), ref)


def test_block_edge(eng, emit):
    """a 32-event word is the last word of block 0, another the first word of block 1"""
    rng = np.random.default_rng(2)
    w = random_words(PER_BLOCK + 1, 12)
    w[0] = th(77)
    w[PER_BLOCK - 1] = vec(1, 9, 64, 11, ONES)
    w[PER_BLOCK] = vec(0, 10, 96, 12, ONES)
    assert len(w) == 2049 and _popcounts(w)[PER_BLOCK - 1] == 32 == _popcounts(w)[PER_BLOCK] and (_kinds(w)[PER_BLOCK - 1:] <= 1).all()
    ref = ER.decode(w)
    assert _tuples(ref[-32:]) == [(96 + n, 12, 0, int(ref["t"][-1])) for n in range(32)]
    with evt21.DeviceEvt21Decoder(eng, max_words=len(w), max_events=len(ref)) as dec:
        assert _same(dec.decode(w), ref)
        dec.reset()
        cut = int(rng.integers(1, PER_BLOCK))
        sm = ER.Evt21StateMachine()
        for piece in (w[:cut], w[cut:PER_BLOCK], w[PER_BLOCK:]):
            assert _same(dec.decode(piece), sm.feed(piece))


@pytest.fixture(scope="module")
def long_chunk():
    """526 000 uniformly random words and the checker's events, computed once"""
    w = random_words(526_000, 49)
    return w, ER.decode(w)


def test_prefix_carry_second_trip(eng, long_chunk):
    """more than 256 blocks: the prefix kernel's carry goes into a second trip; then the same words cut inside that trip"""
    w, ref = long_chunk
    hi = (w[_kinds(w) == 8] >> np.uint64(32)).astype(np.int64) & 0x0FFFFFFF
    assert len(w) > 256 * PER_BLOCK and ((hi[:-1] - hi[1:]) > (1 << 27)).sum() > 100 and len(ref) > (1 << 20)
    with evt21.DeviceEvt21Decoder(eng, max_words=len(w), max_events=1 << 21) as dec:
        assert _same(dec.decode(w), ref)
        dec.reset()
        cut = 256 * PER_BLOCK + 1000
        sm = ER.Evt21StateMachine()
        a, b = sm.feed(w[:cut]), sm.feed(w[cut:])
        assert len(a) + len(b) == len(ref)
        assert _same(dec.decode(w[:cut]), a)
        assert _same(dec.decode(w[cut:]), b)


def test_prefix_carry_second_trip_slot_emit(eng, long_chunk, emit):
    if emit != "by_slot":
        return  # (the default kernel's run is the case above)
    w, ref = long_chunk
    with evt21.DeviceEvt21Decoder(eng, max_words=len(w), max_events=1 << 21) as dec:
        assert _same(dec.decode(w), ref)


@pytest.mark.parametrize("use_vectors", [True, False])
def test_loops(eng, emit, use_vectors):
    """encoded events across t = 2^34 and t = 2^35, whole and in chunks"""
    ev = _cat(clustered_events(3000, (1 << 34) - 6000, seed=4), clustered_events(3000, (1 << 35) - 6000, seed=5))
    assert ev["t"][0] < (1 << 34) < ev["t"][2999] < (1 << 35) - 6000 <= ev["t"][3000] < (1 << 35) < ev["t"][-1]
    # the second loop needs a TIME_HIGH in between that is not itself a fall-back: the clock at 2^34 + 2^33
    mid = np.zeros(1, S.EVENT_CD_DTYPE)
    mid["t"], mid["x"], mid["y"], mid["p"] = (1 << 34) + (1 << 33), 3, 4, 1
    ev = _cat(ev[:3000], mid, ev[3000:])
    w = evt21.encode_evt21(ev, use_vectors=use_vectors, time_high_every_us=1000)
    ref = ER.decode(w)
    assert _same(ref, ev) and (len(w) < len(ev)) == use_vectors
    with evt21.DeviceEvt21Decoder(eng, max_words=len(w) + 8, max_events=len(ev)) as dec:
        assert _same(dec.decode(w), ref)
        dec.reset()
        sm = ER.Evt21StateMachine()
        for a in range(0, len(w), 1111):
            assert _same(dec.decode(w[a:a + 1111]), sm.feed(w[a:a + 1111]))


def test_wait_for_time_base(eng, emit):
    """3000 vector words and no time word: nothing with the option, everything at high field 0 without; counted per EVENT"""
    rng = np.random.default_rng(3)
    w = random_words(3000, 13)
    w = (w & np.uint64((1 << 60) - 1)) | (rng.integers(0, 2, 3000).astype(np.uint64) << np.uint64(60))
    assert (_kinds(w) <= 1).all() and _popcounts(w).sum() > 40_000
    ref = ER.decode(w)
    assert len(ref) == _popcounts(w).sum() and int(ref["t"].max()) < 64 and len(ER.decode(w, wait_for_time_base=True)) == 0
    with evt21.DeviceEvt21Decoder(eng, max_words=4096, max_events=len(ref), wait_for_time_base=True) as dec:
        assert dec.decode_device(w)[1] == 0
        follow = _u8([vec(1, 1, 0, 0, 0b111), th(9), vec(1, 2, 32, 1, 0b11)])  # still waiting in the next chunk, until its TIME_HIGH
        assert _tuples(dec.decode(follow)) == [(32, 1, 1, 9 * 64 + 2), (33, 1, 1, 9 * 64 + 2)]
        assert _tuples(dec.decode(_u8([vec(0, 3, 0, 2, 1)]))) == [(0, 2, 0, 9 * 64 + 3)]
    with evt21.DeviceEvt21Decoder(eng, max_words=4096, max_events=len(ref)) as dec:
        assert _same(dec.decode(w), ref)
    half = np.concatenate((w[:1500], _u8([th(5)]), w[1500:]))  # the time base arrives in the middle of a block
    with evt21.DeviceEvt21Decoder(eng, max_words=4096, max_events=len(ref), wait_for_time_base=True) as dec:
        assert _same(dec.decode(half), ER.decode(half, wait_for_time_base=True))


def test_cap_inside_a_word(eng, emit):
    masks = [0x3FF, 0xFFFFF, 0xF, 0xFFFFF000, 0x3FF00000]  # 10, 20 | 4, 20, 10 events
    w = _u8([th(5)] + [vec(i & 1, i, 32 * i, i, m) for i, m in enumerate(masks)])
    cum = np.cumsum(_popcounts(w))
    K = 40
    assert cum.tolist() == [0, 10, 30, 34, 54, 64] and cum[3] < K < cum[4] and cum[2] <= K and cum[5] - cum[2] <= K
    ref = ER.decode(w)
    with evt21.DeviceEvt21Decoder(eng, max_words=len(w), max_events=K) as dec:
        assert _tuples(dec.decode(_u8([th(3), vec(1, 1, 0, 0, 1)]))) == [(0, 0, 1, 193)]  # a state to keep
        with pytest.raises(N.XMapsTooMany, match="decodes to 64 events"):
            dec.decode_device(w)
        sm = ER.Evt21StateMachine()
        sm.feed(_u8([th(3)]))
        for piece in (w[1:3], w[3:]):  # (without the chunk's own TIME_HIGH: the state the refused call left is the one from before)
            assert _same(dec.decode(piece), sm.feed(piece))
        dec.reset()
        assert _same(_cat(dec.decode(w[:3]), dec.decode(w[3:])), ref)


def test_limits_and_the_wrong_format_are_reported(eng):
    import ctypes as C
    w = _u8([th(1), vec(1, 1, 0, 0, 1)])
    with evt21.DeviceEvt21Decoder(eng, max_words=1) as dec:
        with pytest.raises(N.XMapsTooMany, match="max_words"):
            dec.decode_device(w)
    with pytest.raises(Exception, match="2\\^27"):
        evt21.DeviceEvt21Decoder(eng, max_words=1 << 27)
    n = C.c_size_t(0)
    with evt3.DeviceEvt3Decoder(eng, max_words=64) as d3, evt21.DeviceEvt21Decoder(eng, max_words=64) as d21, \
            dat.DeviceDatDecoder(eng, max_words=64) as dd:
        lib = d3._lib
        for fn, d, name in ((lib.xm_evt21_decode, d3, "EVT 3.0"), (lib.xm_evt3_decode, d21, "EVT 2.1"), (lib.xm_dat_decode, d21, "EVT 2.1"),
                            (lib.xm_evt21_decode, dd, "DAT"), (lib.xm_evt2_decode, dd, "DAT")):
            assert fn(d._d, C.c_void_p(w.ctypes.data), 2, None, C.byref(n)) == N.XM_ERR_INVALID and name in N.last_error()
        assert lib.xm_evt21_set_legacy_halves(d3._d, 1) == N.XM_ERR_INVALID and lib.xm_evt21_set_legacy_halves(dd._d, 1) == N.XM_ERR_INVALID


def test_legacy_halves(eng, emit):
    w = random_words(5000, 14)
    sw = evt21.swap_halves(w)
    ref = ER.decode(w)
    assert len(ref) > 8000 and not np.array_equal(sw, w)
    with evt21.DeviceEvt21Decoder(eng, max_words=len(w), max_events=len(ref), legacy_halves=True) as dec:
        assert _same(dec.decode(sw), ref)
        dec.reset()
        dec.set_legacy_halves(False)
        assert _same(dec.decode(w), ref)


def _with_neighbours(stream, seed):
    """every third event gets companions at the same (t, y, p) in the columns to its right, inside its block of 32 columns: what an
    EVT 2.1 camera sends as ONE word"""
    rng = np.random.default_rng(seed)
    reps = np.where((np.arange(len(stream)) % 3 == 0) & (stream["x"] % 32 < 28), rng.integers(2, 5, len(stream)), 1)
    out = np.zeros(int(reps.sum()), S.EVENT_CD_DTYPE)
    idx = np.repeat(np.arange(len(stream)), reps)
    for k in ("x", "y", "p", "t"):
        out[k] = stream[k][idx]
    out["x"] = stream["x"][idx].astype(np.int64) + np.arange(len(idx)) - np.repeat(np.cumsum(reps) - reps, reps)
    return out


def _frames_of(make_push, packets, tb, fps=60):
    from x_maps_amd.ingest import DeviceIngest
    got = []
    with XMapsEngine(tb) as e, DeviceIngest(e, fps, max_packet_events=16384, capacity_events=1 << 17, result_ring=64) as ing:
        push, closer = make_push(e, ing)
        try:
            for pk in packets:
                push(pk)
                got += ing.poll()
            ing.flush()
            got += ing.poll()
        finally:
            closer()
    return got


def test_into_the_ingest():
    """the same stream as EVT 2.1 words in period chunks (vectors on), as DAT records and as EventCD packets: identical frames"""
    tb = S.make_tables(S.C_TINY)
    stream = _with_neighbours(IH._tiny_stream(8, seed=5), 1)
    assert stream["x"].max() < S.C_TINY.cam_w and (np.diff(stream["t"]) >= 0).all()
    packets = [pk for pk in IH._packets(stream, int(1e6 / 60)) if len(pk)]
    words = [evt21.encode_evt21(pk, time_high_every_us=16) for pk in packets]
    assert sum((_popcounts(w) > 1).sum() for w in words) > 1000 and sum(int(_popcounts(w).sum()) for w in words) == len(stream)

    def as_evt21(e, ing):
        dec = evt21.DeviceEvt21Decoder(e, max_words=16384)
        state = {"i": 0}

        def push(pk):
            i = state["i"]
            state["i"] += 1
            w = evt21.encode_evt21(pk, time_high_every_us=16)
            if i % 2 == 0:
                assert dec.push(ing, w) == len(pk)
            else:
                assert dec.push(ing, w, count=False) is None
        return push, dec.close

    def as_dat(e, ing):
        dec = dat.DeviceDatDecoder(e, max_words=16384)
        state = {"i": 0}

        def push(pk):
            i = state["i"]
            state["i"] += 1
            r = dat.encode_dat(pk)
            if i % 2 == 0:
                assert dec.push(ing, r) == len(pk)
            else:
                assert dec.push(ing, r, count=False) is None
        return push, dec.close

    def as_records(e, ing):
        return ing.push, lambda: None

    want = _frames_of(as_records, packets, tb)
    assert len(want) >= 5 and not any(f.lost or f.overflow for f in want)
    for make in (as_evt21, as_dat):
        got = _frames_of(make, packets, tb)
        assert len(got) == len(want) and not any(f.lost or f.overflow for f in got), make.__name__
        for a, b in zip(got, want):
            assert (a.n_events, a.t_first, a.t_last, a.n_inliers) == (b.n_events, b.t_first, b.t_last, b.n_inliers), make.__name__
            assert np.array_equal(a.depth, b.depth) and np.array_equal(a.bgr, b.bgr), make.__name__


@pytest.mark.parametrize("device_ingest", [True, False])
def test_processor_methods(device_ingest):
    """process_evt21_words == process_dat_records == process_events on the same packets, on the device ingest and on the host chain"""
    from x_maps_amd.depth_reprojection_processor import DepthReprojectionProcessor, RuntimeParams
    cfg = S.C_TINY
    tb = S.make_tables(cfg)
    stream = _with_neighbours(IH._tiny_stream(10, seed=9), 2)
    packets = [pk for pk in IH._packets(stream, int(1e6 / 60)) if len(pk)]
    assert sum((_popcounts(evt21.encode_evt21(pk)) > 1).sum() for pk in packets) > 1000
    shown = {}
    for mode in ("evt21", "evt21_legacy", "dat", "records"):
        frames = []

        class Window:
            def should_close(self):
                return False

            def show_async(self, img, acc=frames):
                acc.append(np.array(img))

        params = RuntimeParams(camera_width=cfg.cam_w, camera_height=cfg.cam_h, projector_width=cfg.proj_w,
                               projector_height=cfg.proj_h, projector_fps=60, z_near=0.1, z_far=1.2, calib=None,
                               projector_time_map=None, no_frame_dropping=True, camera_perspective=False, tables=tb,
                               device_ingest=device_ingest, raw_legacy_halves=mode == "evt21_legacy")
        with DepthReprojectionProcessor(params, window=Window()) as proc:
            for pk in packets:
                if mode == "evt21":
                    proc.process_evt21_words(evt21.encode_evt21(pk))
                elif mode == "evt21_legacy":
                    proc.process_evt21_words(evt21.swap_halves(evt21.encode_evt21(pk)))
                elif mode == "dat":
                    proc.process_dat_records(dat.encode_dat(pk))
                else:
                    proc.process_events(pk)
            proc.flush()
        shown[mode] = frames
    assert len(shown["records"]) >= 4
    for mode in ("evt21", "evt21_legacy", "dat"):
        assert len(shown[mode]) == len(shown["records"]), mode
        assert all(np.array_equal(a, b) for a, b in zip(shown[mode], shown["records"])), mode


def test_the_tool_on_an_evt21_file_and_a_dat_file(tmp_path, golden_dir):
    """tools/run_esl_on_arrival.py picks the decoder from the header: an EVT 2.1 file (stored legacy halves first) and a DAT file
    of the same events give the frames and the surfaces the EVT 3.0 file gives"""
    from test_gpu_on_arrival import _tool, _write_live_yaml
    from x_maps_amd import calibration as C
    from x_maps_amd import rig
    tool = _tool()
    g = np.load(os.path.join(golden_dir, "g6_esl_calib.npz"))
    live_yaml = tmp_path / "ESL_calib_hhi.yaml"
    _write_live_yaml(live_yaml, g, rig.NEBRA_CAMERA_D)
    cp = C.CamProjCalibrationParams.from_yaml(str(live_yaml), 640, 480, 1080, 1920)
    tables = C.build_tables(cp)
    stream, _ = rig.render_stream(cp, tables, n_frames=5, row_stride=39, seed=11)  # (few enough events for ONE packet per file)
    lead = np.zeros(2, S.EVENT_CD_DTYPE)  # (the trigger finder's first pause: see tests/test_gpu_on_arrival.py)
    lead["t"] = stream["t"][0] - np.array([1600, 1500])
    lead["x"], lead["y"], lead["p"] = [100, 101], [100, 100], 1
    both = _cat(lead, stream)
    files = {"EVT 3.0": tmp_path / "a.raw", "EVT 2.1": tmp_path / "b.raw", "DAT": tmp_path / "c.dat"}
    evt3.write_raw(str(files["EVT 3.0"]), both)
    evt21.write_raw(str(files["EVT 2.1"]), both, legacy_halves=True)
    dat.write_raw(str(files["DAT"]), both)
    assert evt21.raw_legacy_halves(str(files["EVT 2.1"]))
    out = {}
    for name, path in files.items():
        # (one chunk per file: the three encodings have different words per event, so equal chunk sizes would cut different packets)
        rep, shown, kept = tool.replay_raw(str(path), str(live_yaml), 1080, 1920, 60, 0.1, 1.2, chunk_words=1 << 20, keep_frames=8,
                                           tables=tables, scans_dir=str(tmp_path / name.replace(" ", "_")))
        assert rep["format"] == name and rep["chunks"] == 1, rep
        out[name] = (rep, shown, kept)
    want_rep, want_shown, want_kept = out["EVT 3.0"]
    # (one packet per file is one buffer of the trigger finder: it shows fewer frames than were rendered; one is enough to compare)
    assert want_rep["frames_shown"] >= 1 and len(want_kept) == want_rep["frames_shown"] and want_rep["device"]["events_dropped"] == 0
    assert want_rep["device"]["events_appended"] > 50_000 and all((f != 255).any() for f in want_kept)
    for name in ("EVT 2.1", "DAT"):
        rep, shown, kept = out[name]
        assert shown == want_shown and len(kept) == len(want_kept) and all(np.array_equal(a, b) for a, b in zip(kept, want_kept)), name
        assert rep["device"]["events_appended"] == want_rep["device"]["events_appended"], name
        for i in range(rep["frames_shown"]):
            a = np.load(tmp_path / name.replace(" ", "_") / "scans_np" / tool.scan_name(i))
            b = np.load(tmp_path / "EVT_3.0" / "scans_np" / tool.scan_name(i))
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (name, i)
