"""-m gpu: the device ingest (x_maps_amd/csrc/xmaps_ingest.hpp: k_ing_count, k_ing_count_act, k_ing_append, k_ing_segment and the
activity filter inside them) past the first trip of its per-packet loops, against the CPU chain (oracle/ingest_oracle.py) on the
very same packets -- integer bookkeeping throughout, so every comparison is equality:
  a. packets of more than 256 blocks: the second trip of both passes of ing_scan_blocks
  b. runs of blocks that keep nothing: a predecessor beyond the block's own wave of 64, beyond the group before, in the previous
     trip, in the stream's tail, nowhere
  c. the first plausible pair of pauses behind 256 and 512 others, and none among 700
  d. a pause ring that wraps twice
  e. a frame longer than the mirrored half of the event ring
  f. the activity filter's flags for packets of hundreds of blocks: computed in k_ing_count, after a first pass of their own or
     one fused into the packet before's launch, and by the ticket chain of a packet judged sequentially
  g. a packet of ING_MAX_BLOCKS * ING_EPB events, and one event more
tests/ingest_edge_cases.py builds the packets; tests/test_ingest_edge_streams_cpu.py pins what they must reach."""
import numpy as np
import pytest

import ingest_oracle as IO
from x_maps_amd import XMapsEngine
from x_maps_amd import synthetic as S
from x_maps_amd.activity_filter import ActivityNoiseFilterAlgorithm
from x_maps_amd.ingest import DeviceIngest

import ingest_edge_cases as EC
from ingest_helpers import _check_frames, _cpu_chain

pytestmark = pytest.mark.gpu
CFG = S.C_TINY


@pytest.fixture(scope="module")
def tb():
    return S.make_tables(CFG)


@pytest.fixture(scope="module")
def eng(tb):
    with XMapsEngine(tb) as e:
        yield e


def _run(tb, packets, poll_every=1, **kw):
    """the packets through an engine and a DeviceIngest of their own -> (frames, device_stats(), packets judged sequentially)"""
    kw.setdefault("result_ring", 64)
    with XMapsEngine(tb) as eng, DeviceIngest(eng, 60, **kw) as ing:
        got = []
        for k, p in enumerate(packets):
            ing.push(p)
            if k % poll_every == poll_every - 1:
                got += ing.poll()
        ing.flush()
        got += ing.poll()
        ds = ing.device_stats()
        seq = ing.activity_sequential_packets() if kw.get("activity_filter") else 0
        hs = ing.host_stats()
    assert hs["pushes"] == len(packets)  # (no packet was split on the way in)
    return got, ds, seq


# ---- a ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("launch_thread", [True, False])
def test_packets_of_more_than_256_blocks(tb, launch_thread):
    """140 000 events per frame in packets of one period: 275 to 296 blocks, every one of which keeps events"""
    want, _, n_pos = EC.dense_chain()
    assert len(want.frames) >= 4
    got, ds, _ = _run(tb, EC.dense_packets(), capacity_events=1 << 20, max_packet_events=1 << 18, launch_thread=launch_thread)
    _check_frames(tb, got, want.frames)
    assert ds["events_appended"] == n_pos and ds["events_dropped"] == 0 and ds["frames_cut"] == len(want.frames), ds


# ---- b ---------------------------------------------------------------------------------------------------------------------------------
def test_predecessors_across_groups_and_trips(tb):
    """runs of 33 000, 70 000 and 135 000 negative events inside frames (no pause at their boundary) and in frame gaps (the pause
    the finder cuts at), at the start of the stream and at the start of a later packet: 64, 136 and 263 blocks that keep nothing"""
    pk = EC.negative_run_packets()
    want, _, n_pos = _cpu_chain(pk)
    assert len(want.frames) >= 3
    got, ds, _ = _run(tb, pk, capacity_events=1 << 21, max_packet_events=1 << 19)
    _check_frames(tb, got, want.frames)
    assert ds["events_appended"] == n_pos and ds["events_dropped"] == 0, ds


# ---- c ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_stretch", [300, 700])
def test_the_first_plausible_pair_lies_behind_hundreds_of_pauses(tb, n_stretch):
    """the pair that decides is the 300th / 700th of the buffer: found in the second / third chunk of 256"""
    pk = EC.stretch_packets(n_stretch)
    want, _, n_pos = _cpu_chain(pk)
    assert len(want.frames) == 3
    got, ds, _ = _run(tb, pk, capacity_events=1 << 14, max_packet_events=1 << 12)
    _check_frames(tb, got, want.frames)
    assert ds["events_appended"] == n_pos and ds["events_dropped"] == 0, ds


def test_no_plausible_pair_among_700_pauses_drops_the_buffer(tb):
    """700 pauses over more than a period and nothing else: three chunks without a verdict, the buffer goes, and the frames behind it
    are cut as the CPU chain cuts them (their first pause pairs with none of the stretch's, which have left with their events)"""
    pk = EC.stretch_packets(700, frame_behind=False)
    want, live, n_pos = _cpu_chain(pk)
    assert live[0] == 0 and len(want.frames) >= 3
    with XMapsEngine(tb) as eng, DeviceIngest(eng, 60, capacity_events=1 << 14, max_packet_events=1 << 13, result_ring=64) as ing:
        ing.push(pk[0])
        ing.flush()
        first = ing.device_stats()
        assert ing.poll() == [] and first["events_live"] == 0 and first["events_appended"] == 701 and first["events_dropped"] == 0, first
        for p in pk[1:]:
            ing.push(p)
        ing.flush()
        got = ing.poll()
        ds = ing.device_stats()
    _check_frames(tb, got, want.frames)
    assert ds["events_appended"] == n_pos and ds["events_dropped"] == 0, ds


# ---- d ---------------------------------------------------------------------------------------------------------------------------------
def test_the_pause_ring_wraps_twice(tb):
    """three stretches of 6000 pauses through a pause ring of 8192 entries, frames in front of, between and behind them"""
    pk = EC.pause_wrap_packets()
    want, _, n_pos = _cpu_chain(pk)
    assert len(want.frames) >= 4 + 3
    got, ds, _ = _run(tb, pk, **EC.PAUSE_CAP)
    _check_frames(tb, got, want.frames)
    assert ds["events_appended"] == n_pos and ds["events_dropped"] == 0, ds


# ---- e ---------------------------------------------------------------------------------------------------------------------------------
def test_a_frame_longer_than_the_mirror_is_counted_and_the_stream_goes_on(tb):
    """a frame of 9001 events in a ring whose mirrored half holds 8192: not handed out, counted into `overflow` (its length,
    next - prev - 4), and the frames around it are the CPU chain's"""
    pk = EC.long_frame_packets()
    cpu, _, n_pos = _cpu_chain(pk)
    mirror = EC.MIRROR_CAP["capacity_events"] // 2
    long_at = [k for k, f in enumerate(cpu.frames) if len(f) > mirror]
    assert len(long_at) == 1 and 0 < long_at[0] < len(cpu.frames) - 2
    want = [f for f in cpu.frames if len(f) <= mirror]
    n_long = len(cpu.frames[long_at[0]])
    got, ds, _ = _run(tb, pk, **EC.MIRROR_CAP)
    _check_frames(tb, got, want, overflow=[0] * long_at[0] + [n_long] * (len(want) - long_at[0]))
    assert not any(f.lost for f in got)
    assert ds["events_dropped"] == n_long and ds["events_appended"] == n_pos and ds["frames_cut"] == len(want), ds


# ---- f ---------------------------------------------------------------------------------------------------------------------------------
def test_activity_flags_of_a_packet_of_140_000_events_and_of_an_unsorted_one(eng):
    """the filter alone, flag by flag against the C form of the sequential definition: 140 000 events over 8 buckets (the parallel
    path), then 20 000 whose stamps run backwards (one block judges them in groups of 256); about half of the flags are set"""
    T = 1000
    ora = IO.ActivityFilterC(CFG.cam_w, CFG.cam_h, T)
    with ActivityNoiseFilterAlgorithm(eng, T, max_packet_events=1 << 18) as act:
        ev = EC.lattice_packet(140_000, 1, 8 * (T + 1) - 1)
        want = ora.process(ev)
        got = act.process_events(ev)
        assert 0.3 < len(want) / len(ev) < 0.7 and len(got) == len(want) and np.array_equal(got, want)
        assert act.sequential_packets() == 0
        ev = EC.lattice_packet(20_000, 2, 4 * T, support=0.05, sort=False, start=1_010_000)
        want = ora.process(ev)
        got = act.process_events(ev)
        assert 0.3 < len(want) / len(ev) < 0.7 and len(got) == len(want) and np.array_equal(got, want)
        assert act.sequential_packets() == 1


@pytest.mark.parametrize("thresh", [0, 3000])
def test_activity_filter_inside_the_ingest_on_packets_of_more_than_256_blocks(tb, thresh):
    """the dense stream with the filter on, pushed in pairs with nothing polled in between (the second packet's first pass may ride
    on the first one's counting launch): default threshold -- one bucket per packet (two in the first) --, and 3000 us -- six"""
    T = thresh or int(1e6 / 60)
    want, _, n_kept = EC.activity_chain(EC.dense_packets(), T)
    assert len(want.frames) >= 4
    got, ds, seq = _run(tb, EC.dense_packets(), poll_every=2, activity_filter=True, activity_thresh_us=thresh,
                        capacity_events=1 << 20, max_packet_events=1 << 18)
    assert seq == 0
    _check_frames(tb, got, want.frames)
    assert ds["events_appended"] == n_kept and ds["events_dropped"] == 0, ds


def test_a_packet_of_300_blocks_judged_sequentially(tb):
    """stamps that step back by more than a bucket in the middle of a packet of 153 590 events: its 300 blocks take their turns by
    ticket; the same events are kept and the same frames cut as by the CPU chain"""
    pk = EC.backwards_packets()
    want, _, n_kept = EC.activity_chain(pk)
    assert len(want.frames) >= 4
    got, ds, seq = _run(tb, pk, poll_every=2, activity_filter=True, capacity_events=1 << 20, max_packet_events=1 << 18)
    assert seq >= 1
    _check_frames(tb, got, want.frames)
    assert ds["events_appended"] == n_kept and ds["events_dropped"] == 0, ds


# ---- g ---------------------------------------------------------------------------------------------------------------------------------
def test_one_event_more_than_the_limit_is_refused(eng):
    from x_maps_amd._native import XMapsNativeError
    for cap in (1 << 22, 1 << 23):  # (the second: at least twice the packet, so nothing but the limit itself can object)
        with pytest.raises((XMapsNativeError, ValueError)):
            DeviceIngest(eng, 60, max_packet_events=EC.LIMIT + 1, capacity_events=cap)


def test_a_packet_of_exactly_the_limit(tb):
    """2 097 152 events, 9478 of them positive, in 12 pieces with ~370 blocks that keep nothing between them; blocks 0 and 4095 keep
    events; three frame gaps lie across such runs.  Then the rest of the stream in packets of 900."""
    pk = EC.limit_packets()
    want, _, n_pos = _cpu_chain(pk)
    assert len(pk[0]) == EC.LIMIT and len(want.frames) >= 3
    got, ds, _ = _run(tb, pk, max_packet_events=EC.LIMIT, capacity_events=1 << 22)
    _check_frames(tb, got, want.frames)
    assert ds["events_appended"] == n_pos and ds["events_dropped"] == 0 and ds["frames_cut"] == len(want.frames), ds
