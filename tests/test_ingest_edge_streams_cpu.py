"""The streams of tests/test_gpu_ingest_edges.py, checked with the CPU oracle alone: every case must reach the piece of the device
ingest's bookkeeping it was built for (x_maps_amd/csrc/xmaps_ingest.hpp) -- a second trip of ing_scan_blocks' loops over 256 block
records, a predecessor beyond a block's own wave of 64 blocks, a second and third chunk of ing_find_trigger's search over 256 pairs
of pauses, a wrapped pause ring, a frame longer than the ring's mirrored half -- and the reference's trigger finder must still cut
frames from it.  A change to a builder that moves a case back inside a first trip fails here, without a GPU."""
import numpy as np

import ingest_oracle as IO
from x_maps_amd import synthetic as S

import ingest_edge_cases as EC
from ingest_helpers import (_block_kept, _cpu_chain, _dense_stream, _empty_runs, _first_plausible_pair, _pause_indices, _period_packets,
                            _sparse_stretch, _with_negative_run)

PERIOD = 1e6 / 60


def _in_flight(packets, live):
    """the most events the ring must hold at once: what the finder kept behind a packet + the next packet's positive events"""
    return max(before + int((p["p"] == 1).sum()) for before, p in zip([0] + live[:-1], packets))


def _sorted(packets):
    return all(np.all(np.diff(p["t"]) >= 0) for p in packets if len(p))


def test_the_builders_do_what_they_say():
    s = _dense_stream(3, 20_000, seed=1)
    assert len(s) == 3 * (20_000 + 520) and np.all(np.diff(s["t"]) >= 0)
    assert len(np.unique(s["t"])) < len(s)  # equal stamps are allowed (and, at this rate, certain)
    pos = IO.polarity_filter(s)
    assert 0.88 < len(pos) / len(s) < 0.92
    assert list(np.diff(pos["t"])[_pause_indices(pos)] > 3_000) == [True, True]  # the two frame gaps and no pause inside a frame
    assert s["x"].max() < S.C_TINY.cam_w and s["y"].max() < S.C_TINY.cam_h
    pk = _period_packets(s)
    assert sum(len(p) for p in pk) == len(s) and [int(p["t"][-1]) // 100 * 100 for p in pk[:-1]] == [2_017_500, 2_034_100]
    run = _with_negative_run(s, 1000, 77)
    assert len(run) == len(s) + 77 and np.all(run["p"][1000:1077] == 0) and np.all(run["t"][1000:1078] == s["t"][1000])
    assert np.array_equal(IO.polarity_filter(run), pos) and np.all(np.diff(run["t"]) >= 0)
    st = _sparse_stretch(50, 123)
    assert np.all(st["p"] == 1) and np.all(np.diff(st["t"]) == 45) and st["t"][0] == 123 and _first_plausible_pair(st) == (-1, 49)


def test_a_dense_stream_in_period_packets_takes_the_block_scan_into_its_second_trip():
    pk = EC.dense_packets()
    tf, live, n_pos = EC.dense_chain()
    assert _sorted(pk) and max(len(p) for p in pk) <= 1 << 18
    assert [EC.n_blocks(p) for p in pk] == [296, 275, 275, 275, 275, 275, 254]  # the scan's trips are 256 blocks
    assert all(_empty_runs(p) == [] for p in pk)  # every block keeps events: the in-wave ballot finds every predecessor
    assert [len(f) for f in tf.frames] == [126_456, 126_491, 126_409, 126_532]  # >= 4
    assert n_pos == 885_381
    # capacity 1 << 20, max_packet 1 << 18 (one packet ahead: room 1 << 19)
    assert max(live) + (1 << 19) <= 1 << 20 and _in_flight(pk, live) <= 1 << 20 and max(len(f) for f in tf.frames) <= 1 << 19


def test_negative_runs_put_predecessors_beyond_the_wave_the_group_and_the_trip():
    pk = EC.negative_run_packets()
    tf, live, n_pos = _cpu_chain(pk)
    want, _, want_pos = EC.dense_chain()
    assert _sorted(pk) and max(len(p) for p in pk) <= 1 << 19
    # negative events never reach the finder: the same frames as without the runs (>= 3)
    assert n_pos == want_pos and len(tf.frames) == len(want.frames) == 4 and all(np.array_equal(a, b) for a, b in zip(tf.frames, want.frames))
    assert [EC.n_blocks(p) for p in pk[:4]] == [425, 404, 675, 676]
    # (first block behind the run, blocks the run empties)
    runs = [_empty_runs(p) for p in pk[:4]]
    assert runs == [[(64, 64), (165, 64)], [(64, 64), (382, 64)], [(300, 263), (653, 136)], [(286, 136), (653, 262)]]
    for packet_runs in runs:
        for after, length in packet_runs:
            first = after - length
            assert length >= 64 and (first == 0 or first % 64 != 0)
    kept = [_block_kept(p) for p in pk[:4]]
    pred = lambda k, b: max(j for j in range(b) if k[j])  # noqa: E731
    # 33 000: the predecessor is in the group before; 70 000: two groups back or more; 135 000: more than 256 blocks back, in the
    # scan's previous trip
    assert (pred(kept[0], 165) >> 6, 165 >> 6) == (1, 2) and (pred(kept[1], 382) >> 6, 382 >> 6) == (4, 5)
    assert (653 >> 6) - (pred(kept[2], 653) >> 6) >= 2 and (286 >> 6) - (pred(kept[3], 286) >> 6) >= 2
    assert 300 - pred(kept[2], 300) > 256 and 300 // 256 != pred(kept[2], 300) // 256
    assert 653 - pred(kept[3], 653) > 256 and 653 // 256 != pred(kept[3], 653) // 256
    # the leading runs: no kept block in front of block 64 (packet 0: nothing in front of the packet either)
    assert not kept[0][:64].any() and not kept[1][:64].any()

    def boundary_gap(p, after):  # between the last positive event in front of the run and the first one behind it
        pos = np.nonzero(p["p"] == 1)[0]
        k = int(np.searchsorted(pos, (after - 1) * EC.EPB))  # (block after - 1 is empty: the first positive behind it)
        return int(p["t"][pos[k]] - p["t"][pos[k - 1]])
    # inside a frame: no pause at the boundary; in a frame gap: the pause the finder cuts at
    assert boundary_gap(pk[0], 165) < 40 and boundary_gap(pk[2], 300) < 40 and boundary_gap(pk[3], 286) < 40
    assert all(boundary_gap(pk[i], 382 if i == 1 else 653) > 3_000 for i in (1, 2, 3))
    assert int(pk[1]["t"][64 * EC.EPB + 300] - pk[0]["t"][-1]) < 40  # the stream's tail against packet 1's first kept event: no pause
    assert max(live) + (1 << 20) <= 1 << 21  # capacity 1 << 21, max_packet 1 << 19, one packet ahead


def test_sparse_stretches_push_the_first_plausible_pair_past_one_and_two_chunks():
    for n, events in ((300, 3549), (700, 3949)):
        pk = EC.stretch_packets(n)
        tf, live, _ = _cpu_chain(pk)
        assert _sorted(pk) and max(len(p) for p in pk) == len(pk[0]) == events <= 1 << 12
        # pause n - 1 is the stretch's last event, pause n the first frame's: the search's chunks are 256 pairs
        assert _first_plausible_pair(pk[0]) == (n - 1, n + 1) and (n - 1) // 256 == (1 if n == 300 else 2)
        assert [len(f) for f in tf.frames] == [3116, 3116, 3116]
        assert max(live) + (1 << 13) <= 1 << 14  # capacity 1 << 14, max_packet 1 << 12, one packet ahead
    pk = EC.stretch_packets(700, frame_behind=False)
    tf, live, _ = _cpu_chain(pk)
    assert len(pk[0]) == 701 and pk[0]["t"][-1] - pk[0]["t"][0] > PERIOD and _first_plausible_pair(pk[0]) == (-1, 700)  # 699 pairs: 3 chunks
    assert live[0] == 0 and [len(f) for f in tf.frames] == [3116] * 4 and max(len(p) for p in pk) == 6364
    assert max(live) + (1 << 13) <= 1 << 14  # capacity 1 << 14, max_packet 1 << 13, none ahead


def test_the_pause_ring_case_wraps_twice_and_leaves_frames_behind_the_second_wrap():
    pk = EC.pause_wrap_packets()
    tf, live, _ = _cpu_chain(pk)
    cap, max_packet = EC.PAUSE_CAP["capacity_events"], EC.PAUSE_CAP["max_packet_events"]
    assert _sorted(pk) and max(len(p) for p in pk) <= max_packet
    pos = IO.polarity_filter(np.concatenate(pk))
    pauses = _pause_indices(pos)
    assert len(pauses) == 18_022 > 2 * (2 * cap) + 1000
    before = [int(np.searchsorted(pos["t"][pauses], f["t"][0])) for f in tf.frames]  # pauses appended when the frame's first event is
    assert len(tf.frames) == 14 and sum(b >= 2 * (2 * cap) for b in before) == 5  # >= 4 behind the second wrap
    assert sum(b < 2 * cap for b in before) == 6 and sum(2 * cap <= b < 4 * cap for b in before) == 3
    # the room rule (no packets ahead at this size: room = one packet) never fires, and the ring holds what is in flight
    assert max(live) == 2003 <= cap - max_packet and _in_flight(pk, live) == 4003 <= cap


def test_the_long_frame_is_longer_than_the_mirror_and_the_room_rule_stays_quiet():
    pk = EC.long_frame_packets()
    tf, live, _ = _cpu_chain(pk)
    cap, max_packet = EC.MIRROR_CAP["capacity_events"], EC.MIRROR_CAP["max_packet_events"]
    assert _sorted(pk) and max(len(p) for p in pk) <= max_packet
    assert [len(f) for f in tf.frames] == [1666, 2523, 9001, 2535, 2487, 2491, 2480, 2476, 2478]
    assert sum(len(f) > cap // 2 for f in tf.frames) == 1
    # k_ing_segment drops the live part when write_abs - start_abs + room > cap, room = 3 packets (two ahead): the finder's buffer
    # behind any packet stays below that, the long frame's packets included
    assert max(live) == 7933 <= cap - 3 * max_packet and _in_flight(pk, live) == 9208 <= cap


def test_the_activity_cases_take_the_paths_they_are_meant_for():
    T = int(PERIOD)
    # default threshold: one bucket of T + 1 us per packet (the first one, a period and the lead long: two)
    assert [int(p["t"][-1] - p["t"][0]) // (T + 1) for p in EC.dense_packets()] == [1, 0, 0, 0, 0, 0, 0]
    assert max(-(-(int(p["t"][-1] - p["t"][0]) + 1) // 3001) for p in EC.dense_packets()) == 6  # 3000 us: several buckets, at most 8
    tf, _, n = EC.activity_chain(EC.dense_packets())
    assert [len(f) for f in tf.frames] == [126_456, 126_491, 126_409, 126_532] and n == 885_226
    tf, _, n = EC.activity_chain(EC.dense_packets(), 3000)
    assert [len(f) for f in tf.frames] == [126_295, 126_321, 126_266, 126_360] and n == 884_233
    pk = EC.backwards_packets()
    half = len(pk[0]) // 2
    assert EC.n_blocks(pk[0]) == 300 and pk[0]["t"][half - 1] - pk[0]["t"][half] > T + 1
    tf, live, n = EC.activity_chain(pk)
    assert [len(f) for f in tf.frames] == [126_447, 126_491, 126_409, 126_532] and n == 885_164
    assert all(np.all(np.diff(f["t"]) >= 0) for f in tf.frames)  # (the step lies in a packet the finder drops)
    assert max(live) + (1 << 19) <= 1 << 20
    # the filter alone: about half of the flags are set, on 8 buckets / on a packet that is not sorted
    ev = EC.lattice_packet(140_000, 1, 8 * 1001 - 1)
    assert np.all(np.diff(ev["t"]) >= 0) and (ev["t"][-1] - ev["t"][0]) // 1001 == 7
    assert len(IO.ActivityFilterC(S.C_TINY.cam_w, S.C_TINY.cam_h, 1000).process(ev)) == 66_661
    ev = EC.lattice_packet(20_000, 2, 4000, support=0.05, sort=False)
    assert np.any(np.diff(ev["t"]) < -1001)
    assert len(IO.ActivityFilterC(S.C_TINY.cam_w, S.C_TINY.cam_h, 1000).process(ev)) == 10_992


def test_the_packet_at_the_limit_keeps_events_in_its_first_and_last_block_and_hundreds_of_empty_blocks_between():
    pk = EC.limit_packets()
    big = pk[0]
    assert len(big) == EC.LIMIT == 2_097_152 and EC.n_blocks(big) == 4096 and np.all(np.diff(big["t"]) >= 0)
    kept = _block_kept(big)
    assert kept[0] > 0 and kept[4095] > 0 and int(kept.sum()) == 9478
    runs = _empty_runs(big)
    assert len(runs) == 11 and all(369 <= length <= 372 for _, length in runs) and runs[-1][0] == 4095
    tf, live, n_pos = _cpu_chain(pk)
    assert np.array_equal(IO.polarity_filter(np.concatenate(pk)), _dense_stream(6, 2600, seed=130, neg=0)) and n_pos == 18_720
    assert [len(f) for f in tf.frames] == [3116] * 4
    # a frame gap lies across a run: the boundary pause of the block behind it is decided against a block ~370 blocks back
    pos = np.nonzero(big["p"] == 1)[0]
    gaps = np.nonzero(np.diff(big["t"][pos]) >= 40)[0]
    assert len(gaps) == 3 and all(pos[g + 1] - pos[g] > 256 * EC.EPB for g in gaps)
