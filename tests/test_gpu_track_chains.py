"""Peak tracks on the device (beamformer_hip_track_peaks_last_frames; csrc/frame_tracks.hip: link, jump, keep, scan, finish).  Frames are
PLANTED (tests/planted.py) by one burst push (tests/ring_frames.py planted_burst): a frame then is the array, and the numpy reference
(tests/track_chains_ref.py) runs on the downloaded frames; the plans are tests/track_plans.py's, and tests/test_track_chains_host.py checks
without a device that they hold what they claim.  On complex frames the reference chains the records beamformer_hip_find_peaks_last_frames
returns (tests/test_gpu_tracks.py says why: a magnitude may differ from numpy's by 1 ulp).

Everything compared is an integer or a bit pattern and is asked exactly: there is no tolerance in this file."""
import ctypes as C

import numpy as np
import pytest

from ogl_beamforming_amd import lib as bf
from ogl_beamforming_amd import params as P
from tests import localisation_ref, planted, tracks_ref
from tests import ring_frames
from tests import track_plans
from tests import track_chains_ref as ref
from tests import variants_cases as vc
from tests.frame_info import newest_info
from tests.ring_frames import (metrics_block as block, planted_burst as burst, finer, fraction_of_max, fresh_maps, map_view, placement_onto,
                               same_tracks_call as same_call, same_maps, track, variants_push)
from tests.scaffold import automatic_path  # noqa: F401

pytestmark = pytest.mark.gpu
E = P.LibError
IDENTITY, LEVEL, REACH, CAP = track_plans.IDENTITY, track_plans.LEVEL, track_plans.REACH, ring_frames.CAP
POINTS, LINKS = P.HIP_TRACK_DEPOSIT_POINTS, P.HIP_TRACK_DEPOSIT_LINKS
FIELD = (20, 1, 40)                                        # both maps over the plane plan: its spots at x = 20, 21 and 22 lie outside


@pytest.fixture(autouse=True)
def maps_reset(automatic_path, bflib):
    yield
    bflib.localisation_map_reset(None)
    bflib.track_map_reset(None)


@pytest.fixture
def plane(bflib):
    """the plane plan on the device: the 11 downloaded frames"""
    stack, _ = track_plans.plane_plan()
    frames, _ = burst(stack)
    return list(frames)


# ----------------------------------------------------------------------------- 1: the plane plan

@pytest.mark.parametrize("min_length", [1, 3, 9, 12])
def test_the_plane_plan_at_four_lengths_with_every_deposit(min_length, plane, bflib):
    K = len(plane)
    everything = ref.chain_frames(plane, LEVEL, IDENTITY, REACH, CAP, 1)
    assert sorted(everything["lengths"]) == [1, 1, 2, 3, 5, 6, 8, 9, 11] and len(everything["pairs"]) == 37
    assert ref.one_sided(everything["pair_rows"]) >= 1                # a forward choice that is not mutual
    for deposit in (0, POINTS, LINKS, POINTS | LINKS):
        density, counts, sums = fresh_maps(FIELD)
        got = track(K, LEVEL, IDENTITY, REACH, min_length, deposit=deposit)
        want = ref.chain_frames(plane, LEVEL, IDENTITY, REACH, CAP, min_length, deposit=deposit, point_map=density, counts=counts, sums=sums)
        same_call(got, want, K, LEVEL)
        point_info, link_info = same_maps(FIELD, density, counts, sums)
        rows = want["rows"]
        assert (point_info.calls, int(point_info.deposited), int(point_info.outside)) == \
            ((1, sum(r["points_deposited"] for r in rows), sum(r["points_outside"] for r in rows)) if deposit & POINTS else (0, 0, 0))
        assert (link_info.calls, int(link_info.pairs), int(link_info.deposited), int(link_info.outside)) == \
            ((1, sum(r["kept_links"] for r in rows), sum(r["links_deposited"] for r in rows), sum(r["links_outside"] for r in rows)) if deposit & LINKS else (0, 0, 0, 0))
        assert int(density.sum()) == int(point_info.deposited) and int(counts.sum()) == int(link_info.deposited)
    if min_length in (3, 9):
        track_plans.teeth(want, min_length, K)
        assert int(point_info.outside) + int(link_info.outside) >= (1 if min_length == 3 else 0)
    elif min_length == 1:
        assert len(want["tracks"]) == 9 and int(point_info.outside) == 4 and int(link_info.outside) == 2
    else:
        assert len(want["tracks"]) == 0 and len(want["points"]) == 0 and not density.any() and not counts.any()      # min_length > count: legal, keeps nothing


# ----------------------------------------------------------------------------- 2: more than 512 peaks a frame

def test_a_lattice_of_more_than_512_peaks_a_frame(bflib):
    stack, placements = track_plans.volume_plan()
    frames, _ = burst(stack)
    K, field = len(frames), (12, 16, 32)                       # both maps end at x = 12: the lattice's last columns lie outside
    density, counts, sums = fresh_maps(field)
    got = track(K, LEVEL, placements, 1.0, 3, deposit=POINTS | LINKS)
    want = ref.chain_frames(list(frames), LEVEL, placements, 1.0, CAP, 3, deposit=POINTS | LINKS, point_map=density, counts=counts, sums=sums)
    same_call(got, want, K, LEVEL)
    same_maps(field, density, counts, sums)
    # tracks cross the blocks of 256 records of every pass: a point and its successor lie in different ones
    assert all(r["peaks"] > 512 for r in want["rows"]) and len(want["tracks"]) > 256 and set(want["lengths"]) >= {1, 2, 3, 4, 5}
    firsts = np.concatenate([[0], np.cumsum([r["peaks"] for r in want["rows"]])])
    for t in want["tracks"]:
        run = want["points"][int(t["first"]):int(t["first"]) + int(t["length"])]
        index = firsts[run["frame"]] + run["rank"]
        assert (index[1:] >> 8 != index[:-1] >> 8).all()
    assert int(want["tracks"]["first"][-1]) >> 8 >= 4 and sum(r["points_outside"] for r in want["rows"]) >= 1


# ----------------------------------------------------------------------------- 3: the three equalities

def test_the_three_equalities_with_the_pair_call_and_the_accumulate_call(plane, bflib):
    K = len(plane)
    # (i) min_length <= 2 with LINKS: the track map's bytes are the pair call's
    bf.track_map_reset(FIELD)
    pair_rows, pairs = ring_frames.pair(K, LEVEL, IDENTITY, REACH, deposit=True)
    of_the_pairs = bf.track_map_copy(FIELD)
    assert int(of_the_pairs[2].pairs) == len(pairs) == 37 and int(of_the_pairs[2].outside) == 2
    for min_length in (1, 2):
        bf.track_map_reset(FIELD)
        rows, tracks, points = track(K, LEVEL, IDENTITY, REACH, min_length, deposit=LINKS)
        mine = bf.track_map_copy(FIELD)
        assert mine[0].tobytes() == of_the_pairs[0].tobytes() and mine[1].tobytes() == of_the_pairs[1].tobytes()
        assert bytes(mine[2]) == bytes(of_the_pairs[2])                # the totals too: calls, pairs, deposited, outside
    # (ii) min_length == 1 with POINTS, no cap reached, no unplaced peak: the localisation map's bytes are the accumulate call's
    bf.localisation_map_reset(FIELD)
    deposits, _ = bf.accumulate_peaks_last_frames(K, LEVEL, IDENTITY)
    of_the_peaks = bf.localisation_map_copy(FIELD)
    bf.localisation_map_reset(FIELD)
    rows, tracks, points = track(K, LEVEL, IDENTITY, REACH, 1, deposit=POINTS)
    assert all(int(r.found) <= CAP and r.unplaced == 0 for r in rows)
    mine = bf.localisation_map_copy(FIELD)
    assert mine[0].tobytes() == of_the_peaks[0].tobytes() and bytes(mine[1]) == bytes(of_the_peaks[1]) and int(mine[1].deposited) == 42
    assert [(r.points_deposited, r.points_outside) for r in rows] == [(int(m.deposited), int(m.outside)) for m in deposits]
    # (iii) the links of all tracks at min_length == 1 are exactly the pair call's records
    links = []
    for t in tracks:
        run = points[int(t["first"]):int(t["first"]) + int(t["length"])]
        links += [(int(p["frame"]), int(p["rank"]), int(q["rank"]), (q["position"] - p["position"]).tobytes()) for p, q in zip(run[:-1], run[1:])]
    assert sorted(links) == [(int(r["frame"]), int(r["a"]), int(r["b"]), r["displacement"].tobytes()) for r in pairs]
    assert [int(r.kept_links) for r in rows][:-1] == [int(r.pairs) for r in pair_rows] and rows[K - 1].kept_links == 0


# ----------------------------------------------------------------------------- 4: complex frames

def test_complex_frames_chain_as_their_find_peaks_records_say(bflib):
    acq = block("A")
    frames, ids = variants_push("A")
    assert np.iscomplexobj(frames)
    grid = map_view(finer(vc.POINTS), vc.LO, vc.HI)
    field = tuple(grid.output_points)
    A = placement_onto(grid, acq.bp.das_voxel_transform, vc.POINTS)
    thresholds = fraction_of_max(frames, 0.1)
    kept = 0
    for min_length, use_offsets in ((1, True), (2, True), (3, True), (2, False)):
        density, counts, sums = fresh_maps(field)
        got = track(3, thresholds, A, 6.0, min_length, use_offsets=use_offsets, deposit=POINTS | LINKS)
        want = ref.chain_records(ring_frames.peak_lists(3, thresholds), A, 6.0, min_length, use_offsets, deposit=POINTS | LINKS,
                                 point_map=density, counts=counts, sums=sums)
        same_call(got, want, 3, thresholds)
        same_maps(field, density, counts, sums)
        kept += len(want["tracks"])
        assert [int(r.frame_id) for r in got[0]] == ids
    assert kept >= 8 and {1, 2, 3} <= set(want["lengths"])


# ----------------------------------------------------------------------------- 5: placements and caps

def test_an_unplaced_frame_a_cap_a_box_and_no_offsets(plane, bflib):
    K = len(plane)
    # frame 5 placed at infinity: finite entries whose sum overflows (every spot has x >= 2); every track breaks there
    lost = np.stack([IDENTITY] * K)
    lost[5, 0, 0] = lost[5, 0, 3] = 1.7e308
    density, counts, sums = fresh_maps(FIELD)
    got = track(K, LEVEL, lost, REACH, 2, deposit=POINTS | LINKS)
    want = ref.chain_frames(plane, LEVEL, lost, REACH, CAP, 2, deposit=POINTS | LINKS, point_map=density, counts=counts, sums=sums)
    same_call(got, want, K, LEVEL)
    same_maps(FIELD, density, counts, sums)
    rows = want["rows"]
    assert rows[5]["unplaced"] == rows[5]["peaks"] == 6 and rows[5]["heads"] == 0 and rows[4]["kept_links"] == 0
    assert all(t["frame"] + t["length"] <= 5 or t["frame"] >= 6 for t in want["tracks"]) and sorted(want["lengths"])[-1] == 5
    # max_per_frame below found: the first three peaks of a frame in flat order
    got = track(K, LEVEL, IDENTITY, REACH, 2, cap=3)
    want = ref.chain_frames(plane, LEVEL, IDENTITY, REACH, 3, 2)
    same_call(got, want, K, LEVEL, cap=3)
    assert any(r["found"] > 3 for r in want["rows"]) and all(r["peaks"] <= 3 for r in want["rows"]) and len(want["tracks"]) >= 2
    # a box that leaves out the spots at x = 2 and from x = 20 on; without offsets
    box = ((4, 0, 0), (16, 1, 40))
    for use_offsets in (True, False):
        got = track(K, LEVEL, IDENTITY, REACH, 2, use_offsets=use_offsets, box=box)
        want = ref.chain_frames(plane, LEVEL, IDENTITY, REACH, CAP, 2, use_offsets, first=box[0], count=box[1])
        same_call(got, want, K, LEVEL, box=box)
        assert sorted(want["lengths"]) == [1, 2, 5, 6, 8, 9]
    # per-frame thresholds: frame 6 asks for more than the spots' height, and has no peak
    levels = np.full(K, LEVEL, np.float32)
    levels[6] = 2 * track_plans.HEIGHT
    got = track(K, levels, IDENTITY, REACH, 1)
    want = ref.chain_frames(plane, levels, IDENTITY, REACH, CAP, 1)
    same_call(got, want, K, levels)
    assert want["rows"][6]["peaks"] == 0 and max(want["lengths"]) == 6


# ----------------------------------------------------------------------------- 6: repeatability

def test_the_same_call_twice_and_without_records(plane, bflib):
    K = len(plane)
    first = track(K, LEVEL, IDENTITY, REACH, 3)
    again = track(K, LEVEL, IDENTITY, REACH, 3)
    assert [bytes(v) for v in first] == [bytes(v) for v in again] and len(first[1]) == 6
    # records False: no list comes back, the rows are the same; one list alone comes back as it does with the other
    rows, tracks, points, ms = bf.track_peaks_last_frames(K, LEVEL, IDENTITY, REACH, CAP, 3, records=False)
    assert bytes(rows) == bytes(first[0]) and len(tracks) == 0 and len(points) == 0 and ms > 0
    L = bflib.library()
    out_rows, out_points = (P.HipTrackedFrame * K)(), np.zeros(K * CAP, ref.POINT)
    totals, level = (C.c_uint32(0), C.c_uint32(0)), (C.c_float * 1)(LEVEL)
    assert L.beamformer_hip_track_peaks_last_frames(K, None, level, 1, IDENTITY.ctypes.data_as(C.POINTER(C.c_double)), 1, 1, REACH, CAP, 3, 0, out_rows,
                                                    None, out_points.ctypes.data_as(C.POINTER(P.HipTrackPoint)), C.byref(totals[0]),
                                                    C.byref(totals[1]), None)
    assert (totals[0].value, totals[1].value) == (len(first[1]), len(first[2])) and bytes(out_rows) == bytes(first[0])
    assert out_points[:totals[1].value].tobytes() == first[2].tobytes() and not out_points[totals[1].value:].view(np.uint8).any()
    # the newest frames of a longer ring: a call over the 4 newest frames sees only them
    got = track(4, LEVEL, IDENTITY, REACH, 2)
    want = ref.chain_frames(plane[-4:], LEVEL, IDENTITY, REACH, CAP, 2)
    same_call(got, want, 4, LEVEL)
    assert (want["tracks"]["flags"] == 3).sum() >= 2                  # cut by the call's window at both ends


# ----------------------------------------------------------------------------- 7: the queue calls behind a depositing track call

def test_both_maps_queue_behind_a_depositing_track_call(plane, bflib):
    L = bflib.library()
    K = len(plane)
    density, counts, sums = fresh_maps(FIELD)
    frame, ms = C.c_uint32(77), C.c_float(-1.0)
    # a call without deposit does not count: neither map is queued behind it
    track(K, LEVEL, IDENTITY, REACH, 3)
    assert not L.beamformer_hip_queue_localisation_map(1.0, 0, C.byref(frame), C.byref(ms)) and bf.last_error()[0] == E.InvalidAccess
    assert not L.beamformer_hip_queue_track_map(3, 1.0, 1, 0, C.byref(frame), C.byref(ms)) and bf.last_error()[0] == E.InvalidAccess
    newest = int(newest_info(L).frame_id)
    block_of_newest = bf.frame_info(newest).parameter_block
    for _ in range(2):                                                # twice: the maps add up
        track(K, LEVEL, IDENTITY, REACH, 3, deposit=POINTS | LINKS)
        want = ref.chain_frames(plane, LEVEL, IDENTITY, REACH, CAP, 3, deposit=POINTS | LINKS, point_map=density, counts=counts, sums=sums)
    point_info, link_info = same_maps(FIELD, density, counts, sums)
    rows = want["rows"]
    assert (point_info.calls, int(point_info.deposited)) == (2, 2 * sum(r["points_deposited"] for r in rows)) and int(point_info.deposited) == int(density.sum())
    assert (link_info.calls, int(link_info.pairs), int(link_info.deposited)) == (2, 2 * sum(r["kept_links"] for r in rows), int(counts.sum()))
    frame_id, _ = bf.queue_localisation_map(0.5, tag=4)
    assert frame_id == newest + 1 and bf.frame_info(frame_id).parameter_block == block_of_newest
    assert np.array_equal(bf.copy_frame(frame_id).view(np.uint32), localisation_ref.queued_frame(density, 0.5).view(np.uint32))
    for component, scale, min_pairs in ((2, 0.37, 1), (3, 1.0, 2), (4, 3.0, 1)):
        frame_id, _ = bf.queue_track_map(component, scale, min_pairs, tag=5)
        assert bf.frame_info(frame_id).parameter_block == block_of_newest
        expected = tracks_ref.queued_frame(counts, sums, component, scale, min_pairs)
        assert np.array_equal(bf.copy_frame(frame_id).view(np.uint32), expected.view(np.uint32)) and np.count_nonzero(expected) >= 4


# ----------------------------------------------------------------------------- 8: refusals

def test_refusals_on_the_device_change_nothing(plane, bflib):
    L = bflib.library()
    K = len(plane)
    fresh_maps(FIELD)
    track(K, LEVEL, IDENTITY, REACH, 3, deposit=POINTS | LINKS)

    def state():
        tracks, density = bf.track_map_copy(FIELD), bf.localisation_map_copy(FIELD)
        return [bytes(v) if not isinstance(v, np.ndarray) else v.tobytes() for v in tracks + density] + [bytes(newest_info(L))]

    before = state()
    rows, tracks, points = (P.HipTrackedFrame * 16)(), (P.HipPeakTrack * 64)(), (P.HipTrackPoint * 64)()
    for out in (rows, tracks, points):
        C.memset(out, 0xA5, C.sizeof(out))
    untouched = bytes(rows), bytes(tracks), bytes(points)
    totals, ms, level = (C.c_uint32(77), C.c_uint32(78)), C.c_float(-1.0), (C.c_float * 1)(LEVEL)

    def refused(kind, count=K, region=None, placements=IDENTITY, placement_count=1, reach=REACH, cap=4, min_length=3, deposit=POINTS | LINKS,
                out_rows=rows, then=None):
        pointer = np.ascontiguousarray(placements, np.float64).ctypes.data_as(C.POINTER(C.c_double))
        assert not L.beamformer_hip_track_peaks_last_frames(count, None if region is None else C.byref(region), level, 1, pointer, placement_count, 1,
                                                            reach, cap, min_length, deposit, out_rows, tracks, points, C.byref(totals[0]),
                                                            C.byref(totals[1]), C.byref(ms))
        assert bf.last_error()[0] == kind and (bytes(rows), bytes(tracks), bytes(points)) == untouched
        assert (totals[0].value, totals[1].value, ms.value) == (77, 78, -1.0)
        assert (then or state)() == (before if then is None else then.want)

    refused(E.InvalidAccess, region=bf.frame_region((20, 0, 0), (8, 1, 9)))              # a box past the grid
    refused(E.InvalidAccess, region=bf.frame_region((0, 0, 0), (7, 0, 9)))
    queued = int(newest_info(L).frame_id) + 1
    if queued < P.HIP_MAX_SCORED_FRAMES:
        refused(E.InvalidAccess, count=queued + 1)                                       # more frames than were ever queued
    refused(E.InvalidAccess, placement_count=2, placements=np.stack([IDENTITY, IDENTITY]))
    broken = IDENTITY.copy()
    broken[2, 1] = np.nan
    refused(E.InvalidAccess, placements=broken)
    refused(E.InvalidAccess, reach=float("inf"))
    refused(E.BufferOverflow, count=1)
    refused(E.BufferOverflow, min_length=0)
    refused(E.BufferOverflow, min_length=P.HIP_MAX_SCORED_FRAMES + 1)
    refused(E.InvalidAccess, deposit=4)
    refused(E.InvalidAccess, deposit=POINTS | LINKS | 8)
    refused(E.InvalidAccess, out_rows=None)
    # POINTS without a localisation map: the track map stays as it was; LINKS without a track map: the localisation map does
    bf.localisation_map_reset(None)
    links_only = lambda: [v.tobytes() for v in bf.track_map_copy(FIELD)[:2]]
    links_only.want = before[:2]
    for deposit in (POINTS, POINTS | LINKS):
        refused(E.InvalidAccess, deposit=deposit, then=links_only)
    got = track(K, LEVEL, IDENTITY, REACH, 12, deposit=LINKS)                            # (legal, keeps nothing: the map stays)
    assert len(got[1]) == 0 and links_only() == links_only.want
    bf.localisation_map_reset(FIELD)
    track(K, LEVEL, IDENTITY, REACH, 3, deposit=POINTS)
    bf.track_map_reset(None)
    points_only = lambda: [bf.localisation_map_copy(FIELD)[0].tobytes()]
    points_only.want = [before[3]]
    for deposit in (LINKS, POINTS | LINKS):
        refused(E.InvalidAccess, deposit=deposit, then=points_only)
