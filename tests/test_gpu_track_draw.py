"""Drawn tracks on the device (beamformer_hip_draw_tracks_last_frames; csrc/frame_tracks.hip: smooth, draw, behind the chain's
launches).  Frames are PLANTED (tests/planted.py) by one burst push, as tests/test_gpu_track_chains.py does it, and the numpy reference
(tests/track_draw_ref.py) runs on the downloaded frames; the plans are tests/track_plans.py's, and tests/test_track_chains_host.py and
tests/test_track_draw_host.py check without a device that they hold what they claim.  On complex frames the reference draws
the records beamformer_hip_find_peaks_last_frames returns.

Everything compared is an integer or a bit pattern and is asked exactly: there is no tolerance in this file."""
import ctypes as C

import numpy as np
import pytest

from ogl_beamforming_amd import lib as bf
from ogl_beamforming_amd import params as P
from tests import localisation_ref, tracks_ref
from tests import ring_frames
from tests import track_plans
from tests import track_draw_ref as ref
from tests import variants_cases as vc
from tests.frame_info import newest_info
from tests.ring_frames import (metrics_block as block, planted_burst as burst, draw, finer, fraction_of_max, fresh_point_and_track_maps as fresh_maps,
                               LINKS, map_view, placement_onto, POINTS, same_infos, same_point_and_track_maps as same_maps, same_rows, variants_push)
from tests.scaffold import automatic_path  # noqa: F401

pytestmark = pytest.mark.gpu
E = P.LibError
IDENTITY, LEVEL, REACH, CAP = track_plans.IDENTITY, track_plans.LEVEL, track_plans.REACH, ring_frames.CAP
FOUR = track_plans.scaled(4)
FIELD4 = track_plans.times(track_plans.PLANE_FIELD, 4)                    # both maps over the plane plan, 4 x finer: its spots beyond x = 20 draw partly outside


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


@pytest.fixture
def own(bflib):
    """the draw plan on the device: the 6 downloaded frames"""
    stack, _ = track_plans.draw_plan()
    frames, _ = burst(stack)
    return list(frames)


def one_call(frames, placements, reach, min_length, smooth, deposit, point_field, track_field, thresholds=LEVEL, cap=CAP, use_offsets=True, box=None):
    """one call on fresh maps against the reference: rows, both maps and both infos, byte for byte; returns the reference's result"""
    K = len(frames)
    density, counts, sums = fresh_maps(point_field, track_field)
    rows = draw(K, thresholds, placements, reach, min_length, smooth, cap, use_offsets, deposit, box)
    want = ref.draw_frames(frames, thresholds, placements, reach, cap, min_length, smooth, use_offsets, *((None, None) if box is None else box),
                           deposit=deposit, point_map=density, counts=counts, sums=sums)
    same_rows(rows, want, K, thresholds, cap, box)
    point_info, link_info = same_maps(point_field, track_field, density, counts, sums)
    same_infos(point_info, link_info, 1, want["rows"], deposit)
    for row in rows:                                                      # samples - repeats is each kind's deposited + outside
        drawn = row.samples - row.repeats
        assert (not deposit & POINTS or drawn == row.points_deposited + row.points_outside) and \
               (not deposit & LINKS or drawn == row.links_deposited + row.links_outside)
    return want


# ----------------------------------------------------------------------------- 1: the plane plan

@pytest.mark.parametrize("min_length", [1, 3, 12])
def test_the_plane_plan_at_three_lengths_four_widths_and_every_deposit(min_length, plane, bflib):
    for smooth in (0, 1, 3, 8):
        for deposit in (0, POINTS, LINKS, POINTS | LINKS):
            want = one_call(plane, FOUR, 6.0, min_length, smooth, deposit, FIELD4, FIELD4)
        total = ref.totals(want["rows"])
        print(f"  min_length {min_length}, w {smooth}: {total}")
        if min_length == 12:
            assert not any(total.values())                            # min_length > count: legal, keeps and draws nothing
        else:
            assert total["samples"] >= 40 and total["repeats"] >= 13 and total["points_outside"] >= 1 and total["links_outside"] >= 1
            assert total["lone"] == (2 if min_length == 1 else 0)


# ----------------------------------------------------------------------------- 2: maps of different sizes

def test_a_sample_inside_one_map_and_outside_the_other(plane, bflib):
    small = (40, 4, 160)
    for point_field, track_field in ((small, FIELD4), (FIELD4, small)):
        want = one_call(plane, FOUR, 6.0, 1, 1, POINTS | LINKS, point_field, track_field)
        total = ref.totals(want["rows"])
        assert total["points_deposited"] != total["links_deposited"] and min(total["points_deposited"], total["links_deposited"]) >= 20


# ----------------------------------------------------------------------------- 3, 4, 5: the draw plan

@pytest.mark.parametrize("case", track_plans.DRAW_CALLS, ids=lambda case: case[0])
def test_the_draw_plan_wide_far_and_at_negative_coordinates(case, own, bflib):
    name, A, reach, point_field, track_field = case
    for min_length, smooth in ((1, 0), (2, 1), (1, 8)):
        want = one_call(own, A, reach, min_length, smooth, POINTS | LINKS, point_field, track_field)
        total = ref.totals(want["rows"])
        print(f"  {name}, min_length {min_length}, w {smooth}: {total}")
        if smooth:
            continue
        sizes = [len(B) for track in want["links"] for skipped, d, B, drawn in track if not skipped]
        if case is track_plans.WIDE:                                             # a link's samples cross any lane group and a whole wave
            assert max(sizes) == 72 and total["links_skipped"] == 0 and total["points_deposited"] >= 100 and total["links_outside"] >= 100
        elif case is track_plans.FAR_AWAY:                                       # the skipped links would have crossed the maps: they stay zero
            assert total["links_skipped"] == 2 and total["points_deposited"] == 0 and total["links_deposited"] == 0 and max(sizes) == 4096
        elif case is track_plans.FAR_EDGE:                                       # e = 4096 exactly still draws
            assert total["links_skipped"] == 2 and max(sizes) == 4096 and total["links_deposited"] >= 4096
        else:
            assert total["repeats"] >= 5 and 1 in sizes and total["points_outside"] >= 10 and total["lone"] == 1


# ----------------------------------------------------------------------------- 6: the lattice

def test_a_lattice_of_more_than_512_peaks_a_frame(bflib):
    stack, placements = track_plans.volume_plan()
    frames, _ = burst(stack)
    field = (36, 48, 96)                                                  # the chain tests' field, 3 x finer: the lattice's last columns lie outside
    for smooth in (0, 2):
        want = one_call(list(frames), placements * 3.0, 3.0, 3, smooth, POINTS | LINKS, field, field)
        total = ref.totals(want["rows"])
        assert all(r["peaks"] > 512 for r in want["rows"]) and len(want["tracks"]) > 256 and total["samples"] >= total["kept_links"] > 512
        assert total["points_outside"] >= 1 and total["points_deposited"] >= 512


# ----------------------------------------------------------------------------- 7: equality with the track call

def test_one_sample_a_link_leaves_the_track_calls_track_map(own, bflib):
    K, box, field = len(own), track_plans.EQUALITY_BOX, (24, 1, 40)
    bf.track_map_reset(field)
    ring_frames.track(K, LEVEL, IDENTITY, REACH, 1, use_offsets=False, deposit=LINKS, box=box)
    of_the_tracks = bf.track_map_copy(field)
    bf.track_map_reset(field)
    rows = draw(K, LEVEL, IDENTITY, REACH, 1, 0, use_offsets=False, deposit=LINKS, box=box)
    mine = bf.track_map_copy(field)
    assert all(r.repeats == 0 and r.links_skipped == 0 and r.samples == r.kept_links for r in rows) and sum(r.samples for r in rows) >= 8
    assert mine[0].tobytes() == of_the_tracks[0].tobytes() and mine[1].tobytes() == of_the_tracks[1].tobytes()
    assert bytes(mine[2]) == bytes(of_the_tracks[2]) and int(mine[2].deposited) == sum(r.samples for r in rows)


# ----------------------------------------------------------------------------- 8: the queue calls behind a draw

def test_both_maps_queue_behind_a_draw(plane, bflib):
    L = bflib.library()
    K = len(plane)
    density, counts, sums = fresh_maps(FIELD4, FIELD4)
    frame, ms = C.c_uint32(77), C.c_float(-1.0)
    draw(K, LEVEL, FOUR, 6.0, 3, 1)                                       # a call without deposit does not count: neither map is queued behind it
    assert not L.beamformer_hip_queue_localisation_map(1.0, 0, C.byref(frame), C.byref(ms)) and bf.last_error()[0] == E.InvalidAccess
    assert not L.beamformer_hip_queue_track_map(3, 1.0, 1, 0, C.byref(frame), C.byref(ms)) and bf.last_error()[0] == E.InvalidAccess
    newest = int(newest_info(L).frame_id)
    block_of_newest = bf.frame_info(newest).parameter_block
    first = None
    for _ in range(2):                                                    # twice: the maps add up, the rows are equal
        rows = draw(K, LEVEL, FOUR, 6.0, 3, 1, deposit=POINTS | LINKS)
        want = ref.draw_frames(plane, LEVEL, FOUR, 6.0, CAP, 3, 1, deposit=POINTS | LINKS, point_map=density, counts=counts, sums=sums)
        first = first or bytes(rows)
        assert bytes(rows) == first
    point_info, link_info = same_maps(FIELD4, FIELD4, density, counts, sums)
    same_infos(point_info, link_info, 2, want["rows"], POINTS | LINKS)
    assert int(density.max()) >= 2 and (density % 2 == 0).all()
    frame_id, _ = bf.queue_localisation_map(0.5, tag=4)
    assert frame_id == newest + 1 and bf.frame_info(frame_id).parameter_block == block_of_newest
    assert np.array_equal(bf.copy_frame(frame_id).view(np.uint32), localisation_ref.queued_frame(density, 0.5).view(np.uint32))
    for component, scale, min_pairs in ((2, 0.37, 1), (3, 1.0, 2), (4, 3.0, 1)):
        frame_id, _ = bf.queue_track_map(component, scale, min_pairs, tag=5)
        assert bf.frame_info(frame_id).parameter_block == block_of_newest
        expected = tracks_ref.queued_frame(counts, sums, component, scale, min_pairs)
        assert np.array_equal(bf.copy_frame(frame_id).view(np.uint32), expected.view(np.uint32)) and np.count_nonzero(expected) >= 16


# ----------------------------------------------------------------------------- 9: complex frames

def test_complex_frames_draw_as_their_find_peaks_records_say(bflib):
    acq = block("A")
    frames, ids = variants_push("A")
    assert np.iscomplexobj(frames)
    grid = map_view(finer(vc.POINTS), vc.LO, vc.HI)
    field = tuple(grid.output_points)
    A = placement_onto(grid, acq.bp.das_voxel_transform, vc.POINTS)
    thresholds = fraction_of_max(frames, 0.1)
    samples = 0
    for min_length, smooth, use_offsets in ((1, 0, True), (2, 1, True), (3, 2, True), (2, 0, False)):
        density, counts, sums = fresh_maps(field, field)
        rows = draw(3, thresholds, A, 6.0, min_length, smooth, use_offsets=use_offsets, deposit=POINTS | LINKS)
        want = ref.draw_records(ring_frames.peak_lists(3, thresholds), A, 6.0, min_length, smooth, use_offsets, deposit=POINTS | LINKS,
                                point_map=density, counts=counts, sums=sums)
        same_rows(rows, want, 3, thresholds)
        same_maps(field, field, density, counts, sums)
        samples += ref.totals(want["rows"])["samples"]
        assert [int(r.frame_id) for r in rows] == ids
    assert samples >= 16


# ----------------------------------------------------------------------------- 10: placements, caps, boxes, thresholds, refusals

def test_an_unplaced_frame_a_cap_a_box_and_thresholds_a_frame(plane, bflib):
    K = len(plane)
    # frame 5 placed at infinity: finite entries whose sum overflows (every spot has x >= 2); every track breaks there
    lost = np.stack([FOUR] * K)
    lost[5, 0, 0] = lost[5, 0, 3] = 1.7e308
    want = one_call(plane, lost, 6.0, 2, 1, POINTS | LINKS, FIELD4, FIELD4)
    assert want["rows"][5]["unplaced"] == want["rows"][5]["peaks"] == 6 and want["rows"][4]["kept_links"] == 0 and want["rows"][4]["samples"] == 0
    # max_per_frame below found: the first three peaks of a frame in flat order
    want = one_call(plane, FOUR, 6.0, 2, 1, POINTS | LINKS, FIELD4, FIELD4, cap=3)
    assert any(r["found"] > 3 for r in want["rows"]) and all(r["peaks"] <= 3 for r in want["rows"]) and ref.totals(want["rows"])["samples"] >= 8
    # a box that leaves out the spots at x = 2 and from x = 20 on; without offsets
    box = ((4, 0, 0), (16, 1, 40))
    for use_offsets in (True, False):
        want = one_call(plane, FOUR, 6.0, 2, 2, POINTS | LINKS, FIELD4, FIELD4, use_offsets=use_offsets, box=box)
        assert sorted(want["lengths"]) == [1, 2, 5, 6, 8, 9]
    # per-frame thresholds: frame 6 asks for more than the spots' height, and has no peak
    levels = np.full(K, LEVEL, np.float32)
    levels[6] = 2 * track_plans.HEIGHT
    want = one_call(plane, FOUR, 6.0, 1, 3, POINTS | LINKS, FIELD4, FIELD4, thresholds=levels)
    assert want["rows"][6]["peaks"] == 0 and max(want["lengths"]) == 6
    # the newest frames of a longer ring: a call over the 4 newest frames sees only them
    density, counts, sums = fresh_maps(FIELD4, FIELD4)
    rows = draw(4, LEVEL, FOUR, 6.0, 2, 1, deposit=POINTS | LINKS)
    want = ref.draw_frames(plane[-4:], LEVEL, FOUR, 6.0, CAP, 2, 1, deposit=POINTS | LINKS, point_map=density, counts=counts, sums=sums)
    same_rows(rows, want, 4, LEVEL)
    same_maps(FIELD4, FIELD4, density, counts, sums)


def test_refusals_on_the_device_change_nothing(plane, bflib):
    L = bflib.library()
    K = len(plane)
    fresh_maps(FIELD4, FIELD4)
    draw(K, LEVEL, FOUR, 6.0, 3, 1, deposit=POINTS | LINKS)

    def state():
        tracks, density = bf.track_map_copy(FIELD4), bf.localisation_map_copy(FIELD4)
        return [bytes(v) if not isinstance(v, np.ndarray) else v.tobytes() for v in tracks + density] + [bytes(newest_info(L))]

    before = state()
    rows = (P.HipDrawnFrame * 16)()
    C.memset(rows, 0xA5, C.sizeof(rows))
    untouched = bytes(rows)
    ms, level = C.c_float(-1.0), (C.c_float * 1)(LEVEL)

    def refused(kind, count=K, region=None, placements=FOUR, placement_count=1, reach=6.0, cap=4, min_length=3, smooth=1, deposit=POINTS | LINKS,
                out_rows=rows, then=None):
        pointer = np.ascontiguousarray(placements, np.float64).ctypes.data_as(C.POINTER(C.c_double))
        assert not L.beamformer_hip_draw_tracks_last_frames(count, None if region is None else C.byref(region), level, 1, pointer, placement_count, 1,
                                                            reach, cap, min_length, smooth, deposit, out_rows, C.byref(ms))
        assert bf.last_error()[0] == kind and bytes(rows) == untouched and ms.value == -1.0
        assert (then or state)() == (before if then is None else then.want)

    refused(E.InvalidAccess, region=bf.frame_region((20, 0, 0), (8, 1, 9)))              # a box past the grid
    refused(E.InvalidAccess, region=bf.frame_region((0, 0, 0), (7, 0, 9)))
    queued = int(newest_info(L).frame_id) + 1
    if queued < P.HIP_MAX_SCORED_FRAMES:
        refused(E.InvalidAccess, count=queued + 1)                                       # more frames than were ever queued
    refused(E.InvalidAccess, placement_count=2, placements=np.stack([FOUR, FOUR]))
    broken = FOUR.copy()
    broken[2, 1] = np.nan
    refused(E.InvalidAccess, placements=broken)
    refused(E.InvalidAccess, reach=float("inf"))
    refused(E.BufferOverflow, count=1)
    refused(E.BufferOverflow, min_length=0)
    refused(E.BufferOverflow, min_length=P.HIP_MAX_SCORED_FRAMES + 1)
    refused(E.BufferOverflow, smooth=P.HIP_MAX_TRACK_SMOOTH + 1)
    refused(E.InvalidAccess, deposit=4)
    refused(E.InvalidAccess, deposit=POINTS | LINKS | 8)
    refused(E.InvalidAccess, out_rows=None)
    # POINTS without a localisation map: the track map stays as it was; LINKS without a track map: the localisation map does
    bf.localisation_map_reset(None)
    links_only = lambda: [v.tobytes() for v in bf.track_map_copy(FIELD4)[:2]]
    links_only.want = before[:2]
    for deposit in (POINTS, POINTS | LINKS):
        refused(E.InvalidAccess, deposit=deposit, then=links_only)
    rows_of_nothing = draw(K, LEVEL, FOUR, 6.0, 12, 1, deposit=LINKS)                    # (legal, keeps nothing: the map stays)
    assert sum(r.samples for r in rows_of_nothing) == 0 and links_only() == links_only.want
    bf.localisation_map_reset(FIELD4)
    draw(K, LEVEL, FOUR, 6.0, 3, 1, deposit=POINTS)
    bf.track_map_reset(None)
    points_only = lambda: [bf.localisation_map_copy(FIELD4)[0].tobytes()]
    points_only.want = [before[3]]
    for deposit in (LINKS, POINTS | LINKS):
        refused(E.InvalidAccess, deposit=deposit, then=points_only)
