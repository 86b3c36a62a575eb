"""Peak pairs and the track map on the device (beamformer_hip_track_map_reset, beamformer_hip_pair_peaks_last_frames,
beamformer_hip_track_map_copy, beamformer_hip_queue_track_map; csrc/frame_tracks.hip).  Frames are produced by the small pushes of the
frame metrics and localisation tests and downloaded; the expected pair lists, rows and maps are the numpy reference
(tests/tracks_ref.py).

Everything compared is an integer or a bit pattern and is asked exactly: there is no tolerance anywhere.  On real frames the reference
runs on the downloaded frames.  On complex frames a magnitude may differ from numpy's by 1 ulp (tests/test_gpu_localisation.py explains
it), so there the reference pairs the records beamformer_hip_find_peaks_last_frames returns for the same frames: the call promises those
positions bit for bit.  The queued frames' double divisions are IEEE divisions on the device as in numpy: components 0..4 are compared
bit for bit."""
import ctypes as C

import numpy as np
import pytest

from ogl_beamforming_amd import lib as bf
from ogl_beamforming_amd import params as P
from tests import tracks_ref as ref
from tests import variants_cases as vc
from tests.frame_info import newest_info
from tests.ring_frames import (metrics_block as block, BOX, CAP, finer, fraction_of_max, map_view, pair, placement_onto, peak_lists as records_of,
                               same_pairs_call as same_call, same_map, variants_push)
from tests.scaffold import automatic_path, run_ring_worker  # noqa: F401

pytestmark = pytest.mark.gpu
E = P.LibError
IDENTITY = np.eye(3, 4)
FAR = np.array([[0.0, 0.0, 0.0, -1e6]] * 3)            # a placement that puts every peak outside any map


@pytest.fixture(autouse=True)
def maps_reset(automatic_path, bflib):
    yield
    bflib.localisation_map_reset(None)
    bflib.track_map_reset(None)


def teeth(numbers):
    """the case decides something: pairs, placed peaks left alone, and forward choices that are not returned"""
    pairs = sum(w["pairs"] for w in numbers)
    alone = sum(sum(w["unpaired"]) for w in numbers)
    one_sided = sum(int((w["forward"] != ref.NONE).sum()) - w["pairs"] for w in numbers)
    print(f"  teeth: {pairs} pairs, {alone} unpaired, {one_sided} forward choices not mutual")
    assert pairs >= 8 and alone >= 1 and one_sided >= 1


def shifted_views(points, count, step=0.04e-3):
    """`count` views of one box, each `step` further along every axis: the same scene seen from a grid that moves"""
    return [bf.view(points, tuple(v + k * step for v in vc.LO3), tuple(v + k * step for v in vc.HI3)) for k in range(count)]


def test_real_frames_a_plane_and_a_volume(bflib):
    # block B: three variants of a real plane, 24 x 1 x 40, whose peaks move with the speed of sound; the map 93 x 1 x 157
    acq = block("B")
    frames, ids = variants_push("B")
    assert frames.dtype == np.float32
    grid = map_view(finer(vc.POINTS), vc.LO, vc.HI)
    A = placement_onto(grid, acq.bp.das_voxel_transform, vc.POINTS)
    thresholds = fraction_of_max(frames, 0.1)
    reach = 6.0                                              # map voxels: a voxel and a half of the frames
    bf.track_map_reset(grid.output_points)
    rows, got = pair(3, thresholds, A, reach, deposit=True)
    counts, sums = ref.empty_map(grid.output_points)
    want, numbers = ref.pair_frames(list(frames), thresholds, A, reach, CAP, counts=counts, sums=sums)
    teeth(numbers)
    same_call(rows, got, want, numbers, 3, thresholds)
    info = same_map(grid.output_points, counts, sums)
    total = sum(w["pairs"] for w in numbers)
    assert [int(r.frame_id[0]) for r in rows] == ids[:2] and [int(r.frame_id[1]) for r in rows] == ids[1:]
    assert (info.calls, int(info.pairs), int(info.deposited), int(info.outside)) == (1, total, total, 0) and int(counts.sum()) == total
    # the offsets decide: without them other pairs
    assert ref.pair_frames(list(frames), thresholds, A, reach, CAP, use_offsets=False)[0].tobytes() != want.tobytes()

    # a real volume, 16 x 16 x 32, on three grids that move: one placement for all, so the peaks move in the map, 61 x 61 x 125
    acq = block("forces")
    views = shifted_views((16, 16, 32), 3)
    frames = [f.copy() for f in bflib.beamform_views(acq.bp, acq.rf, views, acq.filters)]
    assert all(f.dtype == np.float32 and f.shape == (32, 16, 16) for f in frames)
    grid = map_view(finer((16, 16, 32)), vc.LO3, vc.HI3)
    A = placement_onto(grid, views[0].das_voxel_transform, (16, 16, 32))
    bf.track_map_reset(grid.output_points)
    rows, got = pair(3, 0.0, A, reach, deposit=True)
    counts, sums = ref.empty_map(grid.output_points)
    want, numbers = ref.pair_frames(frames, 0.0, A, reach, CAP, counts=counts, sums=sums)
    teeth(numbers)
    same_call(rows, got, want, numbers, 3, 0.0)
    same_map(grid.output_points, counts, sums)


def test_complex_frames_pair_as_their_find_peaks_records_say(bflib):
    acq = block("A")
    frames, _ = variants_push("A")
    assert np.iscomplexobj(frames)
    grid = map_view(finer(vc.POINTS), vc.LO, vc.HI)
    A = placement_onto(grid, acq.bp.das_voxel_transform, vc.POINTS)
    thresholds = fraction_of_max(frames, 0.1)
    bf.track_map_reset(grid.output_points)
    rows, got = pair(3, thresholds, A, 6.0, deposit=True)
    counts, sums = ref.empty_map(grid.output_points)
    want, numbers = ref.pair_records(records_of(3, thresholds), A, 6.0, counts=counts, sums=sums)
    assert sum(w["pairs"] for w in numbers) >= 8
    same_call(rows, got, want, numbers, 3, thresholds)
    same_map(grid.output_points, counts, sums)
    # a volume with NaN voxels (coherency weighting) behind itself: every peak returns to where it was
    acq = block("D3")
    for _ in range(2):
        frame = bflib.beamform(acq.bp, acq.rf, acq.filters).copy()
    assert int(np.isnan(frame).sum()) >= 64
    rows, got = pair(2, 0.0, IDENTITY, 1.0)
    want, numbers = ref.pair_records(records_of(2, 0.0), IDENTITY, 1.0)
    same_call(rows, got, want, numbers, 2, 0.0)
    assert numbers[0]["pairs"] == numbers[0]["peaks"][0] >= 4 and not got["distance2"].any()


def queue_deposit(points, newest, thresholds, placements, use_offsets=False):
    """a frame of exactly known peaks: the peaks of the `newest` newest frames deposited into the localisation map under their
    placements, and the map queued with scale 1: (frame id, the frame)"""
    bf.localisation_map_reset(points)
    bf.accumulate_peaks_last_frames(newest, thresholds, placements, use_offsets)
    frame_id, _ = bf.queue_localisation_map(1.0)
    return frame_id, bf.copy_frame(frame_id)


def test_planted_motion(bflib):
    """one frame's peaks deposited under placements translated by k x (2, 0, 3) whole map voxels, each map queued: frames whose peaks
    move by exactly that.  The source's peaks lie two voxels apart at the least and the map is four times finer, so the planted peaks
    are isolated and seven map voxels apart: the nearest candidate within 4 is the peak's own image."""
    acq = block("B")
    frames, _ = variants_push("B")
    grid = map_view(finer(vc.POINTS), vc.LO, vc.HI)
    points = tuple(grid.output_points)
    A = placement_onto(grid, acq.bp.das_voxel_transform, vc.POINTS)
    level = fraction_of_max(frames[2:], 0.25)[0]
    shift, K = np.array([2.0, 0.0, 3.0]), 4
    planted = []
    for k in range(K):
        moved = A.copy()
        moved[:, 3] += k * shift
        # the newest k + 1 frames: the source, and the k frames queued so far, which are sent outside
        _, frame = queue_deposit(points, k + 1, [level] + [0.5] * k, np.stack([moved] + [FAR] * k))
        assert set(np.unique(frame)) == {0.0, 1.0}
        planted.append(frame)
    bf.track_map_reset(points)
    rows, got = pair(K, 0.5, IDENTITY, 4.0, use_offsets=False, deposit=True)
    counts, sums = ref.empty_map(points)
    want, numbers = ref.pair_frames(planted, 0.5, IDENTITY, 4.0, CAP, use_offsets=False, counts=counts, sums=sums)
    same_call(rows, got, want, numbers, K, 0.5)
    same_map(points, counts, sums)
    assert len(got) >= 3 * 8 and (got["displacement"] == shift).all() and (got["distance2"] == 13.0).all()
    assert all(w["pairs"] == w["peaks"][1] for w in numbers)                  # (a peak whose image left the map has no partner)
    fixed = (shift * 1048576.0).astype(np.int64)
    assert np.array_equal(sums, counts.astype(np.int64)[None] * fixed[:, None, None, None]) and int(counts.sum()) == len(got)
    assert counts.max() >= 1
    # the queued frames: the shift times the scale where there are pairs enough, 0 elsewhere
    least = int(counts.max())
    for component in range(3):
        for min_pairs in (1, least):
            frame_id, _ = bf.queue_track_map(component, 0.25, min_pairs)
            queued = bf.copy_frame(frame_id)
            assert np.array_equal(queued, np.where(counts >= min_pairs, np.float32(shift[component] * 0.25), np.float32(0.0)))
            assert np.array_equal(queued.view(np.uint32), ref.queued_frame(counts, sums, component, 0.25, min_pairs).view(np.uint32))


def test_more_than_one_tile_and_one_block(bflib):
    """the FORCES block on three moving 32 x 32 x 32 grids at threshold 0: about a thousand peaks a frame, four blocks of queries
    and four tiles of candidates"""
    acq = block("forces")
    frames = [f.copy() for f in bflib.beamform_views(acq.bp, acq.rf, shifted_views((32, 32, 32), 3), acq.filters)]
    bf.track_map_reset((32, 32, 32))
    rows, got = pair(3, 0.0, IDENTITY, 1.5, deposit=True)
    assert all(512 < int(r.peaks[k]) <= 4096 for r in rows for k in range(2)), [tuple(r.peaks) for r in rows]
    counts, sums = ref.empty_map((32, 32, 32))
    want, numbers = ref.pair_frames(frames, 0.0, IDENTITY, 1.5, CAP, counts=counts, sums=sums)
    teeth(numbers)
    same_call(rows, got, want, numbers, 3, 0.0)
    same_map((32, 32, 32), counts, sums)
    assert all(w["pairs"] > 256 for w in numbers)                              # the pair list of a frame pair comes from several blocks
    # a cap below what was found: pairs among the stored peaks only, and the rows say so
    cap = 600
    rows, got = pair(3, 0.0, IDENTITY, 1.5, cap=cap)
    want, numbers = ref.pair_frames(frames, 0.0, IDENTITY, 1.5, cap)
    same_call(rows, got, want, numbers, 3, 0.0, cap=cap)
    assert all(tuple(r.peaks) == (cap, cap) and min(r.found) > cap for r in rows) and got["a"].max() < cap and got["b"].max() < cap


def plant(points, lists):
    """consecutive Float32 frames of `points` with 1 at the voxels of each list and 0 elsewhere: (ids, frames).  A map of one voxel,
    queued once a position, gives frames of one peak; every frame is then the deposit of as many of those under translations, the
    frames planted before it sent outside"""
    most = max(len(positions) for positions in lists)
    bf.localisation_map_reset((1, 1, 1))
    bf.accumulate_peaks_last_frames(1, 0.0, np.zeros((3, 4)))                   # the peaks of whatever frame is the newest, all in the one bin
    for _ in range(most):
        bf.queue_localisation_map(1.0)
    ids, frames = [], []
    for j, positions in enumerate(lists):
        placements = [np.concatenate([np.zeros((3, 3)), np.array(p, np.float64).reshape(3, 1)], axis=1) for p in positions]
        frame_id, frame = queue_deposit(points, len(positions) + j, 0.5, np.stack(placements + [FAR] * j))
        expected = np.zeros(points[::-1], np.float32)
        for x, y, z in positions:
            expected[z, y, x] = 1.0
        assert np.array_equal(frame, expected)
        ids.append(frame_id)
        frames.append(frame)
    return ids, frames


def test_ties_go_to_the_lowest_rank_in_both_directions(bflib):
    variants_push("B")
    centre, cross = [(5, 0, 5)], [(5, 0, 7), (7, 0, 5), (5, 0, 3), (3, 0, 5)]          # four candidates at distance 2 exactly: d2 == R2
    ids, frames = plant((16, 1, 16), [centre, cross, centre])
    rows, got = pair(3, 0.5, IDENTITY, 2.0, use_offsets=False)
    want, numbers = ref.pair_frames(frames, 0.5, IDENTITY, 2.0, CAP, use_offsets=False)
    same_call(rows, got, want, numbers, 3, 0.5)
    # rank 0 of the cross is its lowest flat index, (5, 0, 3): chosen forward by the centre, and the one the centre chooses backward
    assert [tuple(int(v) for v in (r["frame"], r["a"], r["b"])) for r in got] == [(0, 0, 0), (1, 0, 0)]
    assert got["displacement"].tolist() == [[0.0, 0.0, -2.0], [0.0, 0.0, 2.0]] and got["distance2"].tolist() == [4.0, 4.0]
    assert [tuple(r.unpaired) for r in rows] == [(0, 3), (3, 0)] and [int(r.frame_id[0]) for r in rows] == ids[:2]
    # a hair below the distance: nothing is within reach
    rows, got = pair(3, 0.5, IDENTITY, float(np.nextafter(np.float32(2.0), np.float32(0.0))), use_offsets=False)
    assert len(got) == 0 and [tuple(r.unpaired) for r in rows] == [(1, 4), (4, 1)]


def copies_one_at_a_time(count, after):
    """the `count` newest frames (real) queued again one at a time, oldest first, as frames of their own; after(k) behind copy k"""
    weights = np.zeros((1, count), np.complex64)
    weights[0, 0] = 1.0
    for k in range(count):
        bf.mix_last_frames(count, weights)                   # the oldest of the `count` newest: the window moves with every copy
        after(k)


def test_map_algebra(bflib):
    acq = block("B")
    frames, _ = variants_push("B")
    grid = map_view(finer(vc.POINTS), vc.LO, vc.HI)
    points = tuple(grid.output_points)
    A = placement_onto(grid, acq.bp.das_voxel_transform, vc.POINTS)
    level = fraction_of_max(frames, 0.1)[1]
    # one call over three frames is the two calls over two frames, byte for byte: the copies arrive one at a time
    bf.track_map_reset(points)
    steps = []
    copies_one_at_a_time(3, lambda k: steps.append(pair(2, level, A, 6.0, deposit=True)) if k else None)
    stepwise = bf.track_map_copy()
    rows, got = pair(3, level, A, 6.0)                                            # deposit = 0: needs no map and changes none
    assert [bytes(c) for c in bf.track_map_copy()] == [bytes(c) for c in stepwise]
    counts, sums = ref.empty_map(points)
    want, numbers = ref.pair_frames(list(frames), level, A, 6.0, CAP, counts=counts, sums=sums)
    assert all(w["deposited"] for w in numbers)
    info = same_map(points, counts, sums)
    assert (info.calls, int(info.pairs)) == (2, len(want))
    for n, (two_rows, two) in enumerate(steps):
        mine = want[want["frame"] == n].copy()
        mine["frame"] = 0
        assert len(two) == numbers[n]["pairs"] and two.tobytes() == mine.tobytes()
        whole, alone = P.HipPeakPairs.from_buffer_copy(rows[n]), P.HipPeakPairs.from_buffer_copy(two_rows[0])
        assert (whole.deposited, whole.outside, alone.deposited, alone.outside) == (0, 0, numbers[n]["deposited"], numbers[n]["outside"])
        whole.first = alone.deposited = alone.outside = 0
        assert bytes(whole) == bytes(alone)
    got_plain = got.copy()
    assert not got_plain["deposited"].any()
    got_plain["deposited"] = want["deposited"]
    assert got_plain.tobytes() == want.tobytes()
    # a repeat from a reset: the same bytes; without a reset: twice the counts and the sums
    bf.track_map_reset(points)
    again_rows, again = pair(3, level, A, 6.0, deposit=True)
    same_call(again_rows, again, want, numbers, 3, level)
    same_map(points, counts, sums)
    pair(3, level, A, 6.0, deposit=True)
    info = same_map(points, counts * np.uint32(2), sums * 2)
    assert (info.calls, int(info.deposited)) == (2, 2 * len(want))
    # midpoints outside the map are counted and nothing is written: the map's origin moved to the middle of the frames
    shifted = A.copy()
    shifted[:, 3] -= (46.0, 0.0, 78.0)
    bf.track_map_reset(points)
    rows, got = pair(3, level, shifted, 6.0, deposit=True)
    counts, sums = ref.empty_map(points)
    want, numbers = ref.pair_frames(list(frames), level, shifted, 6.0, CAP, counts=counts, sums=sums)
    same_call(rows, got, want, numbers, 3, level)
    info = same_map(points, counts, sums)
    outside = sum(w["outside"] for w in numbers)
    assert 0 < outside < len(want) and (int(info.deposited), int(info.outside)) == (len(want) - outside, outside) and int(counts.sum()) == len(want) - outside
    # an unplaced frame: a coordinate that overflows pairs nothing
    beyond = A.copy()
    beyond[0, 0], beyond[0, 3] = 1e308, 1e308
    rows, got = pair(3, level, np.stack([A, beyond, A]), 6.0)
    want, numbers = ref.pair_frames(list(frames), level, np.stack([A, beyond, A]), 6.0, CAP)
    same_call(rows, got, want, numbers, 3, level)
    # (the peaks left of x = 0.79 stay finite, 10^308 map voxels away from anything)
    assert len(got) == 0 and 0 < rows[0].unplaced[1] < rows[0].peaks[1] and rows[1].unplaced[0] == rows[0].unplaced[1] and rows[0].unplaced[0] == 0


def test_boxes_and_frames_of_different_grids(bflib):
    # a box of the FORCES volume on two moving grids: peaks judged by their frame's neighbours
    acq = block("forces")
    views = shifted_views((16, 16, 32), 2)
    frames = [f.copy() for f in bflib.beamform_views(acq.bp, acq.rf, views, acq.filters)]
    rows, got = pair(2, 0.0, IDENTITY, 1.5, box=BOX)
    want, numbers = ref.pair_frames(frames, 0.0, IDENTITY, 1.5, CAP, first=BOX[0], count=BOX[1])
    same_call(rows, got, want, numbers, 2, 0.0, box=BOX)
    assert numbers[0]["pairs"] >= 8
    # a views push: frames of different grids, each with its own placement onto one map
    acq = block("B")
    grids = [(150, 1, 9), (64, 1, 5), (63, 2, 3), (1, 1, 40), (65, 1, 1)]
    views = [bflib.view(points, vc.LO, vc.HI) for points in grids]
    frames = bflib.beamform_views(acq.bp, acq.rf, views, acq.filters)
    grid = bf.view((97, 3, 65), (vc.LO[0], -1e-3, vc.LO[2]), (vc.HI[0], 1e-3, vc.HI[2]))
    points = tuple(grid.output_points)
    placements = np.stack([placement_onto(grid, v.das_voxel_transform, v.output_points) for v in views])
    bf.track_map_reset(points)
    rows, got = pair(5, 0.0, placements, 8.0, deposit=True)
    counts, sums = ref.empty_map(points)
    want, numbers = ref.pair_frames([f.copy() for f in frames], 0.0, placements, 8.0, CAP, counts=counts, sums=sums)
    same_call(rows, got, want, numbers, 5, 0.0)
    same_map(points, counts, sums)
    assert len(want) >= 1 and [tuple(r.peaks) for r in rows] == [tuple(w["peaks"]) for w in numbers]


def test_the_queued_frames(bflib):
    L = bflib.library()
    acq = block("B")
    frames, ids = variants_push("B")
    grid = map_view((47, 1, 79), vc.LO, vc.HI)               # twice finer: bins that collect several pairs
    points = tuple(grid.output_points)
    A = placement_onto(grid, acq.bp.das_voxel_transform, vc.POINTS)
    thresholds = fraction_of_max(frames, 0.05)
    bf.track_map_reset(points)
    pair(3, thresholds, A, 4.0, deposit=True)
    pair(3, thresholds, A, 4.0, use_offsets=False, deposit=True)
    counts, sums, _ = bf.track_map_copy()
    assert len(np.unique(counts)) >= 3 and len(np.unique(sums)) >= 16
    newest = ids[2]
    for component, scale, min_pairs in ((0, 0.37, 1), (1, 1.0, 0), (2, -2.5, 2), (3, 0.37, 1), (4, 3.0, 1), (4, 1.0, 3)):
        frame_id, ms = bf.queue_track_map(component, scale, min_pairs, tag=5 + component)
        newest += 1
        assert frame_id == newest and ms > 0
        info = bf.frame_info(frame_id)
        assert tuple(info.points) == points and info.data_kind == int(P.DataKind.Float32) and info.frame_id == frame_id
        assert int(newest_info(L).frame_id) == frame_id
        queued = bf.copy_frame(frame_id)
        expected = ref.queued_frame(counts, sums, component, scale, min_pairs)
        assert queued.dtype == np.float32 and np.array_equal(queued.view(np.uint32), expected.view(np.uint32)), component
        assert np.count_nonzero(queued) >= (4 if component != 1 else 0)
        metrics, _ = bf.score_last_frames(1)
        assert metrics[0].frame_id == frame_id and metrics[0].image_plane_tag == 5 + component
        assert metrics[0].parameter_block == bf.frame_info(ids[2]).parameter_block and int(metrics[0].voxels) == expected.size
    # the map is as it was, the variants push still the newest multi-frame push, and the timing row is the localisation map's frame's
    again = bf.track_map_copy()
    assert again[0].tobytes() == counts.tobytes() and again[1].tobytes() == sums.tobytes()
    assert int(bf.last_variants_info().first_frame_id) == ids[0]
    def timing_row():
        row = P.HipFrameTimings()
        served = L.beamformer_hip_get_last_frame_timings(C.byref(row))
        return served, row.stage_count, list(row.stage_kind), int(row.das_pairs), int(row.das_voxels), row.das_taps, row.das_path

    bf.localisation_map_reset(points)
    bf.accumulate_peaks_last_frames(1, 0.0, IDENTITY)
    bf.queue_localisation_map(1.0, tag=3)
    of_the_density = timing_row()
    bf.queue_track_map(3, 1.0, 1, tag=3)
    assert timing_row() == of_the_density
    # without a synchronise: another id
    frame_id, ms = bf.queue_track_map(3, 2.0, 1, timed=False)
    assert frame_id == newest + 3 and ms == 0.0
    assert np.array_equal(bf.copy_frame(frame_id).view(np.uint32), ref.queued_frame(counts, sums, 3, 2.0).view(np.uint32))


def test_refusals_on_the_device_change_nothing(bflib):
    L = bflib.library()
    acq = block("B")
    frames, ids = variants_push("B")
    grid = map_view(finer(vc.POINTS), vc.LO, vc.HI)
    points = tuple(grid.output_points)
    A = placement_onto(grid, acq.bp.das_voxel_transform, vc.POINTS)
    thresholds = fraction_of_max(frames, 0.25)
    bf.localisation_map_reset(points)
    bf.accumulate_peaks_last_frames(3, thresholds, A)
    bf.track_map_reset(points)
    pair(3, thresholds, A, 6.0, deposit=True)

    def state():
        tracks = bf.track_map_copy()
        density = bf.localisation_map_copy()
        return [bytes(v) if not isinstance(v, np.ndarray) else v.tobytes() for v in tracks + density] + [bytes(newest_info(L))]

    before = state()
    rows, records = (P.HipPeakPairs * 4)(), (P.HipPeakPair * 64)()
    C.memset(rows, 0xA5, C.sizeof(rows))
    C.memset(records, 0xA5, C.sizeof(records))
    untouched = bytes(rows), bytes(records)
    total, ms, frame = C.c_uint32(77), C.c_float(-1.0), C.c_uint32(77)
    level = (C.c_float * 1)(0.0)

    def refused(kind, count=3, region=None, placements=A, placement_count=1, reach=6.0, deposit=1):
        pointer = np.ascontiguousarray(placements, np.float64).ctypes.data_as(C.POINTER(C.c_double))
        assert not L.beamformer_hip_pair_peaks_last_frames(count, None if region is None else C.byref(region), level, 1, pointer, placement_count, 1,
                                                           reach, 16, deposit, rows, records, C.byref(total), C.byref(ms))
        assert bf.last_error()[0] == kind and (bytes(rows), bytes(records)) == untouched and total.value == 77 and ms.value == -1.0
        assert state() == before

    refused(E.InvalidAccess, region=bf.frame_region((20, 0, 0), (8, 1, 9)))              # a box past the grid
    refused(E.InvalidAccess, region=bf.frame_region((0, 0, 0), (7, 0, 9)))
    queued = int(newest_info(L).frame_id) + 1
    if queued < P.HIP_MAX_SCORED_FRAMES:
        refused(E.InvalidAccess, count=queued + 1)                                       # more frames than were ever queued
    refused(E.InvalidAccess, placement_count=2, placements=np.stack([A, A]))
    broken = A.copy()
    broken[2, 1] = np.nan
    refused(E.InvalidAccess, placements=broken)
    refused(E.InvalidAccess, reach=float("inf"))
    refused(E.InvalidAccess, reach=-0.5)
    refused(E.BufferOverflow, count=1)
    # the map's own calls
    out, sums = (C.c_uint32 * 16)(*([9] * 16)), (C.c_int64 * 48)(*([9] * 48))
    voxels = int(np.prod(points))
    assert not L.beamformer_hip_track_map_copy(out, sums, voxels - 1, None) and bf.last_error()[0] == E.ExportSpaceOverflow
    assert list(out) == [9] * 16 and list(sums) == [9] * 48
    assert not L.beamformer_hip_track_map_reset((C.c_uint32 * 3)(4, 0, 4)) and bf.last_error()[0] == E.InvalidAccess
    assert not L.beamformer_hip_track_map_reset((C.c_uint32 * 3)(1 << 10, 1 << 10, 1 << 10)) and bf.last_error()[0] == E.BufferOverflow
    for component, scale in ((0, float("inf")), (5, 1.0)):
        assert not L.beamformer_hip_queue_track_map(component, scale, 1, 0, C.byref(frame), C.byref(ms)) and bf.last_error()[0] == E.InvalidAccess
    assert frame.value == 77 and ms.value == -1.0 and state() == before
    # a map that has not been deposited into since its reset is not queued; a call without deposit does not count
    bf.track_map_reset(points)
    pair(3, thresholds, A, 6.0)
    newest = bytes(newest_info(L))
    assert not L.beamformer_hip_queue_track_map(3, 1.0, 1, 0, C.byref(frame), C.byref(ms)) and bf.last_error()[0] == E.InvalidAccess
    assert frame.value == 77 and ms.value == -1.0 and bytes(newest_info(L)) == newest
    zeros = bf.track_map_copy()
    assert not zeros[0].any() and not zeros[1].any() and (zeros[2].calls, int(zeros[2].pairs)) == (0, 0)
    # no map: released; a call without deposit still runs
    bf.track_map_reset(None)
    pointer = A.ctypes.data_as(C.POINTER(C.c_double))
    assert not L.beamformer_hip_pair_peaks_last_frames(3, None, level, 1, pointer, 1, 1, 6.0, 16, 1, rows, records, C.byref(total), C.byref(ms))
    assert bf.last_error()[0] == E.InvalidAccess and (bytes(rows), bytes(records)) == untouched and bytes(newest_info(L)) == newest
    assert not L.beamformer_hip_track_map_copy(out, sums, 16, None) and bf.last_error()[0] == E.InvalidAccess
    assert not L.beamformer_hip_queue_track_map(3, 1.0, 1, 0, C.byref(frame), None) and bf.last_error()[0] == E.InvalidAccess
    assert len(pair(3, thresholds, A, 6.0)[1]) >= 8
    # the localisation map went through all of it untouched
    assert bf.localisation_map_copy()[0].tobytes() == before[3]
    # a tombstone among the frames (a variants push that fails at its DAS stage, without any device fault)
    rf = np.ascontiguousarray(acq.rf)
    array = (P.HipDasVariant * 3)(*vc.candidates(acq.bp))
    L.beamformer_hip_set_das_path(P.HIP_DAS_PATH_FAIL_VIEWS_DAS)
    assert not L.beamformer_hip_push_data_variants_with_compute(rf.ctypes.data_as(C.c_void_p), rf.nbytes, array, 3, 0, 0)
    L.beamformer_hip_set_das_path(0)
    assert not L.beamformer_hip_pair_peaks_last_frames(2, None, level, 1, pointer, 1, 1, 6.0, 16, 0, rows, records, C.byref(total), C.byref(ms))
    assert bf.last_error()[0] == E.InvalidAccess and (bytes(rows), bytes(records)) == untouched and total.value == 77


def test_the_ring_a_queued_track_map_that_wraps_and_one_that_does_not_fit():
    """a 1 MiB frame ring in a process of its own (the ring is sized once per process): tests/tracks_wrap_worker.py"""
    run_ring_worker("tracks_wrap_worker", 1 << 20, expect=("refused", "wrapped"))
