"""The localisation map on the device (beamformer_hip_localisation_map_reset, beamformer_hip_accumulate_peaks_last_frames,
beamformer_hip_localisation_map_copy, beamformer_hip_queue_localisation_map; csrc/frame_peaks.hip).  Frames are produced by the small
pushes of the frame metrics and frame peaks tests and downloaded; the expected maps are the numpy reference (tests/localisation_ref.py).

Everything compared is an integer or a bit pattern and is asked exactly: there is no tolerance anywhere.  On real frames every value
that takes part -- the decision value, the magnitudes, the parabola's offsets -- is formed by the same IEEE operations on the device and
in numpy, and the placement is float64 arithmetic in a fixed order: the map is the reference applied to the downloaded frames, byte for
byte.  On complex frames a magnitude may differ from numpy's by 1 ulp (tests/test_gpu_frame_peaks.py), so there the reference bins the
records beamformer_hip_find_peaks_last_frames returns for the same frames: the call promises those positions bit for bit."""
import ctypes as C

import numpy as np
import pytest

from ogl_beamforming_amd import lib as bf
from ogl_beamforming_amd import params as P
from tests import frame_peaks_ref
from tests import localisation_ref as ref
from tests import variants_cases as vc
from tests.frame_info import newest_info
from tests.ring_frames import (binned_records, metrics_block as block, BOX, check_rows, finer, fraction_of_max, map_view, placement_onto, points_of,
                               run_localise as run, same_localise as same, variants_push)
from tests.scaffold import automatic_path, run_ring_worker  # noqa: F401

pytestmark = pytest.mark.gpu
E = P.LibError


@pytest.fixture(autouse=True)
def map_reset(automatic_path, bflib):
    yield
    bflib.localisation_map_reset(None)


def test_real_frames_a_plane_and_a_volume(bflib):
    # block B: three variants of a real plane, 24 x 1 x 40; the map 93 x 1 x 157
    acq = block("B")
    frames, ids = variants_push("B")
    assert frames.dtype == np.float32
    grid = map_view(finer(vc.POINTS), vc.LO, vc.HI)
    A = placement_onto(grid, acq.bp.das_voxel_transform, vc.POINTS)
    thresholds = fraction_of_max(frames, 0.25)
    counts, rows, info = run(grid, frames, thresholds, A)
    expected, numbers = ref.accumulate(grid.output_points, frames, thresholds, A)
    same(counts, expected)
    check_rows(rows, numbers, frames, thresholds)
    assert [int(r.frame_id) for r in rows] == ids
    total = sum(n["found"] for n in numbers)
    assert (info.calls, int(info.deposited), int(info.outside)) == (1, total, 0) and int(counts.sum()) == total >= 24
    # the case has teeth: the offsets move peaks to other bins, and the bins are not the coarse voxels
    without, _ = ref.accumulate(grid.output_points, frames, thresholds, A, use_offsets=False)
    assert without.tobytes() != expected.tobytes() and int(expected.sum()) > int(expected[::4, :, ::4].sum())

    # a real volume, 16 x 16 x 32: one frame, the map 61 x 61 x 125
    acq = block("forces")
    frame = bflib.beamform(acq.bp, acq.rf, acq.filters).copy()
    assert frame.dtype == np.float32 and frame.shape == (32, 16, 16)
    grid = map_view(finer(points_of(frame)), vc.LO3, vc.HI3)
    A = placement_onto(grid, acq.bp.das_voxel_transform, points_of(frame))
    threshold = fraction_of_max([frame], 0.05)[0]
    counts, rows, info = run(grid, [frame], threshold, A)
    expected, numbers = ref.accumulate(grid.output_points, [frame], threshold, A)
    same(counts, expected)
    check_rows(rows, numbers, [frame], threshold)
    assert numbers[0]["found"] >= 4 and int(info.deposited) == numbers[0]["found"]
    # ... and its box, judged by the frame's neighbours
    counts, rows, _ = run(grid, [frame], threshold, A, box=BOX)
    expected, numbers = ref.accumulate(grid.output_points, [frame], threshold, A, first=BOX[0], count=BOX[1])
    same(counts, expected)
    check_rows(rows, numbers, [frame], threshold, box=BOX)


def test_complex_frames_land_where_their_find_peaks_records_say(bflib):
    acq = block("A")
    frames, _ = variants_push("A")
    assert np.iscomplexobj(frames)
    grid = map_view(finer(vc.POINTS), vc.LO, vc.HI)
    A = placement_onto(grid, acq.bp.das_voxel_transform, vc.POINTS)
    thresholds = fraction_of_max(frames, 0.25)
    counts, rows, _ = run(grid, frames, thresholds, A)
    expected, numbers = binned_records(grid.output_points, 3, thresholds, A)
    same(counts, expected)
    check_rows(rows, numbers, frames, thresholds)
    assert sum(n["found"] for n in numbers) >= 24
    # a volume with NaN voxels (coherency weighting), whole and boxed
    acq = block("D3")
    frame = bflib.beamform(acq.bp, acq.rf, acq.filters).copy()
    assert int(np.isnan(frame).sum()) >= 64
    grid = map_view(finer(points_of(frame)), (-12e-3, -12e-3, 0.5e-3), (12e-3, 12e-3, 5.5e-3))
    A = placement_onto(grid, acq.bp.das_voxel_transform, points_of(frame))
    for box in (None, BOX):
        counts, rows, _ = run(grid, [frame], 0.0, A, box=box)
        expected, numbers = binned_records(grid.output_points, 1, 0.0, A, box=box)
        same(counts, expected)
        check_rows(rows, numbers, [frame], 0.0, box=box)
        assert box is not None or numbers[0]["found"] >= 4              # (the box holds no peak: the map stays empty, the rows say so)


def test_offsets_one_placement_or_one_a_frame_and_a_translation_of_one_frame(bflib):
    acq = block("B")
    frames, _ = variants_push("B")
    grid = map_view(finer(vc.POINTS), vc.LO, vc.HI)
    A = placement_onto(grid, acq.bp.das_voxel_transform, vc.POINTS)
    thresholds = fraction_of_max(frames, 0.25)
    with_offsets, _, _ = run(grid, frames, thresholds, A, use_offsets=True)
    without, _, _ = run(grid, frames, thresholds, A, use_offsets=False)
    same(with_offsets, ref.accumulate(grid.output_points, frames, thresholds, A, use_offsets=True)[0])
    same(without, ref.accumulate(grid.output_points, frames, thresholds, A, use_offsets=False)[0])
    assert with_offsets.tobytes() != without.tobytes()
    # without offsets every deposit lies on a coarse voxel
    assert int(without.sum()) == int(without[::4, :, ::4].sum())
    # one placement for all frames is that placement once a frame
    repeated, _, _ = run(grid, frames, thresholds, np.stack([A, A, A]))
    same(repeated, with_offsets)
    # the newest frame moved by (+3, 0, -2) bins: only its deposits move
    moved = A.copy()
    moved[:, 3] += (3.0, 0.0, -2.0)
    mixed, rows, _ = run(grid, frames, thresholds, np.stack([A, A, moved]))
    expected, numbers = ref.accumulate(grid.output_points, frames, thresholds, np.stack([A, A, moved]))
    same(mixed, expected)
    check_rows(rows, numbers, frames, thresholds)
    alone, _, _ = run(grid, frames[2:], thresholds[2], A)
    alone_moved, _, _ = run(grid, frames[2:], thresholds[2], moved)
    assert alone.tobytes() != alone_moved.tobytes()
    assert np.array_equal(mixed.astype(np.int64) - with_offsets, alone_moved.astype(np.int64) - alone)


def test_peaks_outside_the_map_are_counted_and_nothing_is_written(bflib):
    acq = block("B")
    frames, _ = variants_push("B")
    grid = map_view(finer(vc.POINTS), vc.LO, vc.HI)
    A = placement_onto(grid, acq.bp.das_voxel_transform, vc.POINTS)
    thresholds = fraction_of_max(frames, 0.1)
    # the map's origin moved to the middle of the frames: what lies left of it or above it is outside
    shifted = A.copy()
    shifted[:, 3] -= (46.0, 0.0, 78.0)
    counts, rows, info = run(grid, frames, thresholds, shifted)
    expected, numbers = ref.accumulate(grid.output_points, frames, thresholds, shifted)
    same(counts, expected)
    check_rows(rows, numbers, frames, thresholds)
    outside, found = sum(n["outside"] for n in numbers), sum(n["found"] for n in numbers)
    print(f"  {outside} of {found} peaks outside")
    assert 0 < outside < found and (int(info.deposited), int(info.outside)) == (found - outside, outside)
    assert all(0 < n["outside"] < n["found"] for n in numbers)
    # half a bin short of the first bin on y: every peak outside, on one axis only
    below = A.copy()
    below[1, 3] = -0.5000001
    # a coordinate that overflows: every peak outside, the map untouched
    beyond = A.copy()
    beyond[0, 0], beyond[0, 3] = 1e308, 1e308
    for placement in (below, beyond):
        counts, rows, info = run(grid, frames, thresholds, placement)
        assert not counts.any() and int(info.deposited) == 0 and int(info.outside) == found
        assert all(r.outside == r.found and r.deposited == 0 for r in rows)
    # a map smaller than its buffer (the buffer of the larger map above is kept): the counts behind it stay as they were
    small = map_view((5, 1, 7), vc.LO, vc.HI)
    Asmall = placement_onto(small, acq.bp.das_voxel_transform, vc.POINTS)
    counts, rows, _ = run(small, frames, thresholds, Asmall)
    same(counts, ref.accumulate(small.output_points, frames, thresholds, Asmall)[0])
    assert int(counts.sum()) == found


def test_every_peak_of_eight_frames_in_one_bin(bflib):
    frames = np.concatenate([variants_push("A")[0] for _ in range(3)])[1:]
    assert len(frames) == 8
    grid = map_view((1, 1, 1), vc.LO, vc.HI)
    counts, rows, info = run(grid, list(frames), 0.0, np.zeros((3, 4)))
    found, _, _ = bf.find_peaks_last_frames(8, 0.0, 16)
    total = sum(int(r.found) for r in found)
    print(f"  {total} peaks of 8 frames into one bin")
    assert total >= 64 and counts.shape == (1, 1, 1) and int(counts[0, 0, 0]) == total == int(info.deposited)
    assert [int(r.deposited) for r in rows] == [int(r.found) for r in found] and not any(r.outside for r in rows)


def test_boxes_that_tile_a_frame_give_the_frames_map_and_calls_add_up(bflib):
    acq = block("forces")
    frame = bflib.beamform(acq.bp, acq.rf, acq.filters).copy()
    grid = map_view(finer(points_of(frame)), vc.LO3, vc.HI3)
    A = placement_onto(grid, acq.bp.das_voxel_transform, points_of(frame))
    threshold = fraction_of_max([frame], 0.05)[0]
    whole, rows, _ = run(grid, [frame], threshold, A)
    assert rows[0].found >= 4
    first = True
    for z in (0, 16):
        for y in (0, 8):
            for x in (0, 8):
                tiled, _, info = run(grid, [frame], threshold, A, box=((x, y, z), (8, 8, 16)), reset=first)
                first = False
    same(tiled, whole)
    assert (info.calls, int(info.deposited)) == (8, int(rows[0].found))
    # two identical calls: exactly twice the counts; a reset: zeros
    run(grid, [frame], threshold, A)
    twice, _, info = run(grid, [frame], threshold, A, reset=False)
    same(twice, whole * np.uint32(2))
    assert (info.calls, int(info.deposited)) == (2, 2 * int(rows[0].found))
    bf.localisation_map_reset(grid.output_points)
    zeros, info = bf.localisation_map_copy()
    assert not zeros.any() and (info.calls, int(info.deposited), int(info.outside)) == (0, 0, 0)


def test_a_views_push_frames_of_different_grids_each_with_its_placement(bflib):
    acq = block("B")
    grids = [(150, 1, 9), (64, 1, 5), (63, 2, 3), (1, 1, 40), (65, 1, 1)]
    views = [bflib.view(points, vc.LO, vc.HI) for points in grids]
    frames = bflib.beamform_views(acq.bp, acq.rf, views, acq.filters)
    assert all(f.dtype == np.float32 for f in frames)
    grid = bf.view((97, 3, 65), (vc.LO[0], -1e-3, vc.LO[2]), (vc.HI[0], 1e-3, vc.HI[2]))
    placements = np.stack([placement_onto(grid, v.das_voxel_transform, v.output_points) for v in views])
    counts, rows, _ = run(grid, frames, 0.0, placements)
    expected, numbers = ref.accumulate(grid.output_points, frames, 0.0, placements)
    same(counts, expected)
    check_rows(rows, numbers, frames, 0.0)
    assert [tuple(r.points) for r in rows] == grids and all(n["found"] >= 1 for n in numbers)
    # the frames' plane y = 0 is the map's middle plane; every view contributed inside the map
    assert not counts[:, 0].any() and not counts[:, 2].any() and all(n["deposited"] >= 1 for n in numbers)


def test_the_queued_frame(bflib):
    L = bflib.library()
    acq = block("B")
    frames, ids = variants_push("B")
    grid = map_view(finer(vc.POINTS), vc.LO, vc.HI)
    A = placement_onto(grid, acq.bp.das_voxel_transform, vc.POINTS)
    thresholds = fraction_of_max(frames, 0.1)
    # the same frames three times, the third time without offsets: bins of several different counts
    run(grid, frames, thresholds, A)
    run(grid, frames, thresholds, A, reset=False)
    counts, _, _ = run(grid, frames, thresholds, A, use_offsets=False, reset=False)
    assert len(np.unique(counts)) >= 3
    scale = 0.37
    frame_id, ms = bf.queue_localisation_map(scale, tag=5)
    assert frame_id == ids[2] + 1 and ms > 0
    info = bf.frame_info(frame_id)
    assert tuple(info.points) == tuple(grid.output_points) and info.data_kind == int(P.DataKind.Float32) and info.frame_id == frame_id
    assert int(newest_info(L).frame_id) == frame_id
    queued = bf.copy_frame(frame_id)
    expected = ref.queued_frame(counts, scale)
    assert queued.dtype == np.float32 and np.array_equal(queued.view(np.uint32), expected.view(np.uint32))
    # the map itself is as it was
    same(bf.localisation_map_copy()[0], counts)
    # the frame operations take it: metrics, peaks, the Gaussian that renders it, the display
    metrics, _ = bf.score_last_frames(1)
    assert metrics[0].frame_id == frame_id and metrics[0].image_plane_tag == 5 and metrics[0].parameter_block == bf.frame_info(ids[2]).parameter_block
    assert metrics[0].max_abs == expected.max() and int(metrics[0].voxels) == expected.size
    rows, peaks, _ = bf.find_peaks_last_frames(1, 0.5 * scale, 4096)
    want = frame_peaks_ref.peaks(queued, 0.5 * scale)
    assert int(rows[0].found) == want["found"] >= 8
    assert np.array_equal(np.frombuffer(bytes(peaks), np.dtype(P.HipFramePeak))["index"], want["index"])
    # the variants push is still the newest multi-frame push behind it
    assert int(bf.last_variants_info().first_frame_id) == ids[0]
    gauss = np.exp(-0.5 * (np.arange(-4, 5) / 1.5) ** 2).astype(np.float32)
    smooth_id, _ = bf.convolve_last_frames(1, [gauss, None, gauss])
    assert smooth_id == frame_id + 1
    smooth = bf.copy_frame(smooth_id)
    assert smooth.shape == queued.shape and np.isfinite(smooth).all() and smooth.max() > 0
    assert int(bf.last_variants_info().first_frame_id) == ids[0]
    # a second frame of the same map, without a synchronise: another id, another scale
    again, ms = bf.queue_localisation_map(2.0, tag=6, timed=False)
    assert again == smooth_id + 1 and ms == 0.0
    assert np.array_equal(bf.copy_frame(again).view(np.uint32), ref.queued_frame(counts, 2.0).view(np.uint32))
    assert bf.score_last_frames(1)[0][0].image_plane_tag == 6


def test_refusals_on_the_device_change_nothing(bflib):
    L = bflib.library()
    acq = block("B")
    frames, ids = variants_push("B")
    grid = map_view(finer(vc.POINTS), vc.LO, vc.HI)
    A = placement_onto(grid, acq.bp.das_voxel_transform, vc.POINTS)
    thresholds = fraction_of_max(frames, 0.25)
    counts, _, _ = run(grid, frames, thresholds, A)

    def state():
        c, info = bf.localisation_map_copy()
        return c.tobytes(), bytes(info), bytes(newest_info(L))

    before = state()
    rows = (P.HipMapDeposits * 4)()
    C.memset(rows, 0xA5, C.sizeof(rows))
    untouched = bytes(rows)
    ms, frame = C.c_float(-1.0), C.c_uint32(77)
    level = (C.c_float * 1)(0.0)

    def refused(kind, count=3, region=None, placements=A, placement_count=1):
        pointer = np.ascontiguousarray(placements, np.float64).ctypes.data_as(C.POINTER(C.c_double))
        assert not L.beamformer_hip_accumulate_peaks_last_frames(count, None if region is None else C.byref(region), level, 1, pointer,
                                                                 placement_count, 1, rows, C.byref(ms))
        assert bf.last_error()[0] == kind and bytes(rows) == untouched and ms.value == -1.0 and state() == before

    refused(E.InvalidAccess, region=bf.frame_region((20, 0, 0), (8, 1, 9)))              # a box past the grid
    refused(E.InvalidAccess, region=bf.frame_region((0, 0, 0), (7, 0, 9)))
    queued = int(newest_info(L).frame_id) + 1
    if queued < P.HIP_MAX_SCORED_FRAMES:
        refused(E.InvalidAccess, count=queued + 1)                                       # more frames than were ever queued
    refused(E.InvalidAccess, placement_count=2, placements=np.stack([A, A]))
    broken = A.copy()
    broken[2, 1] = np.nan
    refused(E.InvalidAccess, placements=broken)
    refused(E.BufferOverflow, count=0)
    # the map's own calls
    out = (C.c_uint32 * 16)(*([9] * 16))
    assert not L.beamformer_hip_localisation_map_copy(out, counts.size - 1, None) and bf.last_error()[0] == E.ExportSpaceOverflow and list(out) == [9] * 16
    assert not L.beamformer_hip_localisation_map_reset((C.c_uint32 * 3)(4, 0, 4)) and bf.last_error()[0] == E.InvalidAccess
    assert not L.beamformer_hip_localisation_map_reset((C.c_uint32 * 3)(1 << 10, 1 << 10, 1 << 10)) and bf.last_error()[0] == E.BufferOverflow
    assert not L.beamformer_hip_queue_localisation_map(float("inf"), 0, C.byref(frame), C.byref(ms)) and bf.last_error()[0] == E.InvalidAccess
    assert frame.value == 77 and ms.value == -1.0 and state() == before
    # a map that has not been deposited into since its reset is not queued
    bf.localisation_map_reset(grid.output_points)
    newest = bytes(newest_info(L))
    assert not L.beamformer_hip_queue_localisation_map(1.0, 0, C.byref(frame), C.byref(ms)) and bf.last_error()[0] == E.InvalidAccess
    assert frame.value == 77 and ms.value == -1.0 and bytes(newest_info(L)) == newest
    # no map: released
    bf.localisation_map_reset(None)
    assert not L.beamformer_hip_accumulate_peaks_last_frames(3, None, level, 1, A.ctypes.data_as(C.POINTER(C.c_double)), 1, 1, rows, C.byref(ms))
    assert bf.last_error()[0] == E.InvalidAccess and bytes(rows) == untouched and bytes(newest_info(L)) == newest
    assert not L.beamformer_hip_localisation_map_copy(out, 16, None) and bf.last_error()[0] == E.InvalidAccess
    assert not L.beamformer_hip_queue_localisation_map(1.0, 0, C.byref(frame), None) and bf.last_error()[0] == E.InvalidAccess
    # a tombstone among the frames (a variants push that fails at its DAS stage, without any device fault)
    bf.localisation_map_reset(grid.output_points)
    rf = np.ascontiguousarray(acq.rf)
    array = (P.HipDasVariant * 3)(*vc.candidates(acq.bp))
    L.beamformer_hip_set_das_path(P.HIP_DAS_PATH_FAIL_VIEWS_DAS)
    assert not L.beamformer_hip_push_data_variants_with_compute(rf.ctypes.data_as(C.c_void_p), rf.nbytes, array, 3, 0, 0)
    L.beamformer_hip_set_das_path(0)
    assert not L.beamformer_hip_accumulate_peaks_last_frames(1, None, level, 1, A.ctypes.data_as(C.POINTER(C.c_double)), 1, 1, rows, C.byref(ms))
    assert bf.last_error()[0] == E.InvalidAccess and bytes(rows) == untouched
    zeros, info = bf.localisation_map_copy()
    assert not zeros.any() and info.calls == 0


def test_the_ring_a_queued_map_that_wraps_and_one_that_does_not_fit():
    """a 1 MiB frame ring in a process of its own (the ring is sized once per process): tests/localisation_wrap_worker.py"""
    run_ring_worker("localisation_wrap_worker", 1 << 20, expect=("refused", "wrapped"))
