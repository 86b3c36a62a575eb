"""Frame peaks on the device (beamformer_hip_find_peaks_last_frames; csrc/frame_peaks.hip).  Frames are produced by ordinary pushes and
downloaded with beamformer_get_last_frames; the expected lists are the numpy reference (tests/frame_peaks_ref.py) applied to those
downloaded arrays -- parity of the frames themselves is other tests' business, except in the loop at the end.

The bars are derived, not measured.  Every decision is taken on q = re * re + im * im (or |v|), formed by the same IEEE operations in the
same order on the device and in numpy: found, above_threshold, stored, first, every index and every fitted bit are asked exactly.  On
real frames the magnitudes are q itself and the offset is three float32 operations in a fixed order with a correctly rounded division:
bit-equal.  On complex frames the magnitude is sqrtf(q): within 1 ulp (DESIGN 3.7a expects bit-equal, the square root being correctly
rounded; the test prints how many are).  An offset 0.5 (a - b) / den formed from magnitudes that are each 1 ulp (2^-23 relative, at most
2^-23 m0 as m0 is the largest of the three) off: the numerator moves by at most 2 x 2^-23 m0 / 2, the denominator by at most
4 x 2^-23 m0, the quotient -- at most 1/2 in magnitude before clamping -- by at most (1 + 2) x 2^-23 m0 / |den| to first order; with the
roundings of the three operations and the second-order term the bar is 8 x 2^-23 m0 / |den| + 2^-20."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

from ogl_beamforming_amd import configs as cfg
from ogl_beamforming_amd import params as P
from tests import cases
from tests import frame_peaks_ref as ref
from tests import variants_cases as vc
from tests.das_push import compare
from tests.parity import reference
from tests.frame_info import newest_info
from tests.ring_frames import (metrics_block as block, BOX, CAP, check_peaks as check_call, fraction_of_max, peak_records as records_of, region_of,
                               variants_push)
from tests.scaffold import automatic_path  # noqa: F401

pytestmark = pytest.mark.gpu
E = P.LibError


def test_block_a_three_variants_of_a_complex_plane(bflib):
    frames, ids = variants_push("A")
    thresholds = fraction_of_max(frames, 0.25)
    rows, peaks, expected = check_call(frames, thresholds, what="A, a threshold each")
    assert [int(r.frame_id) for r in rows] == ids
    assert all(r["found"] >= 8 for r in expected) and all(r["above_threshold"] < frames[0].size for r in expected)
    # the three lists differ: a kernel that reads one frame for every row fails above
    assert not np.array_equal(expected[0]["index"], expected[1]["index"]) and not np.array_equal(expected[1]["index"], expected[2]["index"])
    # one threshold for all three: the middle frame's
    check_call(frames, thresholds[1], what="A, one threshold")
    check_call(frames, thresholds, box=((5, 0, 7), (11, 1, 21)), what="A, box")


def test_block_b_real_frames(bflib):
    frames, ids = variants_push("B")
    assert frames.dtype == np.float32
    thresholds = fraction_of_max(frames, 0.25)
    rows, peaks, expected = check_call(frames, thresholds, what="B")
    assert all(r["found"] >= 8 for r in expected) and any((r["fitted"] == 5).any() for r in expected)
    check_call(frames, 0.0, what="B, threshold 0")
    check_call(frames, thresholds, box=((5, 0, 7), (11, 1, 21)), what="B, box")


def test_block_d3_a_volume_with_nan_and_a_box_judged_by_the_frames_neighbours(bflib):
    acq = block("D3")
    frame = bflib.beamform(acq.bp, acq.rf, acq.filters).copy()
    nan = int(np.isnan(frame).sum())
    threshold = fraction_of_max([frame], 0.25)[0]
    inside, clipped = ref.peaks(frame, threshold, *BOX), ref.peaks(frame, threshold, *BOX, clip_to_box=True)
    print(f"  D3: {nan} NaN voxels; box {BOX}: {inside['found']} peaks, {clipped['found']} with the neighbourhood clipped to the box")
    # the case has teeth: a kernel that clipped the neighbourhood to the box would give another list
    assert nan >= 64 and not np.array_equal(inside["index"], clipped["index"])
    check_call([frame], threshold, box=BOX, what="D3 box")
    _, _, whole = check_call([frame], threshold, what="D3")
    assert whole[0]["found"] >= 4
    check_call([frame], 0.0, what="D3, threshold 0")
    # tiling: the peaks of the eight octants together are the frame's, none invented, none doubled
    tiled = []
    for z in (0, 16):
        for y in (0, 8):
            for x in (0, 8):
                rows, peaks, _ = check_call([frame], threshold, box=((x, y, z), (8, 8, 16)), what=f"D3 octant {x, y, z}")
                tiled += [tuple(int(v) for v in i) for i in records_of(rows[0], peaks)["index"]]
    assert sorted(tiled) == sorted(tuple(int(v) for v in i) for i in whole[0]["index"])


def test_block_d_rows_shorter_than_a_wave(bflib):
    acq = block("D")
    frame = bflib.beamform(acq.bp, acq.rf, acq.filters).copy()
    assert frame.shape == (40, 1, 24) and int(np.isnan(frame).sum()) >= 64
    for fraction in (0.0, 0.1, 0.25):
        _, _, expected = check_call([frame], fraction_of_max([frame], fraction)[0], what=f"D at {fraction}")
        assert expected[0]["found"] >= 8


def test_a_views_push_of_rows_across_a_wave_exactly_a_wave_and_one_past_it(bflib):
    acq = block("A")
    grids = [(150, 1, 9), (64, 1, 5), (63, 2, 3), (1, 1, 40), (65, 1, 1)]
    views = [bflib.view(points, vc.LO, vc.HI) for points in grids]
    frames = bflib.beamform_views(acq.bp, acq.rf, views, acq.filters)
    rows, peaks, expected = check_call(frames, 0.0, what="views")
    assert [tuple(r.points) for r in rows] == grids
    assert all(r["found"] >= 1 for r in expected) and expected[0]["found"] >= 8
    # peaks lie on both sides of a wave's last lane in the rows that cross one
    for k in (0, 4):
        x = expected[k]["index"][:, 0]
        assert (x < 64).any() and (x >= 64).any(), k
    # and a positive threshold, one a frame
    check_call(frames, fraction_of_max(frames, 0.3), what="views, 0.3 of each maximum")


@functools.lru_cache(maxsize=None)
def tall_volume():
    """3 x 65 x 64: rows of three voxels, 4160 waves in 1040 blocks -- one more round of 1024 blocks for the scan than any frame above"""
    return cfg.rca("frame_peaks_tall", 16, 8, 256, (3, 65, 64), vc.LO3, vc.HI3, seed=7401, orientation=0x12, demodulate=False,
                   data_kind=P.DataKind.Float32Complex, angles=np.linspace(-8, 8, 8))


def test_a_frame_of_more_than_1024_blocks(bflib):
    acq = tall_volume()
    frame = bflib.beamform(acq.bp, acq.rf, acq.filters).copy()
    assert frame.shape == (64, 65, 3)
    _, _, expected = check_call([frame], 0.0, what="tall")
    # peaks lie in the blocks of the scan's second round (waves from 4096: z = 63, y >= 1), and several before them
    z, y = expected[0]["index"][:, 2], expected[0]["index"][:, 1]
    assert ((z == 63) & (y >= 2)).any() and (z < 63).sum() >= 8
    check_call([frame], fraction_of_max([frame], 0.25)[0], what="tall, 0.25 of the maximum")
    check_call([frame], 0.0, cap=int(expected[0]["found"]) - 1, what="tall, the last peak cut off")


def test_the_cap_keeps_the_first_records_in_flat_order(bflib):
    frames, ids = variants_push("A")
    thresholds = fraction_of_max(frames, 0.25)
    full_rows, full_peaks, _ = check_call(frames, thresholds, what="uncapped")
    rows, peaks, _ = check_call(frames, thresholds, cap=5, what="cap 5")
    assert len(peaks) == 15
    for k in range(3):
        assert full_rows[k].found > 5 and rows[k].found == full_rows[k].found and rows[k].above_threshold == full_rows[k].above_threshold
        assert rows[k].stored == 5 and rows[k].first == 5 * k
        assert records_of(rows[k], peaks).tobytes() == records_of(full_rows[k], full_peaks)[:5].tobytes()
    # the caller's buffer behind the stored records is left alone
    L = bflib.library()
    out = (P.HipFramePeak * 15)()
    C.memset(out, 0x5A, C.sizeof(out))
    frames_out, total = (P.HipFramePeaks * 3)(), C.c_uint32(0)
    levels = (C.c_float * 3)(*thresholds)
    assert L.beamformer_hip_find_peaks_last_frames(3, None, levels, 3, 2, frames_out, out, C.byref(total), None), bflib.last_error()
    assert total.value == 6 and bytes(out)[6 * 32:] == b"\x5A" * (9 * 32)
    assert bytes(out)[:2 * 32] == records_of(full_rows[0], full_peaks)[:2].tobytes()
    assert bytes(out)[4 * 32:6 * 32] == records_of(full_rows[2], full_peaks)[:2].tobytes()


def test_a_frame_of_zeros_has_one_peak_at_the_origin(bflib):
    acq = block("B")
    frame = bflib.beamform(acq.bp, np.zeros_like(acq.rf), acq.filters).copy()
    assert frame.dtype == np.float32 and not frame.any()
    rows, peaks, _ = check_call([frame], 0.0, what="zeros")
    assert rows[0].found == 1 and rows[0].above_threshold == frame.size and tuple(peaks[0].index) == (0, 0, 0)
    assert peaks[0].fitted == 0 and peaks[0].magnitude == 0.0 and not any(peaks[0].offset)
    rows, peaks, _ = check_call([frame], 0.0, box=((1, 0, 0), (23, 1, 40)), what="zeros, off the origin")
    assert rows[0].found == 0 and rows[0].stored == 0 and len(peaks) == 0 and rows[0].above_threshold == 23 * 40
    rows, peaks, _ = check_call([frame], 1e-30, what="zeros, a positive threshold")
    assert rows[0].found == 0 and rows[0].above_threshold == 0


def test_a_frames_list_depends_on_that_frame_the_box_and_the_threshold_only(bflib):
    frames, ids = variants_push("A")
    thresholds = fraction_of_max(frames, 0.25)
    size = C.sizeof(P.HipFramePeaks)
    for box in (None, ((5, 0, 7), (11, 1, 21))):
        region = region_of(box)
        three, three_peaks, _ = bflib.find_peaks_last_frames(3, thresholds, CAP, region)
        again, again_peaks, _ = bflib.find_peaks_last_frames(3, thresholds, CAP, region)
        assert bytes(three) == bytes(again) and bytes(three_peaks) == bytes(again_peaks) and len(three_peaks) >= 8
        one, one_peaks, _ = bflib.find_peaks_last_frames(1, thresholds[2], CAP, region)
        assert one[0].first == 0 and three[2].first == three[0].stored + three[1].stored
        alone, inside = bytearray(bytes(one[0])), bytearray(bytes(three)[2 * size:])
        offset = P.HipFramePeaks.first.offset
        alone[offset:offset + 4] = inside[offset:offset + 4] = b"\0\0\0\0"
        assert alone == inside
        assert bytes(one_peaks) == records_of(three[2], three_peaks).tobytes()
        # ... nor on the cap, below it
        capped, capped_peaks, _ = bflib.find_peaks_last_frames(3, thresholds, int(three[0].found), region)
        assert records_of(capped[0], capped_peaks).tobytes() == records_of(three[0], three_peaks).tobytes()


def test_refusals_on_the_device(bflib):
    L = bflib.library()
    acq = block("A")
    views = [bflib.view(points, vc.LO, vc.HI) for points in ((24, 1, 40), (7, 1, 9))]
    bflib.beamform_views(acq.bp, acq.rf, views, acq.filters)
    rows, peaks = (P.HipFramePeaks * 4)(), (P.HipFramePeak * 64)()
    C.memset(rows, 0xA5, C.sizeof(rows))
    C.memset(peaks, 0xA5, C.sizeof(peaks))
    untouched = bytes(rows), bytes(peaks)
    total, ms, level = C.c_uint32(77), C.c_float(-1.0), (C.c_float * 1)(0.0)

    def refused(count, region=None, kind=E.InvalidAccess):
        assert not L.beamformer_hip_find_peaks_last_frames(count, None if region is None else C.byref(region), level, 1, 16, rows, peaks,
                                                           C.byref(total), C.byref(ms))
        assert bflib.last_error()[0] == kind and (bytes(rows), bytes(peaks)) == untouched and total.value == 77 and ms.value == -1.0

    # a box that fits the first view but not the second; a zero count; a box past the grid
    refused(2, bflib.frame_region((0, 0, 0), (8, 1, 9)))
    refused(2, bflib.frame_region((6, 0, 8), (2, 1, 2)))
    refused(1, bflib.frame_region((0, 0, 0), (7, 0, 9)))
    refused(1, bflib.frame_region((0xFFFFFFFF, 0, 0), (2, 1, 1)))
    refused(0, kind=E.BufferOverflow)
    found, _, _ = bflib.find_peaks_last_frames(2, 0.0, 16, bflib.frame_region((0, 0, 0), (7, 1, 9)))
    assert found[0].found >= 1 and found[1].found >= 1
    # more frames than were ever queued
    queued = int(newest_info(L).frame_id) + 1
    if queued < P.HIP_MAX_SCORED_FRAMES:
        refused(queued + 1)
    # a variants push that fails at its DAS stage (das path flag 0x2000) leaves tombstones under its three ids, without any device fault
    rf = np.ascontiguousarray(acq.rf)
    variants = vc.candidates(acq.bp)
    array = (P.HipDasVariant * 3)(*variants)
    L.beamformer_hip_set_das_path(P.HIP_DAS_PATH_FAIL_VIEWS_DAS)
    assert not L.beamformer_hip_push_data_variants_with_compute(rf.ctypes.data_as(C.c_void_p), rf.nbytes, array, 3, 0, 0)
    assert bflib.last_error()[0] == E.InvalidAccess
    L.beamformer_hip_set_das_path(0)
    refused(1)
    refused(4)
    # a good single frame behind the tombstones is served, two frames are not
    frame = bflib.beamform(acq.bp, acq.rf, acq.filters).copy()
    check_call([frame], fraction_of_max([frame], 0.25)[0], what="behind the tombstones")
    refused(2)


# ---- the loop: coarse ensemble -> peaks -> patches -> refined ensemble ----

LOOP_POINTS, LOOP_LO, LOOP_HI = (32, 1, 48), (-2.5e-3, 0.0, 3.0e-3), (2.5e-3, 0.0, 5.5e-3)
SCATTERERS = [(-1.3e-3, 0.0, 3.7e-3), (0.9e-3, 0.0, 4.6e-3), (1.7e-3, 0.0, 3.5e-3)]
PATCH, EXTENT = (17, 1, 17), (4.0, 0.0, 4.0)              # odd patch points; 16 steps over 4 source voxels: 4 x finer


@functools.lru_cache(maxsize=None)
def loop_case():
    """Three isolated point scatterers seen by 16 channels x 2 plane waves of Int16 RF, demodulated: a complex plane with three smooth
    blobs.  Two RF frames: the acquisition's, and the same at 0.75 of the amplitude."""
    acq = cfg.rca("frame_peaks_loop", 16, 2, 256, LOOP_POINTS, LOOP_LO, LOOP_HI, seed=7400, interp=P.InterpolationMode.Linear,
                  angles=np.array([-6.0, 6.0]), scatterers=SCATTERERS, noise=False)
    rf = np.stack([acq.rf, np.rint(acq.rf * 0.75).astype(acq.rf.dtype)])
    return acq, rf


def on_grid(acq, view, rf):
    bp = type(acq.bp).from_buffer_copy(acq.bp)
    bp.das_voxel_transform[:] = list(view.das_voxel_transform)
    bp.output_points[:3] = [int(n) for n in view.output_points]
    return dataclasses.replace(acq, bp=bp, rf=rf)


def strongest_peak_from_centre(frame):
    """the strongest peak of a patch frame: its distance from the patch centre per axis, in SOURCE voxels"""
    q = ref.peaks(frame, 0.0)
    best = int(np.argmax(q["magnitude"]))
    at = q["index"][best].astype(np.float64) + q["offset"][best]
    centre = np.array([(n - 1) / 2 for n in PATCH])
    steps = np.array([EXTENT[a] / max(1, PATCH[a] - 1) for a in range(3)])
    return (at - centre) * steps


def test_the_ulm_loop(bflib, oracle):
    """burst push on a coarse plane -> peaks -> peaks_to_views -> burst views push: every patch frame is the oracle's frame of the block
    with that grid, and the patch's strongest peak lies within 1.5 source voxels of its centre"""
    acq, rf = loop_case()
    coarse = bflib.beamform_burst(acq.bp, rf, acq.filters).copy()
    assert coarse.shape == (2, 48, 1, 32) and np.iscomplexobj(coarse)
    metrics, _ = bflib.score_last_frames(2)
    thresholds = [0.5 * float(m.max_abs) for m in metrics]
    rows, peaks, expected = check_call(list(coarse), thresholds, cap=16, what="coarse")
    assert rows[0].found == rows[1].found == len(SCATTERERS)
    mine = records_of(rows[0], peaks)
    for p, s in zip(sorted(mine, key=lambda p: int(p["index"][0])), sorted(SCATTERERS)):
        x = LOOP_LO[0] + (LOOP_HI[0] - LOOP_LO[0]) * (int(p["index"][0]) + float(p["offset"][0])) / (LOOP_POINTS[0] - 1)
        print(f"  peak at x = {x * 1e3:.3f} mm, scatterer at {s[0] * 1e3:.3f} mm")
        assert abs(x - s[0]) < 1.5 * (LOOP_HI[0] - LOOP_LO[0]) / (LOOP_POINTS[0] - 1)
    first = [peaks[int(rows[0].first) + k] for k in range(int(rows[0].stored))]
    views = bflib.peaks_to_views(list(acq.bp.das_voxel_transform), LOOP_POINTS, first, PATCH, EXTENT, use_offsets=True)
    # the oracle first, on the CPU: its own patch frames meet the condition
    refs = [[(on_grid(acq, v, rf[k]),) + tuple(reference(oracle, on_grid(acq, v, rf[k]))) for k in range(2)] for v in views]
    for v in range(len(views)):
        for k in range(2):
            away = strongest_peak_from_centre(refs[v][k][1])
            print(f"  oracle patch {v} frame {k}: strongest peak {away} source voxels from the centre")
            assert np.abs(away).max() <= 1.5
    patches = bflib.beamform_burst_views(acq.bp, rf, views, acq.filters)
    tol = cases.tolerance(acq)
    for v in range(len(views)):
        for k in range(2):
            acq_v, expected_frame, _, flags = refs[v][k]
            verdict = compare(patches[v][k], expected_frame, acq_v, flags, label=f"frame_peaks_loop/patch {v}/{k}")
            away = strongest_peak_from_centre(patches[v][k])
            print(f"  patch {v} frame {k}: max_rel_err {verdict.max_rel_err:.3e} (tolerance {tol}); strongest peak {away} source voxels from the centre")
            assert np.abs(away).max() <= 1.5
