"""Frame metrics on the device (beamformer_hip_score_last_frames, beamformer_hip_copy_frame, beamformer_hip_get_frame_info; csrc/
frame_metrics.hip).  Frames are produced by ordinary pushes and downloaded with beamformer_get_last_frames; the expected rows are the
numpy reference (tests/frame_metrics_ref.py) applied to those downloaded arrays -- parity of the frames themselves is other tests'
business.

The bars are derived, not measured.  A float32 magnitude formed by two roundings and a square root is within 2 ulp of numpy's, 2.4e-7
relative; the terms are non-negative, so a sum inherits that bound times the power (1e-6 / 2e-6 / 4e-6 for |v|, |v|^2, |v|^4), the double
accumulation adding about n x 2^-53.  The perturbation of a sum G of (a - b)^2 under magnitude errors of eps |v| is at most
2 sqrt(G) sqrt(sum of (da + db)^2); a voxel sits in at most two pairs of an axis, so that is at most 4 eps sqrt(G S2), about
1e-6 sqrt(G S2): the bar is twice that, plus 1e-12 S2.  On real frames fabsf is exact and only the order of the double additions differs:
1e-12 relative.  Every test prints what it measured before it asserts."""
import ctypes as C

import numpy as np
import pytest

from ogl_beamforming_amd import params as P
from tests import frame_metrics_ref as ref
from tests import variants_cases as vc
from tests.frame_info import newest_info
from tests.ring_frames import BOX, metrics_block as block, check_row, region_of, variants_push
from tests.scaffold import automatic_path, run_ring_worker, two_contexts_on_device_0  # noqa: F401

pytestmark = pytest.mark.gpu
E = P.LibError
S = P.FrameScore


def test_block_a_three_variants_of_a_complex_plane(bflib):
    frames, ids = variants_push("A")
    rows, ms = bflib.score_last_frames(3)
    assert [int(r.frame_id) for r in rows] == ids and ms > 0
    expected = [check_row(rows[k], frames[k], what=f"A variant {k}") for k in range(3)]
    # the three frames are far more than any tolerance apart: a kernel that reads the wrong frame, or one frame for every row, fails above
    sharpness = [ref.score(r, S.Sharpness) for r in expected]
    print("  sharpness", sharpness, "sum_abs2", [r["sum_abs2"] for r in expected], "argmax", [r["max_index"] for r in expected])
    for a in range(3):
        for b in range(a + 1, 3):
            assert abs(expected[a]["sum_abs2"] - expected[b]["sum_abs2"]) > 1e-3 * expected[a]["sum_abs2"]
            assert expected[a]["max_index"] != expected[b]["max_index"]


def test_block_b_real_frames(bflib):
    frames, ids = variants_push("B")
    assert frames.dtype == np.float32
    rows, _ = bflib.score_last_frames(3)
    for k in range(3):
        check_row(rows[k], frames[k], what=f"B variant {k}")
    rows, _ = bflib.score_last_frames(3, region_of(((5, 0, 7), (11, 1, 21))))
    for k in range(3):
        check_row(rows[k], frames[k], ((5, 0, 7), (11, 1, 21)), what=f"B variant {k}, box")


@pytest.mark.parametrize("box", [None, BOX], ids=["whole", "box"])
def test_block_c_a_volume_of_several_blocks(box, bflib):
    frames, ids = variants_push("C")
    assert frames.shape[1:] == (32, 16, 16)
    rows, _ = bflib.score_last_frames(3, region_of(box))
    assert [int(r.frame_id) for r in rows] == ids
    for k in range(3):
        check_row(rows[k], frames[k], box, what=f"C variant {k}")


@pytest.mark.parametrize("which", ["D", "D3"])
def test_block_d_frames_with_nan_voxels(which, bflib):
    acq = block(which)
    frame = bflib.beamform(acq.bp, acq.rf, acq.filters).copy()
    nan, finite = int(np.isnan(frame).sum()), int(np.isfinite(np.abs(frame)).sum())
    print(f"  {which}: {nan} NaN voxels, {finite} finite of {frame.size}")
    assert nan >= 64 and 4 * finite >= frame.size
    rows, _ = bflib.score_last_frames(1)
    r = check_row(rows[0], frame, what=which)
    assert r["non_finite"] >= nan
    if which == "D3":
        rows, _ = bflib.score_last_frames(1, region_of(BOX))
        check_row(rows[0], frame, BOX, what=which + " box")


def test_block_e_a_views_push_of_three_sizes(bflib):
    L = bflib.library()
    acq = block("A")
    views = [bflib.view(points, vc.LO, vc.HI, tag=tag) for points, tag in (((24, 1, 40), 0), ((7, 1, 9), 3), ((1, 1, 1), 2))]
    frames = bflib.beamform_views(acq.bp, acq.rf, views, acq.filters)
    rows, _ = bflib.score_last_frames(3)
    assert [tuple(r.points) for r in rows] == [(24, 1, 40), (7, 1, 9), (1, 1, 1)] and [int(r.image_plane_tag) for r in rows] == [0, 3, 2]
    for k in range(3):
        check_row(rows[k], frames[k], what=f"E view {k}")
    assert rows[2].voxels + rows[2].non_finite == 1 and list(rows[2].gradient_pairs) == [0, 0, 0]
    # a region that fits the first view but not the third: InvalidAccess, and out is untouched
    out = (P.HipFrameMetrics * 3)()
    C.memset(out, 0xA5, C.sizeof(out))
    untouched = bytes(out)
    ms = C.c_float(-1.0)
    assert not L.beamformer_hip_score_last_frames(3, C.byref(bflib.frame_region((0, 0, 0), (2, 1, 2))), out, C.byref(ms))
    assert bflib.last_error()[0] == E.InvalidAccess and bytes(out) == untouched and ms.value == -1.0
    # the 1 x 1 x 1 box at the origin fits all three
    rows, _ = bflib.score_last_frames(3, bflib.frame_region((0, 0, 0), (1, 1, 1)))
    for k in range(3):
        check_row(rows[k], frames[k], ((0, 0, 0), (1, 1, 1)), what=f"E view {k}, one voxel")


def test_a_rows_bits_depend_on_its_frame_and_the_region_only(bflib):
    variants_push("C")
    for box in (None, BOX):
        region = region_of(box)
        three, _ = bflib.score_last_frames(3, region)
        again, _ = bflib.score_last_frames(3, region)
        one, _ = bflib.score_last_frames(1, region)
        two, _ = bflib.score_last_frames(2, region)
        assert bytes(three) == bytes(again)
        assert bytes(one[0]) == bytes(three[2])
        assert bytes(two) == bytes(three)[C.sizeof(P.HipFrameMetrics):]
    # no region is the explicit whole-frame box, byte for byte
    whole, _ = bflib.score_last_frames(3, bflib.frame_region((0, 0, 0), (16, 16, 32)))
    none, _ = bflib.score_last_frames(3)
    assert bytes(whole) == bytes(none)


def test_edge_regions(bflib):
    frames, ids = variants_push("C")
    frame = frames[2]
    # one voxel, the last one of the frame
    box = ((15, 15, 31), (1, 1, 1))
    rows, _ = bflib.score_last_frames(1, region_of(box))
    r = check_row(rows[0], frame, box, what="one voxel")
    assert rows[0].voxels == 1 and list(rows[0].gradient_pairs) == [0, 0, 0] and list(rows[0].gradient2) == [0.0, 0.0, 0.0]
    assert tuple(rows[0].max_index) == (15, 15, 31) and r["max_index"] == (15, 15, 31)
    # one plane along each axis: that axis has no pairs, the others do
    for axis in range(3):
        first, count = [2, 3, 4], [9, 8, 7]
        count[axis] = 1
        rows, _ = bflib.score_last_frames(1, region_of((first, count)))
        check_row(rows[0], frame, (first, count), what=f"one plane across axis {axis}")
        pairs = [int(n) for n in rows[0].gradient_pairs]
        assert pairs[axis] == 0 and rows[0].gradient2[axis] == 0.0 and all(pairs[a] > 0 for a in range(3) if a != axis)


def test_two_single_pushes_of_different_kinds_and_grids(bflib):
    a, forces = block("A"), block("forces")
    frame_a = bflib.beamform(a.bp, a.rf, a.filters).copy()
    frame_f = bflib.beamform(forces.bp, forces.rf, forces.filters).copy()
    assert np.iscomplexobj(frame_a) and frame_a.shape == (40, 1, 24) and frame_f.dtype == np.float32 and frame_f.shape == (32, 16, 16)
    rows, _ = bflib.score_last_frames(2)
    assert rows[1].frame_id == rows[0].frame_id + 1
    check_row(rows[0], frame_a, what="single push, complex plane")
    check_row(rows[1], frame_f, what="single push, real volume")


def test_refusals(bflib):
    L = bflib.library()
    acq = block("A")
    variants = vc.candidates(acq.bp)
    good = bflib.beamform_variants(acq.bp, acq.rf, variants, acq.filters).copy()
    last_good = int(newest_info(L).frame_id)
    rf = np.ascontiguousarray(acq.rf)
    array = (P.HipDasVariant * 3)(*variants)
    out = (P.HipFrameMetrics * 8)()
    C.memset(out, 0x5A, C.sizeof(out))
    untouched = bytes(out)

    def refused(count, region=None, kind=E.InvalidAccess):
        assert not L.beamformer_hip_score_last_frames(count, None if region is None else C.byref(region), out, None)
        assert bflib.last_error()[0] == kind and bytes(out) == untouched

    refused(0, kind=E.BufferOverflow)
    refused(P.HIP_MAX_SCORED_FRAMES + 1, kind=E.BufferOverflow)
    assert not L.beamformer_hip_score_last_frames(1, None, None, None) and bflib.last_error()[0] == E.InvalidAccess
    # a zero count in a region, a region past the grid
    refused(1, bflib.frame_region((0, 0, 0), (24, 0, 40)))
    refused(1, bflib.frame_region((0, 0, 0), (25, 1, 40)))
    refused(1, bflib.frame_region((1, 0, 0), (24, 1, 40)))
    refused(1, bflib.frame_region((0, 0, 40), (1, 1, 1)))
    refused(1, bflib.frame_region((0xFFFFFFFF, 0, 0), (2, 1, 1)))
    # a variants push that fails at its DAS stage (das path flag 0x2000) leaves tombstones under its three ids, without any device fault
    L.beamformer_hip_set_das_path(P.HIP_DAS_PATH_FAIL_VIEWS_DAS)
    assert not L.beamformer_hip_push_data_variants_with_compute(rf.ctypes.data_as(C.c_void_p), rf.nbytes, array, 3, 0, 0)
    assert bflib.last_error()[0] == E.InvalidAccess
    L.beamformer_hip_set_das_path(0)
    refused(1)
    refused(4)
    raw = np.zeros(good[0].nbytes // 4 + 16, np.float32)
    for dead in (last_good + 1, last_good + 3):
        assert not L.beamformer_hip_copy_frame(dead, raw.ctypes.data_as(C.c_void_p), raw.nbytes) and bflib.last_error()[0] == E.InvalidAccess
        assert not L.beamformer_hip_get_frame_info(dead, C.byref(P.HipFrameInfo())) and bflib.last_error()[0] == E.InvalidAccess
    assert not raw.any()
    assert np.array_equal(bflib.copy_frame(last_good).view(np.uint32), good[2].view(np.uint32))      # the frame before the tombstones is still served
    # a good single frame behind the tombstones
    single = bflib.beamform(acq.bp, acq.rf, acq.filters).copy()
    rows, _ = bflib.score_last_frames(1)
    assert rows[0].frame_id == last_good + 4
    check_row(rows[0], single, what="the single frame behind the tombstones")
    refused(2)
    # more frames than were ever queued (tests/frame_metrics_wrap_worker.py asks the same of a process that has queued three)
    queued = last_good + 5
    if queued < P.HIP_MAX_SCORED_FRAMES:
        refused(queued + 1)


def test_several_devices_are_refused(bflib):
    """with the devices of beamformer_hip_set_devices (the same ordinal twice: how a one-GPU box tests the path) a frame is a set of
    z-slabs: the single push is served, scoring and the by-id calls are InvalidAccess"""
    L = bflib.library()
    acq = block("C")
    with two_contexts_on_device_0(bflib, acq) as frame:
        assert frame.shape == (32, 16, 16)
        out = (P.HipFrameMetrics * 1)()
        untouched = bytes(out)
        assert not L.beamformer_hip_score_last_frames(1, None, out, None) and bflib.last_error()[0] == E.InvalidAccess and bytes(out) == untouched
        newest = int(newest_info(L).frame_id)
        raw = np.zeros(frame.nbytes // 4, np.float32)
        assert not L.beamformer_hip_copy_frame(newest, raw.ctypes.data_as(C.c_void_p), raw.nbytes) and bflib.last_error()[0] == E.InvalidAccess
        assert not L.beamformer_hip_get_frame_info(newest, C.byref(P.HipFrameInfo())) and bflib.last_error()[0] == E.InvalidAccess
        assert not raw.any()
    # and one device again scores
    single = bflib.beamform(acq.bp, acq.rf, acq.filters).copy()
    rows, _ = bflib.score_last_frames(1)
    check_row(rows[0], single, what="one device again")


def test_copy_frame_and_frame_info(bflib):
    L = bflib.library()
    frames, ids = variants_push("A")
    for k, frame_id in enumerate(ids):
        mine = bflib.copy_frame(frame_id)
        assert mine.shape == frames[k].shape and mine.dtype == frames[k].dtype
        assert np.array_equal(mine.view(np.uint32), frames[k].view(np.uint32)), k
    # the whole 64-byte-rounded export, byte for byte
    each = int(newest_info(L).size_bytes)
    assert each == (24 * 40 * 8 + 63) // 64 * 64
    exported = np.zeros(3 * each // 4, np.uint32)
    assert L.beamformer_get_last_frames(exported.ctypes.data_as(C.c_void_p), exported.nbytes, 3)
    for k, frame_id in enumerate(ids):
        raw = np.full(each // 4 + 4, 0xDEADBEEF, np.uint32)
        assert L.beamformer_hip_copy_frame(frame_id, raw.ctypes.data_as(C.c_void_p), each), bflib.last_error()
        assert np.array_equal(raw[: each // 4], exported[k * each // 4:(k + 1) * each // 4]) and (raw[each // 4:] == 0xDEADBEEF).all()
        # one byte short
        raw[:] = 0xDEADBEEF
        assert not L.beamformer_hip_copy_frame(frame_id, raw.ctypes.data_as(C.c_void_p), each - 1) and bflib.last_error()[0] == E.ExportSpaceOverflow
        assert (raw == 0xDEADBEEF).all()
    assert bytes(bflib.frame_info(ids[2])) == bytes(newest_info(L))
    older = bflib.frame_info(ids[0])
    assert older.frame_id == ids[0] and int(older.device_pointer) == int(newest_info(L).device_pointer) - 2 * each and older.size_bytes == each
    assert not L.beamformer_hip_get_frame_info(ids[2] + 1, C.byref(P.HipFrameInfo())) and bflib.last_error()[0] == E.InvalidAccess
    assert not L.beamformer_hip_get_frame_info(ids[2], None) and bflib.last_error()[0] == E.InvalidAccess


def test_the_autofocus_loop(bflib):
    """variants push -> score -> rank -> copy_frame of the winner, against the host route: download the three frames, apply the reference,
    take the argmax of the same formula"""
    acq = block("A")
    variants = vc.candidates(acq.bp)
    frames = bflib.beamform_variants(acq.bp, acq.rf, variants, acq.filters).copy()
    rows, _ = bflib.score_last_frames(len(variants))
    for criterion in S:
        scores, best = bflib.rank_frames(rows, criterion)
        print(f"  {criterion.name}: device {list(scores)} best {best}; host {[ref.score(ref.metrics(f), criterion) for f in frames]}")
    scores, best = bflib.rank_frames(rows, S.Sharpness)
    host = [ref.score(ref.metrics(f), S.Sharpness) for f in frames]
    # (the three sharpnesses lie percents apart; the rows' sums are within 4e-6 of the reference's: 4e-6 + 2 x 2e-6 for the quotient)
    assert best == int(np.argmax(host)) and np.allclose(scores, host, rtol=1e-5, atol=0.0)
    kept = bflib.copy_frame(rows[best].frame_id)
    assert np.array_equal(kept.view(np.uint32), frames[int(np.argmax(host))].view(np.uint32))


def test_storage_that_a_newer_frame_reused():
    """a 1 MiB frame ring in a process of its own (the ring is sized once per process): tests/frame_metrics_wrap_worker.py"""
    run_ring_worker("frame_metrics_wrap_worker", 1 << 20, expect=("reused",))
