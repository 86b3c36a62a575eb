"""What every frame operation owes its caller, on the device, asked of the operations of tests/frame_ops_table.py.  csrc/frame_ops.cpp
takes their source frames through shared functions (newest_ensemble_frames, frames_once_a_box, queue_frames_of_newest), so each rule
is one test, parametrised over OPS, and every refusal is asked in the strictest form (frame_ops_table.refused): the error kind, every
output untouched, the newest id and the newest record's bytes unchanged, the next single push at id + 1 and at the old pointer +
round64(size).

Value parity and everything that is about one operation alone are in that operation's own test_gpu_*.py module.  Das path flag 0x2000
is the only failure a test here causes: a refusal on the host, before any DAS launch."""
import ctypes as C

import numpy as np
import pytest

from ogl_beamforming_amd import params as P
from tests import variants_cases as vc
from tests.frame_info import newest_id
from tests.frame_ops_table import OPS, PRODUCE, refused
from tests.ring_frames import block, ensemble, metrics_block, rf_frames
from tests.scaffold import automatic_path, run_ring_worker, two_contexts_on_device_0  # noqa: F401

pytestmark = pytest.mark.gpu
E = P.LibError


def of(ops):
    return pytest.mark.parametrize("op", ops, ids=[op.name for op in ops])


def single_push(bflib, which):
    acq = block(which)
    bflib.beamform(acq.bp, rf_frames(which, 1)[0], acq.filters)


@of(OPS)
def test_more_frames_than_were_ever_queued_are_refused(op, bflib):
    """a fresh context with two frames, and three are asked for"""
    L = bflib.library()
    for form in op.forms(3):
        L.beamformer_hip_shutdown()                                   # (refused() pushes a third frame: a fresh context for every form)
        assert L.beamformer_hip_set_devices((C.c_int32 * 1)(0), 1)
        frames, ids = ensemble("plane", 2)
        assert ids == [0, 1]
        refused(L, op, 3, E.InvalidAccess, **form)
    frames, ids = ensemble("plane", 2)
    op.good_call("plane", frames, ids, "two frames")


@of(OPS)
def test_a_tombstone_among_the_frames_is_refused(op, bflib):
    """a variants push that fails at its DAS stage (das path flag 0x2000) leaves three tombstones, without any device fault: a call
    that covers only tombstones, tombstones and good frames, a good frame and a tombstone; a good frame behind them is then served"""
    L = bflib.library()
    acq = metrics_block("A")
    variants = vc.candidates(acq.bp)
    bflib.beamform_variants(acq.bp, acq.rf, variants, acq.filters)
    rf = np.ascontiguousarray(acq.rf)
    L.beamformer_hip_set_das_path(P.HIP_DAS_PATH_FAIL_VIEWS_DAS)
    assert not L.beamformer_hip_push_data_variants_with_compute(rf.ctypes.data_as(C.c_void_p), rf.nbytes, (P.HipDasVariant * 3)(*variants), 3, 0, 0)
    L.beamformer_hip_set_das_path(0)
    # the newest push is a tombstone: there is no newest record, so refused() holds these two to the error kind, the sentinels and the
    # id alone and pushes nothing -- K = 2 below still covers a tombstone
    assert newest_id(L) is None
    refused(L, op, 1, E.InvalidAccess)
    refused(L, op, 4, E.InvalidAccess)
    frames, ids = ensemble("plane", 1)
    refused(L, op, 2, E.InvalidAccess)                                # the strict form; it pushes the same plane frame once more
    op.good_call("plane", frames, [newest_id(L)], "behind the tombstones")


@of(OPS)
def test_several_devices_are_refused(op, bflib):
    L = bflib.library()
    with two_contexts_on_device_0(bflib, vc.separable_volume()):
        for form in op.forms(1):
            refused(L, op, 1, E.InvalidAccess, **form)
    frames, ids = ensemble("plane", 2)
    op.good_call("plane", frames, ids, "one device again")


@of(OPS)
def test_frames_of_two_grids_and_of_two_kinds_are_refused(op, bflib):
    """DataSizeMismatch (csrc/frame_ops.cpp newest_ensemble_frames); refused() leaves a complex plane frame behind each time"""
    L = bflib.library()
    ensemble("plane", 2)
    single_push(bflib, "volume")
    for form in op.forms(2):
        refused(L, op, 2, E.DataSizeMismatch, **form)                 # plane, volume
        single_push(bflib, "volume")
    single_push(bflib, "square")
    refused(L, op, 2, E.DataSizeMismatch)                             # volume, square
    refused(L, op, 3, E.DataSizeMismatch)                             # volume, square, plane
    for form in op.forms(2):
        single_push(bflib, "real")
        refused(L, op, 2, E.DataSizeMismatch, **form)                 # one grid, two kinds: the plane refused() pushed, the real plane
    frames, ids = ensemble("plane", 2)
    op.good_call("plane", frames, ids, "one grid again")


# a box one voxel too wide, one voxel too far, behind the last plane, without extent along y, and a first that wraps: on the plane 33 x 1 x 7
OUTSIDE = (((0, 0, 0), (34, 1, 7)), ((1, 0, 0), (33, 1, 7)), ((0, 0, 7), (1, 1, 1)), ((0, 0, 0), (33, 0, 7)), ((0xFFFFFFFF, 0, 0), (2, 1, 1)))


@of([op for op in OPS if op.takes_region])
def test_a_box_outside_the_frames_or_without_extent_is_refused(op, bflib):
    L = bflib.library()
    ensemble("plane", 2)
    for box in OUTSIDE:
        for boxes in op.box_lists(box):
            refused(L, op, 2, E.InvalidAccess, boxes=boxes)
    frames, ids = ensemble("plane", 2)
    op.good_call("plane", frames, ids, "behind the boxes")


@of([op for op in OPS if op.malformed])
def test_every_malformed_call_on_a_live_device_with_frames_present_changes_nothing(op, bflib):
    L = bflib.library()
    for row in op.malformed:
        ensemble(row.which, row.K)
        print(f"  {op.name}: {row.what}")
        refused(L, op, row.K, row.error, **row.change())
        if row.counterpart:
            row.counterpart(*ensemble(row.which, row.K))             # the nearest good call runs
    which = op.malformed[-1].which
    frames, ids = ensemble(which, 3)
    op.good_call(which, frames, ids, "after the refusals")


@of(PRODUCE)
def test_an_untimed_call_does_not_synchronise_and_what_follows_sees_the_frames(op, bflib):
    frames, ids = ensemble("square", 3)
    run = op.run(3, np.random.default_rng(9960))
    first, ms = run.call(timed=False)
    assert ms == 0 and first == ids[-1] + 1
    got = bflib.get_last_frames(block("square").bp, run.outputs)
    print(f"  {op.name} untimed: worst error {run.judge(got, frames):.4f} of its bound")


@of(PRODUCE)
def test_the_ring_a_run_that_wraps_and_one_that_would_reuse_its_sources(op):
    """a 1 MiB frame ring in a process of its own (the ring is sized once per process): tests/frame_run_wrap_worker.py"""
    run_ring_worker("frame_run_wrap_worker", 1 << 20, expect=("refused", "wrapped"), args=(op.name,))
