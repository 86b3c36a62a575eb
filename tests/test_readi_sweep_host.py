"""READI sweeps (beamformer_hip_push_data_readi_sweep_with_compute), everything that needs no device: the route
beamformer_hip_describe_readi_sweep reports and its reason, how the group list is resolved, and the refusals -- which the push makes
before it touches a device, so they are asked of the push itself as well."""
import ctypes as C

import numpy as np
import pytest

from ogl_beamforming_amd import params as P
from tests import cases

E = P.LibError
SYMBOLS = ["beamformer_hip_push_data_readi_sweep_with_compute", "beamformer_hip_push_device_data_readi_sweep_with_compute",
           "beamformer_hip_describe_readi_sweep"]


@pytest.fixture()
def L(bflib):
    lib = bflib.library()
    lib.beamformer_reserve_parameter_blocks(1)
    lib.beamformer_hip_set_das_path(0)
    yield lib
    lib.beamformer_hip_set_das_path(0)


def refused(bflib, kind, call):
    with pytest.raises(bflib.BeamformerError) as e:
        call()
    assert e.value.kind == kind, e.value
    return e.value


def push(bflib, acq, n, groups=None):
    """the host push of n copies of the case's RF: reaches the device only when nothing refuses it first"""
    lib = bflib.library()
    assert lib.beamformer_push_simple_parameters(C.byref(acq.bp)), bflib.last_error()
    rf = np.ascontiguousarray(np.broadcast_to(acq.rf, (max(n, 1),) + acq.rf.shape))
    array = None if groups is None else (C.c_uint32 * len(groups))(*groups)
    bflib._check(lib.beamformer_hip_push_data_readi_sweep_with_compute(rf.ctypes.data_as(C.c_void_p), acq.rf.nbytes, n, array, 0, 0))


def test_the_kernel_takes_sweeps_from_the_threshold_on(L, bflib):
    acq = cases.make("readi")
    first = bflib.describe_readi_sweep(acq.bp, 8)
    m = int(first.min_frames)
    assert m >= 1
    for n in (m, m + 1, 9, 64, 1024):
        d = bflib.describe_readi_sweep(acq.bp, n, [k % 4 for k in range(n)])
        assert d.burst_kernel == 1 and d.das_launches == 1 and d.frames_per_thread == 4 and d.single_path == 0, (n, d.reason)
        assert d.min_frames == m and b"READI sweep" in d.reason


def test_the_per_frame_route_says_why(L, bflib):
    acq = cases.make("readi")
    m = int(bflib.describe_readi_sweep(acq.bp, 8).min_frames)
    if m > 1:
        d = bflib.describe_readi_sweep(acq.bp, m - 1)
        assert d.burst_kernel == 0 and d.das_launches == m - 1 and d.frames_per_thread == 1
        assert f"fewer than {m} frames".encode() in d.reason
    for mode in (0x400, 0x401):
        L.beamformer_hip_set_das_path(mode)
        d = bflib.describe_readi_sweep(acq.bp, 9)
        assert d.burst_kernel == 0 and d.das_launches == 9 and d.frames_per_thread == 1 and d.single_path == 0
        assert b"0x400" in d.reason, d.reason
    # das path 1 alone asks for the general kernel, which the block runs anyway: the sweep kernel takes it
    L.beamformer_hip_set_das_path(1)
    assert bflib.describe_readi_sweep(acq.bp, 9).burst_kernel == 1


@pytest.mark.parametrize("name", ["config1_small", "forces", "readi_one_group"])
def test_blocks_that_are_not_readi_are_refused(name, L, bflib, capfd):
    if name == "readi_one_group":
        acq = cases.make("readi")
        acq.bp.readi_group_count, acq.bp.readi_group = 1, 0
    else:
        acq = cases.make(name)
    capfd.readouterr()
    refused(bflib, E.InvalidAccess, lambda: bflib.describe_readi_sweep(acq.bp, 8))
    assert "READI sweep" in capfd.readouterr().err
    refused(bflib, E.InvalidAccess, lambda: push(bflib, acq, 8))
    assert "READI sweep" in capfd.readouterr().err


def test_a_group_out_of_range_gets_the_single_pushs_error(L, bflib):
    """the documented kind: InvalidComputeStage, what the planner's refusal of a block with that readi_group comes out as"""
    acq = cases.make("readi")
    for groups in ([0, 1, 2, 3, 4], [4, 0, 0, 0, 0], [0, 0, 0, 0, 0xFFFFFFFF]):
        refused(bflib, E.InvalidComputeStage, lambda: bflib.describe_readi_sweep(acq.bp, 5, groups))
        refused(bflib, E.InvalidComputeStage, lambda: push(bflib, acq, 5, groups))
    bad = cases.make("readi")
    bad.bp.readi_group = 4
    assert L.beamformer_push_simple_parameters(C.byref(bad.bp))
    d = P.HipBurstDescription()
    assert not L.beamformer_hip_describe_burst(0, 5, C.byref(d)) and bflib.last_error()[0] == E.InvalidComputeStage


def test_no_list_means_the_blocks_group_onwards(L, bflib):
    acq = cases.make("readi")                      # readi_group 2 of 4
    assert bflib.resolve_readi_groups(acq.bp, 7) == [2, 3, 0, 1, 2, 3, 0]
    assert bflib.resolve_readi_groups(acq.bp, 5, [2, 0, 3, 3, 1]) == [2, 0, 3, 3, 1]
    acq.bp.readi_group = 0
    assert bflib.resolve_readi_groups(acq.bp, 1) == [0]
    a, b = bflib.describe_readi_sweep(acq.bp, 9), bflib.describe_readi_sweep(acq.bp, 9, [k % 4 for k in range(9)])
    assert bytes(a) == bytes(b)


@pytest.mark.parametrize("n", [0, 1025])
def test_frame_counts_out_of_range(n, L, bflib):
    acq = cases.make("readi")
    refused(bflib, E.BufferOverflow, lambda: bflib.describe_readi_sweep(acq.bp, n))
    refused(bflib, E.BufferOverflow, lambda: push(bflib, acq, n))


def test_a_plain_burst_of_the_readi_block_keeps_its_route(L, bflib):
    acq = cases.make("readi")
    assert hasattr(L, SYMBOLS[2])                  # (this module is about the sweep: without it nothing here passes)
    for n in (2, 5, 9):
        d = bflib.describe_burst(acq.bp, n)
        assert d.burst_kernel == 0 and d.das_launches == n and d.frames_per_thread == 1 and d.single_path == 0 and d.min_frames == 5
        assert d.reason.startswith(b"the burst kernel exists for the RCA family")
