"""Bursts (beamformer_hip_push_data_burst_with_compute) on the CPU: beamformer_hip_describe_burst (no device needed) names the route the
rules of csrc/das_select.cpp give.  What a burst shares with every other multi-frame push -- its symbols, its kernel's instantiations,
its refusals -- is asked of all kinds in tests/test_push_contract_host.py."""
import ctypes as C

import numpy as np
import pytest

from ogl_beamforming_amd import lib
from ogl_beamforming_amd import params as P
from tests import burst_chunk_cases, cases

E = P.LibError


@pytest.mark.parametrize("name", ["config1_small", "rca_flash_none_tx", "rca_cubic_real"])
@pytest.mark.parametrize("n", [5, 64])
def test_general_kernel_rca_blocks_take_the_burst_kernel_in_one_launch(name, n):
    acq = cases.make(name)
    lib.library().beamformer_hip_set_das_path(0)
    d = lib.describe_burst(acq.bp, n, acq.filters)
    assert d.burst_kernel == 1 and d.das_launches == 1, d.reason
    assert d.single_path == int(P.DasPath.General) and d.frames_per_thread == 4
    assert d.stage_launches == 1 and d.reason          # ingest and every pre-DAS stage: one launch for the burst


@pytest.mark.parametrize("name, word", [("forces", "family"), ("hercules_real", "family"), ("rca_staged_auto", "kernel")])
def test_other_blocks_take_the_fallback_and_say_why(name, word):
    acq = cases.make(name)
    lib.library().beamformer_hip_set_das_path(0)
    single = lib.describe_das(acq.bp, acq.filters)
    d = lib.describe_burst(acq.bp, 5, acq.filters)
    assert d.burst_kernel == 0 and d.frames_per_thread == 1
    assert d.single_path == single[0]
    assert word in d.reason.decode(), d.reason
    # the single-frame launches, once per frame: rca_staged_auto's frames are cut in two by the row-end rule
    parts = 2 if name == "rca_staged_auto" else 1
    assert d.das_launches == 5 * parts and d.stage_launches == 1


def test_fewer_frames_than_the_threshold_and_the_flag_take_the_fallback():
    acq = cases.make("config1_small")
    L = lib.library()
    L.beamformer_hip_set_das_path(0)
    d = lib.describe_burst(acq.bp, 2, acq.filters)
    assert d.min_frames >= 2
    below = lib.describe_burst(acq.bp, d.min_frames - 1, acq.filters)
    assert below.burst_kernel == 0 and "fewer than" in below.reason.decode()
    assert lib.describe_burst(acq.bp, d.min_frames, acq.filters).burst_kernel == 1
    try:
        L.beamformer_hip_set_das_path(P.HIP_DAS_PATH_NO_BURST_KERNEL)
        forced = lib.describe_burst(acq.bp, 64, acq.filters)
        assert forced.burst_kernel == 0 and forced.das_launches == 64 and "0x400" in forced.reason.decode()
        # the flag changes nothing about single frames
        assert lib.describe_das(acq.bp, acq.filters)[0] == int(P.DasPath.General)
    finally:
        L.beamformer_hip_set_das_path(0)
    assert not L.beamformer_hip_describe_burst(0, 0, C.byref(P.HipBurstDescription())) and lib.last_error()[0] == E.InvalidAccess


def test_long_bursts_of_many_channels_take_the_filters_in_chunks():
    """the filters' grid carries frames x channels on one 16-bit axis: 65535 // 64 = 1023 frames of config 1's 64 channels a launch"""
    acq = cases.make("config1_small")
    acq.bp.channel_count = 64
    acq.bp.raw_data_dimensions[1] = 64
    lib.library().beamformer_hip_set_das_path(0)
    assert lib.describe_burst(acq.bp, 1023, acq.filters).stage_launches == 1
    assert lib.describe_burst(acq.bp, 1024, acq.filters).stage_launches == 2


@pytest.mark.parametrize("name", sorted(burst_chunk_cases.CASES))
def test_the_chunk_boundary_cases_cross_a_chunk(name):
    """tests/burst_chunk_cases.py, which tests/test_gpu_stages_burst.py runs on the device: 257 frames take two launches of the
    filter-shaped stages and 255 take one, so that a change to a case or to the chunk rule cannot turn the device test into a one-launch
    test unseen; and each case keeps the stage form it is there for"""
    bc = burst_chunk_cases
    L = lib.library()
    L.beamformer_hip_set_das_path(0)
    assert L.beamformer_hip_enable_hilbert(1 if name in bc.NEEDS_HILBERT else 0)
    try:
        acq = bc.CASES[name]()
        assert (bc.FRAMES, bc.CHANNELS, bc.CHUNK) == (257, 256, 255) and acq.bp.channel_count == bc.CHANNELS
        assert lib.describe_burst(acq.bp, bc.FRAMES, acq.filters).stage_launches == 2
        assert lib.describe_burst(acq.bp, bc.CHUNK, acq.filters).stage_launches == 1
        plan = P.HipPlan()
        assert L.beamformer_hip_describe_plan(0, C.byref(plan))
        kinds = [int(plan.stages[i].kind) for i in range(plan.stage_count)]
        S = P.ShaderKind
        assert kinds == {"demodulate_das": [S.Demodulate, S.DAS], "demodulate_decode_das": [S.Demodulate, S.Decode, S.DAS],
                         "decode_hilbert_das": [S.Hilbert, S.DAS]}[name]
        first = plan.stages[0]
        if name == "demodulate_decode_das":      # the transposing 1024-thread filter form (csrc/stages.hip launch_filter_chunk)
            assert acq.bp.acquisition_count == 4 and first.out_stride[2] == 1 and first.out_stride[0] >= 4 and first.out_kind & 1
        if name == "demodulate_das":
            assert acq.bp.decimation_rate == 2 and acq.bp.acquisition_count == 1 and acq.bp.data_kind == int(P.DataKind.Int16)
    finally:
        L.beamformer_hip_enable_hilbert(0)
    a = bc.assignment(9400)
    assert len(a) == bc.FRAMES and len({a[254], a[255], a[256]}) == 3 and a[255] != a[0] and a[256] != a[1]
    assert np.array_equal(a, bc.assignment(9400)) and len(set(a)) == bc.SOURCES
