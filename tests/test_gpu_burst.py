"""Bursts through the C ABI (beamformer_hip_push_data_burst_with_compute) on the device.  Frame k of a burst is judged exactly as a
single frame is: tests/parity.py compare() against the CPU oracle's frame of RF k, with cases.tolerance -- nothing is loosened.  The
RF frames of a burst are independent seeded noise of the case's shape and dtype.

The burst kernel (csrc/das_burst.hip) takes a burst when single frames of the block run the general kernel (csrc/das_select.cpp
decide_burst).  rca_nearest_real has three transmits and its single frames run the factored kernel: it is run under das path 1 (the
general kernel for every frame), where the burst kernel takes it -- the nearest x real instantiation -- and on the automatic path,
where the per-frame route must meet the same checks."""
import ctypes as C
import dataclasses
import statistics
import time

import numpy as np
import pytest

from ogl_beamforming_amd import configs as cfg
from ogl_beamforming_amd import params as P
from tests import cases, draws
from tests.das_push import check_burst, compare, I, noise_frames, row_end_case, same_bits, single_push
from tests.parity import reference
from tests.scaffold import automatic_path, run_ring_worker  # noqa: F401

pytestmark = pytest.mark.gpu
E = P.LibError

BURST_KERNEL_CASES = ["config1_small", "rca_flash_none_tx", "rca_nearest_real", "rca_cubic_real", "rca_f32_complex_in", "rca_i16_complex_in",
                      "rca_f32_demod", "rca_shuffled_padded", "rca_a1s2"]
GENERAL_PATH_FOR = {"rca_nearest_real"}            # see the module docstring
FALLBACK_CASES = ["forces", "hercules_wide_cw", "rca_staged_auto", "config5_literal_order"]
# tests/draws.py draw(): the first 30 seeds whose draw is of the RCA family with at most two transmits and a non-empty image
# (checked again in the test)
RCA_SEEDS = [0, 6, 8, 16, 27, 36, 39, 43, 44, 54, 56, 57, 58, 59, 61, 75, 80, 81, 82, 87, 90, 91, 96, 105, 107, 115, 124, 127, 129, 134]


@pytest.mark.parametrize("n", [5, 9])
@pytest.mark.parametrize("name", BURST_KERNEL_CASES)
def test_burst_kernel_parity(name, n, bflib, oracle):
    acq = cases.make(name)
    if name in GENERAL_PATH_FOR:
        bflib.library().beamformer_hip_set_das_path(1)
    check_burst(bflib, oracle, acq, n, seed=4000 + n, expect_kernel=True)


@pytest.mark.parametrize("interp", [I.Nearest, I.Linear, I.Cubic], ids=["nearest", "linear", "cubic"])
def test_burst_kernel_parity_of_real_samples_under_coherency_weighting(interp, bflib, oracle):
    """the three instances of the burst kernel no case above dispatches: real samples with coherency weighting, one per interpolation
    mode, on the file's two small real cases with the mode and the weighting set in the parameter block; the bars are check_burst's"""
    name = "rca_nearest_real" if interp == I.Nearest else "rca_cubic_real"
    acq = cases.make(name)
    acq.bp.interpolation_mode = int(interp)
    acq.bp.coherency_weighting = 1
    if name in GENERAL_PATH_FOR:
        bflib.library().beamformer_hip_set_das_path(1)
    check_burst(bflib, oracle, acq, 5, seed=4300, expect_kernel=True)


def test_three_transmit_nearest_case_on_its_automatic_route(bflib, oracle):
    """rca_nearest_real as the selection gives it: single frames on the factored kernel, so the burst runs that kernel once per frame"""
    check_burst(bflib, oracle, cases.make("rca_nearest_real"), 5, seed=4100, expect_kernel=False)


@pytest.mark.parametrize("interp", [I.Linear, I.Cubic], ids=["linear", "cubic"])
def test_rows_that_end_inside_the_image(interp, bflib, oracle):
    """settle_index survived the restructuring: on a plane whose oracle flip set is not empty (checked first, on the CPU) every frame
    meets compare()'s rule, the flip-set rule included"""
    acq = row_end_case(interp)
    n = 5
    rf = noise_frames(acq, n, 4200)
    flips = []
    for k in range(n):
        acq_k = dataclasses.replace(acq, rf=rf[k])
        ref, _, flags = reference(oracle, acq_k)
        v = compare(ref.copy(), ref, acq_k, flags, path=-1, label=f"{acq.name}/oracle/{k}")     # the oracle against itself: counts its flip set
        flips.append(v.flip_voxels)
    assert min(flips) >= 1, f"the oracle's flip set is empty on some frame: {flips}"
    d = bflib.describe_das(acq.bp, acq.filters)[4]
    assert int(d.row_ends) == 1
    check_burst(bflib, oracle, acq, n, seed=4200, expect_kernel=True)


@pytest.mark.parametrize("n", [5, 9])
@pytest.mark.parametrize("name", FALLBACK_CASES)
def test_fallback_parity(name, n, bflib, oracle):
    acq = cases.make(name)
    check_burst(bflib, oracle, acq, n, seed=4300 + n, expect_kernel=False)


def test_bursts_and_single_pushes_interleaved_come_back_oldest_first(bflib, oracle):
    acq = cases.make("rca_cubic_real")
    rf = noise_frames(acq, 6, 4400)
    L = bflib.library()
    burst = bflib.beamform_burst(acq.bp, rf[1:4], acq.filters).copy()
    singles = [single_push(bflib, acq, rf[k]) for k in range(6)]
    for k in range(3):
        assert np.abs(burst[k] - singles[1 + k]).max() <= 1e-4 * np.abs(singles[1 + k]).max()
    # single, burst of three, single, burst of two: the union, oldest first
    info = P.HipFrameInfo()
    single_push(bflib, acq, rf[0])
    assert L.beamformer_hip_get_last_frame_info(C.byref(info))
    first_id = info.frame_id
    ptr = rf[1:4].ctypes.data_as(C.c_void_p)
    assert L.beamformer_hip_push_data_burst_with_compute(ptr, rf[0].nbytes, 3, 0, 0), bflib.last_error()
    single_push(bflib, acq, rf[4])
    assert L.beamformer_hip_push_data_burst_with_compute(rf[4:6].ctypes.data_as(C.c_void_p), rf[0].nbytes, 2, 0, 0), bflib.last_error()
    assert L.beamformer_hip_get_last_frame_info(C.byref(info)) and info.frame_id == first_id + 6       # consecutive ids
    got = bflib.get_last_frames(acq.bp, 7)
    expected = [singles[0], burst[0], burst[1], burst[2], singles[4]]
    for k, frame in enumerate(expected):
        assert same_bits(got[k], frame), k
    two = bflib.beamform_burst(acq.bp, rf[4:6], acq.filters)
    assert same_bits(got[5], two[0]) and same_bits(got[6], two[1])
    # a burst of one IS the single push
    assert L.beamformer_hip_push_data_burst_with_compute(rf[2:3].ctypes.data_as(C.c_void_p), rf[0].nbytes, 1, 0, 0)
    assert same_bits(bflib.get_last_frame(acq.bp), singles[2])
    assert not L.beamformer_hip_get_last_burst_info(C.byref(P.HipBurstInfo())) and bflib.last_error()[0] == E.InvalidAccess


def test_a_burst_that_wraps_the_ring_stays_exportable():
    """a 1 MiB frame ring in a process of its own (the ring is sized once per process): tests/burst_wrap_worker.py"""
    run_ring_worker("burst_wrap_worker", 1 << 20, expect=("wrapped",), timeout=600)


def test_timings_of_a_burst_are_per_frame_shares(bflib):
    L = bflib.library()
    acq = cases.make("config1_small")
    n = 8
    bflib.beamform_burst(acq.bp, noise_frames(acq, n, 4600), acq.filters)
    info = bflib.last_burst_info()
    table = P.ComputeStatsTable()
    assert L.beamformer_compute_timings(C.byref(table), -1)
    stages = [(int(info.stage_kind[i]), float(info.stage_ms[i])) for i in range(info.stage_count)]
    assert stages[0][0] == 0xFFFF and stages[-1][0] == int(P.ShaderKind.DAS)
    planned = [s for s in stages if s[0] not in (0xFFFF, 0xFFFE)]
    assert table.shader_count == len(planned)
    for col, (kind, ms) in enumerate(planned):
        assert table.shader_ids[col] == kind
        total = sum(table.times[(info.first_frame_id + k) % 32][col] for k in range(n))
        assert ms > 0 and abs(total - ms * 1e-3) <= 1e-5 * ms * 1e-3 + 1e-12, (kind, total, ms)
    t = P.HipFrameTimings()
    assert L.beamformer_hip_get_last_frame_timings(C.byref(t))
    assert t.das_voxels == acq.voxels and t.das_path == 0 and t.das_taps == 2
    assert abs(t.frame_ms * n - info.burst_ms) <= 1e-5 * info.burst_ms
    # pair counting: the geometry-only count runs once; the newest frame reports what a single push reports
    try:
        L.beamformer_hip_enable_pair_counting(1)
        rf = noise_frames(acq, 3, 4601)
        bflib.beamform_burst(acq.bp, rf, acq.filters)
        assert L.beamformer_hip_get_last_frame_timings(C.byref(t))
        burst_pairs = int(t.das_pairs)
        single_push(bflib, acq, rf[0])
        assert L.beamformer_hip_get_last_frame_timings(C.byref(t))
        assert burst_pairs == int(t.das_pairs) > 0
    finally:
        L.beamformer_hip_enable_pair_counting(0)


@pytest.mark.parametrize("seed", RCA_SEEDS)
def test_random_rca_draws(seed, bflib, oracle, hooks):
    """draws of the general generator with at most two transmits, N drawn from {2, 3, 5, 8, 9}: on the route the automatic selection
    gives the draw, and on the burst kernel (das path 1: the general kernel for single frames) where that is another one.  Every third
    draw runs with SCRATCH_POISON: a frame that read another frame's slice, or an element nobody wrote, shows as NaN."""
    acq = draws.draw(seed)
    K = P.AcquisitionKind
    assert K(acq.bp.acquisition_kind) in (K.RCA_TPW, K.RCA_VLS, K.Flash) and acq.bp.acquisition_count <= 2
    n = int(np.random.default_rng(7000 + seed).choice([2, 3, 5, 8, 9]))
    if seed % 3 == 0:
        hooks.set("SCRATCH_POISON")
    automatic = bool(bflib.describe_burst(acq.bp, n, acq.filters).burst_kernel)
    check_burst(bflib, oracle, acq, n, seed=7100 + seed, expect_kernel=automatic, against_single=False)
    if not automatic:
        bflib.library().beamformer_hip_set_das_path(1)
        takes = bool(bflib.describe_burst(acq.bp, n, acq.filters).burst_kernel)        # (not below kBurstMinFrames)
        assert takes == (n >= bflib.describe_burst(acq.bp, n, acq.filters).min_frames)
        check_burst(bflib, oracle, acq, n, seed=7100 + seed, expect_kernel=takes, against_single=False)


def test_a_burst_of_64_full_size_frames_is_not_slower_than_64_single_pushes(bflib):
    """config 1 at full size, wall time fence to fence with the upload, median of 5 after a warm-up of each: the single path is
    the parent commit's code, and the bar is "not slower" """
    L = bflib.library()
    acq = cfg.config(1)
    n = 64
    rf = noise_frames(acq, n, 4800)
    ptr, size = rf.ctypes.data_as(C.c_void_p), rf[0].nbytes
    frames = [rf[k].ctypes.data_as(C.c_void_p) for k in range(n)]
    bflib.beamform_burst(acq.bp, rf[:2], acq.filters)                  # parameters, plan, buffers

    def singles():
        for p in frames:
            assert L.beamformer_push_data_with_compute(p, size, 0, 0)
        assert L.beamformer_hip_synchronize()

    def burst():
        assert L.beamformer_hip_push_data_burst_with_compute(ptr, size, n, 0, 0)
        assert L.beamformer_hip_synchronize()

    def median_seconds(run):
        run(); run()
        times = []
        for _ in range(5):
            assert L.beamformer_hip_synchronize()
            t0 = time.perf_counter()
            run()
            times.append(time.perf_counter() - t0)
        return statistics.median(times)

    single_s, burst_s = median_seconds(singles), median_seconds(burst)
    info = bflib.last_burst_info()
    assert info.route.burst_kernel == 1
    print(f"rate: 64 config-1 frames: singles {single_s / n * 1e6:.1f} us/frame, burst {burst_s / n * 1e6:.1f} us/frame, ratio {burst_s / single_s:.3f}")
    assert burst_s <= single_s, f"one burst of 64 took {burst_s * 1e3:.3f} ms, 64 single pushes {single_s * 1e3:.3f} ms"
