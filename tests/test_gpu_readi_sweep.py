"""READI sweeps through the C ABI (beamformer_hip_push_data_readi_sweep_with_compute) on the device.  Frame k of a sweep is judged exactly
as a single frame is: tests/parity.py compare() against the CPU oracle's frame of RF k with bp.readi_group = groups[k] (a copy of the
parameters per frame), with cases.tolerance -- nothing is loosened.  The RF frames are independent seeded noise of the case's shape.

The cases are the `readi` case's size class (16 channels, 16 transmit elements, 512 samples, 16 x 1 x 16 to 32 x 1 x 32 voxels: one
to four 256-voxel blocks, ragged); between them the parity cases run every interpolation x sample kind x coherency weighting
instantiation of das_readi_burst_kernel (csrc/das_burst.hip) at least once, at N = 5 (one full group of four frame slots and a last
group with three aliased slots) and N = 9."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from ogl_beamforming_amd import configs as cfg
from ogl_beamforming_amd import params as P
from tests import cases
from tests.das_push import close_to_single_push, compare, GEOMETRIES, GROUPS5, groups_for, noise_frames, S, same_bits, sweep_case
from tests.parity import reference
from tests.push_kinds import sweep
from tests.scaffold import automatic_path  # noqa: F401

pytestmark = pytest.mark.gpu
I = P.InterpolationMode

GROUPS9 = [1, 3, 0, 0, 2, 3, 1, 2, 0]


# every interpolation x kind x cw once, the geometries dealt round
VARIANTS = [(list(GEOMETRIES)[i % 3], interp, iq, cw)
            for i, (interp, iq, cw) in enumerate((interp, iq, cw) for interp in (I.Linear, I.Cubic, I.Nearest) for iq in (False, True) for cw in (False, True))]
VARIANT_IDS = [f"{g}-{interp.name.lower()}-{'iq' if iq else 'real'}{'-cw' if cw else ''}" for g, interp, iq, cw in VARIANTS]


def row_end_case(interp):
    """A READI plane of real f32 samples whose 256-sample rows end inside the image: found by a scan of the depth range on the CPU
    (37 um steps of the far depth; of the first 400, steps 55 and 135 qualify for linear and 112 and 223 for cubic), the float oracle
    and its double twin keep or drop a row-end term differently at some voxel of EVERY frame of the sweep below (parity.py's flip set;
    asserted again in the test)."""
    j = ROW_END_STEP[interp]
    return cfg.forces(f"readi_row_ends_{interp.name.lower()}", 16, 4, 256, (32, 1, 32), (-2e-3, 0, 5e-3), (2e-3, 0, 9.0e-3 + j * 37e-6),
                      seed=950 + j, interp=interp, decode=0, data_kind=P.DataKind.Float32, f_number=1.0, readi_groups=4, readi_group=0)


ROW_END_STEP = {I.Linear: 135, I.Cubic: 112}


def with_group(acq, group, rf=None):
    """the acquisition with a COPY of its parameters at readi_group = group (and, given, another RF frame)"""
    bp = type(acq.bp).from_buffer_copy(acq.bp)
    bp.readi_group = int(group)
    return dataclasses.replace(acq, bp=bp, rf=acq.rf if rf is None else rf)


_REFERENCES = {}


def oracle_frame(oracle, acq, rf_seed, k, rf, group):
    """the oracle's (acquisition, frame, flags) of noise frame k of `rf_seed` under `group`: computed once, shared, never written"""
    key = (acq.name, rf_seed, k, int(group))
    if key not in _REFERENCES:
        acq_k = with_group(acq, group, rf)
        ref, _, flags = reference(oracle, acq_k)
        ref.setflags(write=False)
        _REFERENCES[key] = (acq_k, ref, flags)
    return _REFERENCES[key]


def judge(oracle, acq, rf_seed, rf, ks, groups, frames, label):
    """frame i of `frames` is RF ks[i] under groups[i]: compare() against the oracle, each frame; returns the worst relative error"""
    worst = 0.0
    for i, (k, g) in enumerate(zip(ks, groups)):
        acq_k, ref, flags = oracle_frame(oracle, acq, rf_seed, k, rf[k], g)
        v = compare(frames[i], ref, acq_k, flags, label=f"{acq.name}/{label}/{i}")
        worst = max(worst, v.max_rel_err)
    return worst


def single_push(bflib, acq, rf, group):
    """a parameter push with the group, then a single push of the RF"""
    one = with_group(acq, group)
    return bflib.beamform(one.bp, np.ascontiguousarray(rf), acq.filters).copy()


@pytest.mark.parametrize("n", [5, 9])
@pytest.mark.parametrize("geometry,interp,iq,cw", VARIANTS, ids=VARIANT_IDS)
def test_sweep_kernel_parity(geometry, interp, iq, cw, n, bflib, oracle):
    acq = sweep_case(geometry, interp, iq, cw)
    groups = groups_for(acq, GROUPS5 if n == 5 else GROUPS9)
    rf = noise_frames(acq, n, 5000 + n)
    frames = sweep(bflib, acq, rf, groups)
    worst = judge(oracle, acq, 5000 + n, rf, range(n), groups, frames, f"sweep{n}")
    print(f"{acq.name}: sweep of {n} on the sweep kernel: worst max_rel_err {worst:.3e} (tolerance {cases.tolerance(acq):.0e})")


@pytest.mark.parametrize("interp", [I.Linear, I.Cubic, I.Nearest], ids=["linear", "cubic", "nearest"])
def test_the_sign_table_is_read_per_frame(interp, bflib, oracle):
    """the same RF under two groups: two different frames, each its own group's; two RFs under one group: each its own RF's"""
    acq = sweep_case("g4a4", interp, False, True)
    rf = noise_frames(acq, 2, 5100)
    ks, groups = [0, 0, 1, 1, 0], [1, 3, 3, 3, 0]           # frames 0 / 1: RF 0 under 1 and 3; frames 1 / 2: RFs 0 and 1 under 3
    frames = sweep(bflib, acq, rf[ks], groups)
    assert not np.array_equal(frames[0], frames[1], equal_nan=True)
    assert not np.array_equal(frames[1], frames[2], equal_nan=True)
    assert same_bits(frames[2], frames[3])
    judge(oracle, acq, 5100, rf, ks, groups, frames, "signs")


@pytest.mark.parametrize("geometry,interp,iq,cw", [VARIANTS[1], VARIANTS[6], VARIANTS[8]], ids=[VARIANT_IDS[1], VARIANT_IDS[6], VARIANT_IDS[8]])
def test_bits_do_not_depend_on_the_slot(geometry, interp, iq, cw, bflib):
    acq = sweep_case(geometry, interp, iq, cw)
    rf = noise_frames(acq, 9, 5009)
    groups = groups_for(acq, GROUPS9)
    nine = sweep(bflib, acq, rf, groups)
    perm = np.random.default_rng(5201).permutation(9)
    again = sweep(bflib, acq, rf[perm], [groups[p] for p in perm])
    for i in range(9):
        assert same_bits(again[i], nine[perm[i]]), f"frame {i} of the permuted sweep is not the frame of (RF, group) pair {perm[i]}"
    # (RF, group) pairs 4 .. 8 of the nine as a sweep of five: other slots, other groups of slots, the same bits
    five = sweep(bflib, acq, rf[4:9], groups[4:9])
    for i in range(5):
        assert same_bits(five[i], nine[4 + i]), i


@pytest.mark.parametrize("geometry,interp,iq,cw", VARIANTS, ids=VARIANT_IDS)      # (all twelve: the single pushes are the general kernel's READI instances)
def test_the_per_frame_route_is_the_single_push(geometry, interp, iq, cw, bflib, oracle):
    """under das path flag 0x400 every frame is the single push's, bit for bit; the kernel's frames of the same sweep are within
    close_to_single_push's slack of them"""
    acq = sweep_case(geometry, interp, iq, cw)
    n = 5
    groups = groups_for(acq, GROUPS5)
    rf = noise_frames(acq, n, 5005)
    kernel = sweep(bflib, acq, rf, groups)
    L = bflib.library()
    L.beamformer_hip_set_das_path(0x400)
    per_frame = sweep(bflib, acq, rf, groups, expect_kernel=False)
    assert b"0x400" in bflib.last_burst_info().route.reason
    judge(oracle, acq, 5005, rf, range(n), groups, per_frame, "per-frame")
    singles = [single_push(bflib, acq, rf[k], groups[k]) for k in range(n)]
    L.beamformer_hip_set_das_path(0)
    identical = 0
    for k in range(n):
        assert same_bits(per_frame[k], singles[k]), f"frame {k} of the per-frame route is not its single push"
        close_to_single_push(oracle, with_group(acq, groups[k]), rf[k], singles[k], kernel[k], k)
        identical += same_bits(singles[k], kernel[k])
    print(f"{acq.name}: {identical} of {n} frames of the sweep kernel equal their single push bit for bit")
    # below the threshold the automatic path takes the same route: a sweep of two, and of one
    m = int(bflib.describe_readi_sweep(acq.bp, 2).min_frames)
    for count in (1, 2):
        if count < m:
            few = sweep(bflib, acq, rf[:count], groups[:count], expect_kernel=False)
            for k in range(count):
                assert same_bits(few[k], singles[k]), (count, k)


def test_no_list_is_the_blocks_group_onwards(bflib):
    acq = sweep_case("g4a4", I.Cubic, True, False)          # readi_group 1 of 4
    rf = noise_frames(acq, 6, 5300)
    listed = sweep(bflib, acq, rf, [1, 2, 3, 0, 1, 2])
    implied = sweep(bflib, acq, rf, None)
    for k in range(6):
        assert same_bits(listed[k], implied[k]), k
    assert not same_bits(implied[0], implied[4])             # (the same group, another RF)


@pytest.mark.parametrize("interp", [I.Linear, I.Cubic], ids=["linear", "cubic"])
def test_rows_that_end_inside_the_image(interp, bflib, oracle):
    """settle_index in the sweep kernel: on a plane whose oracle flip set is not empty on any frame (checked first, on the CPU) every
    frame meets compare()'s rule, the flip-set rule included"""
    acq = row_end_case(interp)
    n = 5
    groups = groups_for(acq, GROUPS5)
    rf = noise_frames(acq, n, 4200)
    flips = []
    for k in range(n):
        acq_k, ref, flags = oracle_frame(oracle, acq, 4200, k, rf[k], groups[k])
        v = compare(ref.copy(), ref, acq_k, flags, path=-1, label=f"{acq.name}/oracle/{k}")     # the oracle against itself: counts its flip set
        flips.append(v.flip_voxels)
    assert min(flips) >= 1, f"the oracle's flip set is empty on some frame: {flips}"
    assert int(bflib.describe_das(acq.bp, acq.filters)[4].row_ends) == 1
    frames = sweep(bflib, acq, rf, groups)
    judge(oracle, acq, 4200, rf, range(n), groups, frames, "row-ends")


def test_sweeps_single_pushes_and_bursts_interleaved_come_back_oldest_first(bflib):
    acq = sweep_case("g4a4", I.Linear, False, False)
    rf = noise_frames(acq, 8, 5400)
    groups = [3, 1, 0, 2, 2]
    L = bflib.library()
    swept = sweep(bflib, acq, rf[1:6], groups)
    burst = bflib.beamform_burst(acq.bp, rf[6:8], acq.filters).copy()
    first = single_push(bflib, acq, rf[0], acq.bp.readi_group)
    info = P.HipFrameInfo()
    assert L.beamformer_hip_get_last_frame_info(C.byref(info))
    first_id = info.frame_id
    size = rf[0].nbytes
    assert L.beamformer_hip_push_data_readi_sweep_with_compute(rf[1:6].ctypes.data_as(C.c_void_p), size, 5, (C.c_uint32 * 5)(*groups), 0, 0), bflib.last_error()
    assert L.beamformer_hip_push_data_burst_with_compute(rf[6:8].ctypes.data_as(C.c_void_p), size, 2, 0, 0), bflib.last_error()
    assert L.beamformer_push_data_with_compute(rf[0].ctypes.data_as(C.c_void_p), size, 0, 0), bflib.last_error()
    assert L.beamformer_hip_get_last_frame_info(C.byref(info)) and info.frame_id == first_id + 8       # consecutive ids
    got = bflib.get_last_frames(acq.bp, 9)
    for k, frame in enumerate([first] + list(swept) + list(burst) + [first]):
        assert same_bits(got[k], frame), k


def test_timing_rows_are_shares_and_pair_counts_are_the_single_frames(bflib):
    L = bflib.library()
    acq = sweep_case("g4a4", I.Linear, False, False)
    n = 8
    rf = noise_frames(acq, n, 5600)
    sweep(bflib, acq, rf, [k % 4 for k in range(n)])
    info = bflib.last_burst_info()
    table = P.ComputeStatsTable()
    assert L.beamformer_compute_timings(C.byref(table), -1)
    stages = [(int(info.stage_kind[i]), float(info.stage_ms[i])) for i in range(info.stage_count)]
    assert stages[0][0] == 0xFFFF and stages[-1][0] == int(S.DAS)
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
    # pair counting: the geometry-only count does not depend on the group; every frame reports the single push's
    try:
        L.beamformer_hip_enable_pair_counting(1)
        single_push(bflib, acq, rf[0], 0)
        assert L.beamformer_hip_get_last_frame_timings(C.byref(t))
        single_pairs = int(t.das_pairs)
        assert single_pairs > 0
        for mode in (0, 0x400):
            L.beamformer_hip_set_das_path(mode)
            sweep(bflib, acq, rf[:5], [3, 1, 1, 0, 2], expect_kernel=mode == 0)
            assert L.beamformer_hip_get_last_frame_timings(C.byref(t)) and int(t.das_pairs) == single_pairs, mode
        # (the table serves the newest frame: shorter sweeps put other frames of the list there)
        for count in (2, 3):
            sweep(bflib, acq, rf[:count], [3, 1, 1][:count], expect_kernel=False)
            assert L.beamformer_hip_get_last_frame_timings(C.byref(t)) and int(t.das_pairs) == single_pairs, count
    finally:
        L.beamformer_hip_set_das_path(0)
        L.beamformer_hip_enable_pair_counting(0)


def test_a_plain_burst_of_the_readi_block_is_what_it_was(bflib, oracle):
    """every frame under the block's one group, on the per-frame route: the single pushes, bit for bit"""
    acq = cases.make("readi")
    assert hasattr(bflib.library(), "beamformer_hip_describe_readi_sweep")
    n = 5
    rf = noise_frames(acq, n, 5900)
    assert bflib.describe_burst(acq.bp, n, acq.filters).burst_kernel == 0
    frames = bflib.beamform_burst(acq.bp, rf, acq.filters).copy()
    info = bflib.last_burst_info()
    assert info.route.burst_kernel == 0 and info.route.das_launches == n and info.route.min_frames == 5
    group = int(acq.bp.readi_group)
    judge(oracle, acq, 5900, rf, range(n), [group] * n, frames, "plain-burst")
    for k in range(n):
        assert same_bits(frames[k], single_push(bflib, acq, rf[k], group)), k
