"""Variants pushes (beamformer_hip_push_data_variants_with_compute) on the CPU: beamformer_hip_describe_variants (no device needed)
names the route the rules of csrc/das_select.cpp give -- per variant the decision of a block pushed with those values.  What a variants
push shares with every other multi-frame push -- its symbols, its kernel's instantiations, its refusals -- is asked of all kinds in
tests/test_push_contract_host.py."""
import ctypes as C

import pytest

from ogl_beamforming_amd import lib
from ogl_beamforming_amd import params as P
from tests import cases
from tests import variants_cases as vc
from tests.scaffold import automatic_path_on_the_host  # noqa: F401

PREFER, NO_KERNEL = vc.PREFER, vc.NO_KERNEL


def test_an_rca_small_frame_takes_the_variants_kernel_in_one_launch():
    for flash in (False, True):
        acq = vc.block("cubic", iq=True, cw=True, flash=flash)
        variants = vc.candidates(acq.bp)
        # eight candidates: the automatic route (three are fewer than the thresholds: below)
        eight = [lib.variant_of(acq.bp, speed_of_sound=1400.0 + 30.0 * k) for k in range(8)]
        d = lib.describe_variants(acq.bp, eight, acq.filters)
        assert d.min_variants <= 8 and d.kernel_variants == 8 and d.fused_launches == 1 and d.das_launches == 1 and list(d.taken[:8]) == [1] * 8, d.reason
        lib.library().beamformer_hip_set_das_path(PREFER)
        d = lib.describe_variants(acq.bp, variants, acq.filters)
        assert d.kernel_variants == 3 and d.fused_launches == 1 and d.das_launches == 1, d.reason
        assert list(d.path[:3]) == [int(P.DasPath.General)] * 3 and list(d.taken[:3]) == [1, 1, 1]
        # 24 x 1 x 40 voxels: more than three 256-voxel tiles, the last one ragged
        assert d.kernel_tiles % 3 == 0 and d.kernel_tiles // 3 >= 4 and d.min_tiles >= 1 and b"variants kernel" in d.reason
        one = lib.describe_variants(acq.bp, variants[1:2], acq.filters)
        assert one.kernel_variants == 1 and one.kernel_tiles == d.kernel_tiles // 3
        lib.library().beamformer_hip_set_das_path(0)


def test_the_force_flags():
    acq = vc.block("linear", iq=False)
    variants = vc.candidates(acq.bp)
    L = lib.library()
    # 0x4000: every variant on its own launch, and the reason names it; it changes nothing about single frames
    L.beamformer_hip_set_das_path(NO_KERNEL)
    d = lib.describe_variants(acq.bp, variants, acq.filters)
    assert d.kernel_variants == 0 and d.fused_launches == 0 and d.das_launches == 3 and "0x4000" in d.reason.decode()
    assert list(d.path[:3]) == [int(P.DasPath.General)] * 3 and list(d.taken[:3]) == [0, 0, 0]
    assert lib.describe_das(acq.bp, acq.filters)[0] == int(P.DasPath.General)
    # 0x8000: the kernel whatever the tile count (here: as without it)
    L.beamformer_hip_set_das_path(PREFER)
    assert lib.describe_variants(acq.bp, variants, acq.filters).kernel_variants == 3


def on_grid(bp, points):
    out = type(bp).from_buffer_copy(bp)
    out.output_points[:3] = list(points)
    return out


def test_fewer_variants_and_tiles_than_the_thresholds_run_per_variant():
    """two thresholds (csrc/das_select.h): the eligible variants number at least min_variants, or variants x tiles at least min_tiles"""
    acq = vc.block("linear", iq=True)
    L = lib.library()
    speeds = lambda bp, n: [lib.variant_of(bp, speed_of_sound=1400.0 + 5.0 * k) for k in range(n)]
    # a 16 x 1 x 16 grid is ONE 256-voxel tile: the number of variants decides
    bp = on_grid(acq.bp, (16, 1, 16))
    d = lib.describe_variants(bp, speeds(bp, 1), acq.filters)
    few, tiles = int(d.min_variants), int(d.min_tiles)
    assert 2 <= few <= P.HIP_MAX_VARIANTS and tiles > few, (few, tiles)
    below = lib.describe_variants(bp, speeds(bp, few - 1), acq.filters)
    assert below.kernel_variants == 0 and below.das_launches == few - 1 and "fewer than" in below.reason.decode(), below.reason
    at = lib.describe_variants(bp, speeds(bp, few), acq.filters)
    assert at.kernel_variants == few and at.kernel_tiles == few and at.das_launches == 1, at.reason
    L.beamformer_hip_set_das_path(PREFER)
    forced = lib.describe_variants(bp, speeds(bp, 1), acq.filters)
    assert forced.kernel_variants == 1 and forced.kernel_tiles == 1 and forced.das_launches == 1, forced.reason
    # a 256 x 1 x 256 grid: the tiles decide, for fewer than min_variants variants
    bp = on_grid(acq.bp, (256, 1, 256))
    T = int(lib.describe_variants(bp, speeds(bp, 1), acq.filters).kernel_tiles)
    assert T >= 256
    L.beamformer_hip_set_das_path(0)
    need = -(-tiles // T)                        # variants whose tiles reach the threshold
    assert need < few, "the grid is too small to reach the tile threshold with fewer than min_variants variants"
    d = lib.describe_variants(bp, speeds(bp, need), acq.filters)
    assert d.kernel_variants == need and d.kernel_tiles == need * T, d.reason
    if need > 1:
        d = lib.describe_variants(bp, speeds(bp, need - 1), acq.filters)
        assert d.kernel_variants == 0 and "fewer than" in d.reason.decode(), d.reason


def test_other_families_and_faster_kernels_run_per_variant_and_say_why():
    acq = cases.make("forces")
    lib.library().beamformer_hip_set_das_path(PREFER)
    d = lib.describe_variants(acq.bp, vc.candidates(acq.bp), acq.filters)
    assert d.kernel_variants == 0 and d.fused_launches == 0 and d.das_launches == 3 and "family" in d.reason.decode()
    assert d.path[0] == lib.describe_das(acq.bp, acq.filters)[0]
    # rca_staged_auto: the LDS-staged kernel, cut in two by the row-end rule -- two launches a variant
    staged = cases.make("rca_staged_auto")
    mine = [lib.variant_of(staged.bp), lib.variant_of(staged.bp, speed_of_sound=1500.0)]
    d = lib.describe_variants(staged.bp, mine, staged.filters)
    assert d.kernel_variants == 0 and list(d.path[:2]) == [int(P.DasPath.Staged)] * 2 and d.das_launches == 4, d.reason
    assert "row-end rule" in d.reason.decode(), d.reason
    # the two small volumes the device tests run: the factored kernel (FORCES), the separable-delay gather kernel
    for acq, path, word in ((vc.forces_block(), P.DasPath.Factored, "family"), (vc.separable_volume(), P.DasPath.Gather, "gather kernel")):
        d = lib.describe_variants(acq.bp, vc.candidates(acq.bp), acq.filters)
        assert d.kernel_variants == 0 and list(d.path[:3]) == [int(path)] * 3 and d.das_launches == 3 and word in d.reason.decode(), d.reason


@pytest.mark.parametrize("name", ["variants", "forces", "rca_staged_auto", "config1_small", "hercules_wide_cw"])
def test_every_variant_is_described_as_a_block_pushed_with_its_values(name):
    acq = vc.block("cubic", iq=True, demodulate=True) if name == "variants" else cases.make(name)
    bp = acq.bp
    variants = vc.candidates(bp) + [lib.variant_of(bp), lib.variant_of(bp, speed_of_sound=1100.0, f_number=0.4, time_offset=-1e-6)]
    plan_before, das_before = P.HipPlan(), lib.describe_das(bp, acq.filters)
    L = lib.library()
    assert L.beamformer_hip_describe_plan(0, C.byref(plan_before))
    d = lib.describe_variants(bp, variants, acq.filters)
    # the block is as it was: the same plan (its resolved time offset included) and the same DAS decision
    plan_after = P.HipPlan()
    assert L.beamformer_hip_describe_plan(0, C.byref(plan_after)) and bytes(plan_before) == bytes(plan_after)
    described = P.HipDasDescription()
    assert L.beamformer_hip_describe_das(0, C.byref(described)) and bytes(described) == bytes(das_before[4])
    for k, v in enumerate(variants):
        assert d.path[k] == lib.describe_das(lib.with_variant(bp, v), acq.filters)[0], k


def test_the_derived_time_offset_is_the_planners():
    """a block with a Demodulate filter: the plan of the block carrying a variant's time_offset resolves block field + filter delay;
    the variants route's row must carry that float (checked on the device, bit for bit, by tests/test_gpu_variants.py); here: the
    planner adds the delay to whatever the block field is, so a shifted field shifts the resolved offset"""
    acq = vc.block("linear", iq=True, demodulate=True)
    L = lib.library()
    resolved = []
    for shift in (0.0, 0.3e-6):
        bp = lib.with_variant(acq.bp, lib.variant_of(acq.bp, time_offset=acq.bp.time_offset + shift))
        lib.describe_das(bp, acq.filters)
        plan = P.HipPlan()
        assert L.beamformer_hip_describe_plan(0, C.byref(plan))
        resolved.append(float(plan.das_time_offset))
    assert resolved[0] != float(acq.bp.time_offset) and abs((resolved[1] - resolved[0]) - 0.3e-6) < 1e-9
