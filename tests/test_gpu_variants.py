"""Variants pushes through the C ABI (beamformer_hip_push_data_variants_with_compute) on the device: one RF frame beamformed on the
block's grid under K triples of speed of sound, time offset and f-number.  Frame k is an ordinary frame of the reference's das.glsl
for the block carrying variants[k]'s values, so it is judged exactly as a single frame is: tests/parity.py compare() against the CPU
oracle run on THAT block, at the project's bars (cases.tolerance: 1e-4 on Float32 RF straight into DAS, 2e-3 on Int16 RF through
Demodulate) -- nothing is loosened.  The blocks are tests/variants_cases.py's: 16 channels x 2 transmits x 256 samples on 24 x 1 x 40.

The variants kernel (csrc/das_variants.hip) takes the variants whose single frames run the general kernel (csrc/das_select.cpp
decide_variants); under das path flag 0x4000, and for blocks it does not take, every variant runs its single-frame kernel(s) under its
derived plan state and must be the single push of the block carrying its values, bit for bit."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

from ogl_beamforming_amd import lib as bf
from ogl_beamforming_amd import params as P
from tests import cases
from tests import variants_cases as vc
from tests.das_push import compare, same_bits, single_push
from tests.parity import reference
from tests.push_kinds import frame_id, single_push_of
from tests.scaffold import automatic_path, run_ring_worker  # noqa: F401

pytestmark = pytest.mark.gpu
E = P.LibError
PREFER, NO_KERNEL = vc.PREFER, vc.NO_KERNEL
FLOAT32_BLOCKS = [(interp, iq, cw) for interp in ("cubic", "linear", "nearest") for iq in (True, False) for cw in (False, True)]


def carrying(acq, v):
    """the acquisition whose parameter block carries the variant's three values: what frame k of a variants push is a single push of"""
    return dataclasses.replace(acq, bp=bf.with_variant(acq.bp, v))


@functools.lru_cache(maxsize=None)
def prepared(interp="linear", iq=True, cw=False, demodulate=False, which="block"):
    """(acquisition, candidates, per candidate: its acquisition and the oracle's reference) -- computed once, shared, left unchanged"""
    from oracle import binding
    binding.library()
    acq = {"block": lambda: vc.block(interp, iq, cw, demodulate=demodulate), "forces": vc.forces_block, "separable": vc.separable_volume,
           "staged": lambda: cases.make("rca_staged_auto")}[which]()
    variants = vc.candidates(acq.bp)
    refs = [(carrying(acq, v),) + tuple(reference(binding, carrying(acq, v))) for v in variants]
    return acq, variants, refs


def oracle_frames_differ(acq, refs):
    """on the oracle alone: the candidates' frames differ from one another by more than 10 x the bar (of the larger frame's maximum) --
    a kernel that ignored its row would not pass the comparison below"""
    tol = cases.tolerance(acq)
    for a in range(len(refs)):
        for b in range(a + 1, len(refs)):
            ra, rb = refs[a][1], refs[b][1]
            ok = ~np.isnan(ra) & ~np.isnan(rb)
            scale = max(np.abs(ra[ok]).max(), np.abs(rb[ok]).max())
            apart = np.abs(ra[ok] - rb[ok]).max() / scale
            print(f"{acq.name}: oracle frames {a} and {b} differ by {apart:.3e} of the frame maximum")
            assert apart > 10 * tol, (a, b, apart)


def check_parity(name, frames, refs, what):
    worst = 0.0
    for k, (frame, (acq_v, ref, _, flags)) in enumerate(zip(frames, refs)):
        v = compare(frame, ref, acq_v, flags, label=f"{name}/{what}/{k}")
        worst = max(worst, v.max_rel_err)
    print(f"{name}: {len(frames)} variants on the {what}: worst max_rel_err {worst:.3e}")


def close_to_single_pushes(bflib, acq, frames, refs, what):
    """every frame within the case's tolerance of the single push of the block carrying its values (another kernel computed it); returns
    how many are bit-equal"""
    tol = cases.tolerance(acq)
    identical = 0
    for k, (acq_v, _, _, flags) in enumerate(refs):
        one = bflib.beamform(acq_v.bp, acq.rf, acq.filters).copy()
        assert np.array_equal(np.isnan(one), np.isnan(frames[k]))
        ok = ~np.isnan(one)
        scale = np.abs(one[ok]).max()
        slack = tol * scale
        if flags is not None:
            # nearest: a tap within float rounding of k + 1/2 may fall either way in either kernel: the oracle's per-voxel budget, once each
            slack = slack + 2.02 * flags["budget"][ok]
        err = np.abs(one[ok] - frames[k][ok])
        assert (err <= slack).all(), f"variant {k}: {what} and single push differ by {err.max() / scale:.3e} of the frame maximum"
        identical += same_bits(one, frames[k])
    return identical


def check_kernel_block(bflib, acq, variants, refs):
    L = bflib.library()
    oracle_frames_differ(acq, refs)
    L.beamformer_hip_set_das_path(PREFER)         # three variants on five tiles are fewer than the kernel takes on its own
    described = bflib.describe_variants(acq.bp, variants, acq.filters)
    assert described.kernel_variants == 3 and described.das_launches == 1, described.reason
    frames = bflib.beamform_variants(acq.bp, acq.rf, variants, acq.filters).copy()
    info = bflib.last_variants_info()
    assert info.variant_count == 3 and info.route.kernel_variants == 3 and info.route.fused_launches == 1 and info.route.das_launches == 1, info.route.reason
    assert list(info.route.taken[:3]) == [1, 1, 1] and info.route.kernel_tiles == described.kernel_tiles
    check_parity(acq.name, frames, refs, "variants kernel")
    # bits: a permuted list comes back permuted, subsets and single variants give the same bits per variant
    for perm in ([2, 0, 1], [1, 2, 0]):
        again = bflib.beamform_variants(acq.bp, acq.rf, [variants[i] for i in perm], acq.filters)
        for i, p in enumerate(perm):
            assert same_bits(again[i], frames[p]), f"frame {i} of the permuted push is not variant {p}"
    for subset in ([0, 2], [1], [0], [2], [1, 1, 0]):
        for i, frame in zip(subset, bflib.beamform_variants(acq.bp, acq.rf, [variants[i] for i in subset], acq.filters)):
            assert same_bits(frame, frames[i]), (subset, i)
    # the per-variant route: each variant IS parameter push + single push, bit for bit
    L.beamformer_hip_set_das_path(NO_KERNEL)
    own = bflib.beamform_variants(acq.bp, acq.rf, variants, acq.filters).copy()
    info = bflib.last_variants_info()
    assert info.route.kernel_variants == 0 and info.route.fused_launches == 0 and info.route.das_launches == 3, info.route.reason
    check_parity(acq.name, own, refs, "per-variant route")
    for k, (acq_v, _, _, _) in enumerate(refs):
        assert same_bits(bflib.beamform(acq_v.bp, acq.rf, acq.filters), own[k]), f"variant {k} is not the single push of the block carrying its values"
    # ... and the fused route stays within tolerance of that single push
    L.beamformer_hip_set_das_path(0)
    identical = close_to_single_pushes(bflib, acq, frames, refs, "variants kernel")
    print(f"{acq.name}: {identical} of 3 variants of the variants kernel equal their single push bit for bit")
    return frames


@pytest.mark.parametrize("interp,iq,cw", FLOAT32_BLOCKS)
def test_variants_kernel_parity_and_bits(interp, iq, cw, bflib):
    acq, variants, refs = prepared(interp, iq, cw)
    assert cases.tolerance(acq) == 1e-4
    check_kernel_block(bflib, acq, variants, refs)


def test_int16_rf_through_demodulate(bflib):
    """the block's time offset is resolved with the Demodulate filter's delay: the per-variant route's bit equality with the single push
    holds only if the derived plan resolves variant 1's shifted offset exactly as the planner does"""
    acq, variants, refs = prepared("linear", True, False, True)
    assert cases.tolerance(acq) == 2e-3 and acq.rf.dtype == np.int16
    check_kernel_block(bflib, acq, variants, refs)


def test_a_flash_block_and_a_single_variant(bflib):
    from oracle import binding
    acq = vc.block("cubic", iq=True, cw=True, flash=True)
    variants = vc.candidates(acq.bp)
    bflib.library().beamformer_hip_set_das_path(PREFER)
    frames = bflib.beamform_variants(acq.bp, acq.rf, variants, acq.filters).copy()
    assert bflib.last_variants_info().route.kernel_variants == 3
    refs = [(carrying(acq, v),) + tuple(reference(binding, carrying(acq, v))) for v in variants]
    oracle_frames_differ(acq, refs)
    check_parity(acq.name, frames, refs, "variants kernel")
    # K = 1: the same code, the same bits; below the threshold of tiles it would run per variant, so both routes are checked
    for mode, kernel in ((PREFER, 1), (NO_KERNEL, 0)):
        bflib.library().beamformer_hip_set_das_path(mode)
        one = bflib.beamform_variants(acq.bp, acq.rf, variants[1:2], acq.filters).copy()
        info = bflib.last_variants_info()
        assert one.shape[0] == 1 and info.variant_count == 1 and info.route.kernel_variants == kernel
        compare(one[0], refs[1][1], refs[1][0], refs[1][3], label=f"{acq.name}/K=1/{mode:#x}")
        if kernel:
            assert same_bits(one[0], frames[1])


def test_the_automatic_route(bflib):
    """without a flag: eight candidates take the kernel, three on five tiles run per variant (csrc/das_select.h: the two thresholds)"""
    acq, variants, refs = prepared("linear", True, True)
    eight = variants + [bf.variant_of(acq.bp, speed_of_sound=1400.0 + 40.0 * k) for k in range(5)]
    frames = bflib.beamform_variants(acq.bp, acq.rf, eight, acq.filters).copy()
    info = bflib.last_variants_info()
    assert info.route.min_variants <= 8 and info.route.kernel_variants == 8 and info.route.das_launches == 1, info.route.reason
    check_parity(acq.name, frames[:3], refs, "variants kernel, automatic")
    few = bflib.beamform_variants(acq.bp, acq.rf, variants, acq.filters).copy()
    info = bflib.last_variants_info()
    assert info.route.kernel_variants == 0 and info.route.das_launches == 3 and b"fewer than" in info.route.reason, info.route.reason
    check_parity(acq.name, few, refs, "per-variant route, automatic")
    bflib.library().beamformer_hip_set_das_path(PREFER)
    for k, frame in enumerate(bflib.beamform_variants(acq.bp, acq.rf, variants, acq.filters)):
        assert same_bits(frame, frames[k]), k


@pytest.mark.parametrize("interp", ["linear", "cubic"])
def test_rows_that_end_under_one_variant_only(interp, bflib):
    """one candidate slow enough that its terms reach the end of the 256-sample rows (chosen on the CPU: row_ends is 1 for it alone);
    base.row_ends of the launch is the OR, settle_index reads each variant's own speed and margin: all meet the bar, and the clear
    variants are bit-equal to a push without the slow one"""
    from oracle import binding
    acq, variants, refs = prepared(interp, True, True)
    slow = vc.slow_candidate(acq.bp, acq.filters)
    assert [vc.row_ends_of(acq.bp, v, acq.filters) for v in variants] == [0, 0, 0] and vc.row_ends_of(acq.bp, slow, acq.filters) == 1
    mixed = [variants[0], slow, variants[1], variants[2]]
    slow_ref = (carrying(acq, slow),) + tuple(reference(binding, carrying(acq, slow)))
    assert np.abs(slow_ref[1][~np.isnan(slow_ref[1])]).max() > 0
    bflib.library().beamformer_hip_set_das_path(PREFER)
    frames = bflib.beamform_variants(acq.bp, acq.rf, mixed, acq.filters).copy()
    assert bflib.last_variants_info().route.kernel_variants == 4
    check_parity(acq.name, frames, [refs[0], slow_ref, refs[1], refs[2]], f"variants kernel, a variant at {slow.speed_of_sound:.0f} m/s")
    clear = bflib.beamform_variants(acq.bp, acq.rf, variants, acq.filters)
    for k, at in enumerate((0, 2, 3)):
        assert same_bits(clear[k], frames[at]), k
    # the slow variant on the per-variant route: its single push, bit for bit
    bflib.library().beamformer_hip_set_das_path(NO_KERNEL)
    own = bflib.beamform_variants(acq.bp, acq.rf, [slow], acq.filters).copy()
    assert same_bits(bflib.beamform(slow_ref[0].bp, acq.rf, acq.filters), own[0])


@pytest.mark.parametrize("which", ["forces", "separable", "staged"])
def test_blocks_the_variants_kernel_does_not_take(which, bflib):
    """a FORCES block (the factored kernel), a separable volume (the gather kernel) and rca_staged_auto (the LDS-staged kernel with the
    planes the row-end rule cuts): each variant's own launch(es) under its derived plan state -- parity, and the single push bit for bit"""
    acq, variants, refs = prepared(which=which)
    oracle_frames_differ(acq, refs)
    bflib.library().beamformer_hip_set_das_path(PREFER)
    described = bflib.describe_variants(acq.bp, variants, acq.filters)
    assert described.kernel_variants == 0, described.reason
    frames = bflib.beamform_variants(acq.bp, acq.rf, variants, acq.filters).copy()
    info = bflib.last_variants_info()
    assert info.route.kernel_variants == 0 and info.route.das_launches == described.das_launches
    assert list(info.route.path[:3]) == list(described.path[:3])
    check_parity(acq.name, frames, refs, "per-variant route")
    for k, (acq_v, _, _, _) in enumerate(refs):
        assert same_bits(bflib.beamform(acq_v.bp, acq.rf, acq.filters), frames[k]), f"variant {k} is not the single push of the block carrying its values"
    # once more: the derived plan states are reused, the frames are the same
    again = bflib.beamform_variants(acq.bp, acq.rf, variants, acq.filters)
    for k in range(3):
        assert same_bits(again[k], frames[k]), k


def test_derived_plan_states_follow_a_replan_of_the_block(bflib):
    """the same candidates after the block has changed (coherency weighting on, another grid): decided anew, each again its single push"""
    acq, variants, _ = prepared("linear", True, False)
    L = bflib.library()
    L.beamformer_hip_set_das_path(NO_KERNEL)
    first = bflib.beamform_variants(acq.bp, acq.rf, variants, acq.filters).copy()
    bp = type(acq.bp).from_buffer_copy(acq.bp)
    bp.coherency_weighting = 1
    bp.output_points[:3] = [20, 1, 33]
    changed = bflib.beamform_variants(bp, acq.rf, variants, acq.filters).copy()
    assert changed.shape[1:] == (33, 1, 20)
    for k, v in enumerate(variants):
        assert same_bits(bflib.beamform(bf.with_variant(bp, v), acq.rf, acq.filters), changed[k]), k
    back = bflib.beamform_variants(acq.bp, acq.rf, variants, acq.filters)
    for k in range(3):
        assert same_bits(back[k], first[k]), k


def test_ids_layout_info_and_the_block_left_alone(bflib):
    L = bflib.library()
    acq, variants, _ = prepared("cubic", False, False)
    before_push = single_push_of(bflib, acq)
    before = frame_id(L).frame_id
    described = bflib.describe_variants(acq.bp, variants, acq.filters)
    frames = bflib.beamform_variants(acq.bp, acq.rf, variants, acq.filters).copy()
    info = bflib.last_variants_info()
    # consecutive ids, variant 0 first; the frame info describes the last variant's frame: the block's grid
    assert info.first_frame_id == before + 1 and info.variant_count == 3
    last = frame_id(L)
    assert last.frame_id == before + 3 and list(last.points) == list(vc.POINTS)
    assert (info.route.kernel_variants, info.route.das_launches, info.route.min_tiles) == (described.kernel_variants, described.das_launches, described.min_tiles)
    assert list(info.route.path[:3]) == list(described.path[:3]) and info.route.reason == described.reason
    assert info.stage_kind[0] == 0xFFFF and info.stage_kind[info.stage_count - 1] == int(P.ShaderKind.DAS) and info.variants_ms > 0
    # get_last_frames(K): oldest first, each rounded to 64 bytes, contiguous
    sizes = [(f.nbytes + 63) // 64 * 64 for f in frames]
    raw = np.full(sum(sizes) // 4 + 16, -7.0, np.float32)
    assert L.beamformer_get_last_frames(raw.ctypes.data_as(C.c_void_p), sum(sizes), 3)
    at = 0
    for f, size in zip(frames, sizes):
        assert np.array_equal(raw[at // 4: at // 4 + f.size].view(np.uint32), f.reshape(-1).view(np.uint32))
        at += size
    assert (raw[at // 4:] == -7.0).all()
    # every variant's row of the timing table: the push's stage times divided by K
    table = P.ComputeStatsTable()
    assert L.beamformer_compute_timings(C.byref(table), -1)
    das = [i for i in range(info.stage_count) if info.stage_kind[i] == int(P.ShaderKind.DAS)][0]
    col = [i for i in range(table.shader_count) if table.shader_ids[i] == int(P.ShaderKind.DAS)][0]
    total = sum(table.times[(info.first_frame_id + k) % 32][col] for k in range(3))
    assert abs(total - info.stage_ms[das] * 1e-3) <= 1e-5 * info.stage_ms[das] * 1e-3 + 1e-12
    # the other info calls refuse this push
    assert not L.beamformer_hip_get_last_views_info(C.byref(P.HipViewsInfo())) and bflib.last_error()[0] == E.InvalidAccess
    assert not L.beamformer_hip_get_last_burst_info(C.byref(P.HipBurstInfo())) and bflib.last_error()[0] == E.InvalidAccess
    assert not L.beamformer_hip_get_last_burst_views_info(C.byref(P.HipBurstViewsInfo())) and bflib.last_error()[0] == E.InvalidAccess
    # the block was left alone: a single push WITHOUT a parameter push gives the block's own frame, the single push before it bit for bit
    assert same_bits(single_push(bflib, acq, acq.rf), before_push)
    assert not L.beamformer_hip_get_last_variants_info(C.byref(P.HipVariantsInfo())) and bflib.last_error()[0] == E.InvalidAccess
    # ... and the variants info refuses a views push and a burst
    bflib.beamform_views(acq.bp, acq.rf, [bf.view_of(acq.bp)], acq.filters)
    assert not L.beamformer_hip_get_last_variants_info(C.byref(P.HipVariantsInfo())) and bflib.last_error()[0] == E.InvalidAccess
    bflib.beamform_burst(acq.bp, np.stack([acq.rf, acq.rf]), acq.filters)
    assert not L.beamformer_hip_get_last_variants_info(C.byref(P.HipVariantsInfo())) and bflib.last_error()[0] == E.InvalidAccess


def test_pair_counting_runs_per_variant(bflib):
    """f_number changes the count: the last variant's (half the f-number) is its single push's, and more than the first's"""
    L = bflib.library()
    acq, variants, refs = prepared("cubic", True, False)
    t = P.HipFrameTimings()
    counts = []
    try:
        L.beamformer_hip_enable_pair_counting(1)
        for subset in (variants, variants[:1]):
            bflib.beamform_variants(acq.bp, acq.rf, subset, acq.filters)
            assert L.beamformer_hip_get_last_frame_timings(C.byref(t))
            counts.append(int(t.das_pairs))
        bflib.beamform(refs[2][0].bp, acq.rf, acq.filters)
        assert L.beamformer_hip_get_last_frame_timings(C.byref(t))
        assert counts[0] == int(t.das_pairs) > counts[1] > 0
    finally:
        L.beamformer_hip_enable_pair_counting(0)


def test_a_run_that_would_straddle_the_end_of_the_ring_starts_again_at_offset_0():
    """a 1 MiB frame ring in a process of its own (the ring is sized once per process): tests/variants_wrap_worker.py"""
    run_ring_worker("variants_wrap_worker", 1 << 20, expect=("wrapped",), timeout=600)
