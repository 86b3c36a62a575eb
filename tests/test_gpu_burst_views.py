"""Burst views pushes through the C ABI (beamformer_hip_push_data_burst_views_with_compute) on the device: N RF frames beamformed on K
grids.  Frame (view v, RF frame k) is an ordinary frame of the reference's das.glsl -- RF k on the block with view v's grid -- so it
is judged exactly as a single frame is: tests/parity.py compare() against the CPU oracle run on that block and that RF, with
cases.tolerance -- nothing is loosened.  The RF frames are independent seeded noise of the case's shape and dtype.

The ladder (csrc/das_select.cpp decide_burst_views): from kBurstViewsMinFrames RF frames on, the fused kernel (csrc/das_burst_views.hip)
takes the views a views push's kernel is eligible for; below it, or under das path flag 0x400, the views push's own DAS step runs per
RF frame and frame (v, k) must be the views push of RF k alone, bit for bit; under 0x800, and for blocks no views kernel takes, every
frame must be the single push of RF k on the block with that grid, bit for bit.  rca_nearest_real runs under das path 1 as in
tests/test_gpu_views.py."""
import ctypes as C
import functools

import numpy as np
import pytest

from ogl_beamforming_amd import lib as bf
from ogl_beamforming_amd import params as P
from tests import cases
from tests.das_push import (box, case_of, close_to_single_push, compare, DISPATCH_CASES, four_views, I, inner, KERNEL_CASES, mode_for, noise_frames,
                            on_grid, per_view_views, row_end_case, same_bits)
from tests.parity import reference
from tests.push_kinds import frame_id
from tests.scaffold import automatic_path, run_ring_worker  # noqa: F401

pytestmark = pytest.mark.gpu
NO_BURST, NO_VIEWS = P.HIP_DAS_PATH_NO_BURST_KERNEL, P.HIP_DAS_PATH_NO_VIEWS_KERNEL
PER_VIEW_CASES = ["forces", "hercules_wide_cw", "rca_staged_auto"]
N = 5


@functools.lru_cache(maxsize=None)
def prepared(name, which="kernel"):
    """(acquisition, N noise RF frames, views, refs[v][k]: the acquisition on view v's grid with RF k and the oracle's reference of it)
    -- computed once, shared, left unchanged"""
    from oracle import binding
    binding.library()
    if name.startswith("row_ends"):
        # the three views of tests/test_gpu_views.py: the whole plane, the strip around the row ends, the strip wholly past them
        acq = row_end_case({"row_ends_linear": I.Linear, "row_ends_cubic": I.Cubic}[name])
        rf = noise_frames(acq, N, 4200)
        lo, hi = box(acq.bp)
        whole = reference(binding, on_grid(acq, bf.view_of(acq.bp), rf[0]))[0]
        r = int(np.flatnonzero((whole != 0).any(axis=(1, 2)))[-1])
        assert 8 <= r <= 80
        views = [bf.view_of(acq.bp), bf.view((96, 1, 12), *inner(lo, hi, (0, 0, (r - 8) / 95), (1, 1, (r + 3) / 95))),
                 bf.view((96, 1, 12), *inner(lo, hi, (0, 0, 84 / 95), (1, 1, 1)))]
    else:
        acq = case_of(name)
        rf = noise_frames(acq, N, 6000)
        views = four_views(acq) if which == "kernel" else per_view_views(acq)
    refs = []
    for v in views:
        row = []
        for k in range(N):
            acq_vk = on_grid(acq, v, rf[k])
            row.append((acq_vk,) + tuple(reference(binding, acq_vk)))
        refs.append(row)
    return acq, rf, views, refs


def check_parity(name, frames, refs, what):
    worst = 0.0
    for v, row in enumerate(refs):
        for k, (acq_vk, ref, _, flags) in enumerate(row):
            verdict = compare(frames[v][k], ref, acq_vk, flags, label=f"{name}/{what}/view{v}/rf{k}")
            worst = max(worst, verdict.max_rel_err)
    print(f"{name}: {len(refs)} views x {len(refs[0])} RF frames on the {what}: worst max_rel_err {worst:.3e}")


@pytest.mark.parametrize("name", KERNEL_CASES + DISPATCH_CASES)
def test_fused_kernel_parity(name, bflib):
    """every one of the K x 5 frames against the oracle on (block with view v's grid, RF k)"""
    acq, rf, views, refs = prepared(name)
    K = len(views)
    bflib.library().beamformer_hip_set_das_path(mode_for(name, 0))
    described = bflib.describe_burst_views(acq.bp, N, views, acq.filters)
    assert (described.rung, described.kernel_views, described.das_launches) == (1, K, 1), described.reason
    frames = bflib.beamform_burst_views(acq.bp, rf, views, acq.filters)
    info = bflib.last_burst_views_info()
    assert (info.frame_count, info.view_count, info.route.rung, info.route.kernel_views, info.route.das_launches) == (N, K, 1, K, 1), info.route.reason
    assert info.route.frames_per_thread == 4
    check_parity(name, frames, refs, "fused kernel")
    for v in range(K):
        for a in range(N):
            for b in range(a + 1, N):
                assert not np.array_equal(frames[v][a], frames[v][b], equal_nan=True), (v, a, b)


@pytest.mark.parametrize("name", KERNEL_CASES)
def test_a_frames_bits_depend_on_neither_its_slot_nor_its_company(name, bflib):
    acq, rf, views, _ = prepared(name)
    K = len(views)
    bflib.library().beamformer_hip_set_das_path(mode_for(name, 0))
    frames = bflib.beamform_burst_views(acq.bp, rf, views, acq.filters)
    # 1. nine RF frames (groups of 4 + 4 + 1) holding the five at permuted positions
    nine = noise_frames(acq, 9, 6100)
    at = [int(i) for i in np.random.default_rng(6101).permutation(9)[:N]]
    for k, position in enumerate(at):
        nine[position] = rf[k]
    longer = bflib.beamform_burst_views(acq.bp, nine, views, acq.filters)
    assert bflib.last_burst_views_info().route.rung == 1
    for v in range(K):
        for k, position in enumerate(at):
            assert same_bits(longer[v][position], frames[v][k]), f"view {v}: RF frame {k} at position {position} of nine has other bits"
    # ... and with one of the five in the last group's single slot
    tail = noise_frames(acq, 9, 6102)
    tail[8] = rf[2]
    last = bflib.beamform_burst_views(acq.bp, tail, views, acq.filters)
    for v in range(K):
        assert same_bits(last[v][8], frames[v][2]), v
    # 2. the view list permuted, a subset of it, a view repeated
    perm = [int(i) for i in np.random.default_rng(6103).permutation(K)]
    again = bflib.beamform_burst_views(acq.bp, rf, [views[i] for i in perm], acq.filters)
    for i, p in enumerate(perm):
        for k in range(N):
            assert same_bits(again[i][k], frames[p][k]), f"view {i} of the permuted push is not view {p} (RF {k})"
    subset = list(range(0, K, 2))
    for i, row in zip(subset, bflib.beamform_burst_views(acq.bp, rf, [views[i] for i in subset], acq.filters)):
        for k in range(N):
            assert same_bits(row[k], frames[i][k]), (i, k)
    alone = bflib.beamform_burst_views(acq.bp, rf, [views[K - 1]], acq.filters)
    twice = bflib.beamform_burst_views(acq.bp, rf, [views[1], views[0], views[1]], acq.filters)
    for k in range(N):
        assert same_bits(alone[0][k], frames[K - 1][k]), k
        assert same_bits(twice[0][k], frames[1][k]) and same_bits(twice[2][k], frames[1][k]) and same_bits(twice[1][k], frames[0][k]), k


@pytest.mark.parametrize("name", KERNEL_CASES)
def test_against_the_burst_push_of_the_block_with_that_grid(name, bflib, oracle):
    """the burst kernel on the block carrying view v's grid: every frame within the parity tolerance (the two kernels are compiled
    separately and contraction outside burst_term is the compiler's: equality is counted, not asserted)"""
    acq, rf, views, refs = prepared(name)
    L = bflib.library()
    L.beamformer_hip_set_das_path(mode_for(name, 0))
    frames = bflib.beamform_burst_views(acq.bp, rf, views, acq.filters)
    identical = 0
    for v in range(len(views)):
        acq_v = refs[v][0][0]
        assert bflib.describe_burst(acq_v.bp, N, acq_v.filters).burst_kernel == 1
        burst = bflib.beamform_burst(acq_v.bp, rf, acq_v.filters).copy()
        for k in range(N):
            close_to_single_push(oracle, refs[v][k][0], rf[k], burst[k], frames[v][k], k)
            identical += same_bits(burst[k], frames[v][k])
    print(f"{name}: {identical} of {len(views) * N} frames of the fused kernel equal the burst kernel's bit for bit")


@pytest.mark.parametrize("name", KERNEL_CASES)
def test_rung_2_is_the_views_push_of_each_rf_frame(name, bflib):
    """four RF frames (below the threshold), and five under flag 0x400"""
    acq, rf, views, _ = prepared(name)
    L = bflib.library()
    K = len(views)
    for n, flag in ((4, 0), (N, NO_BURST)):
        L.beamformer_hip_set_das_path(mode_for(name, flag))
        described = bflib.describe_burst_views(acq.bp, n, views, acq.filters)
        assert (described.rung, described.kernel_views, described.frame_kernel_views) == (2, 0, K), described.reason
        frames = bflib.beamform_burst_views(acq.bp, rf[:n], views, acq.filters)
        info = bflib.last_burst_views_info()
        assert (info.route.rung, info.route.das_launches) == (2, described.das_launches) and info.route.das_launches == n
        for k in range(n):
            alone = bflib.beamform_views(acq.bp, rf[k], views, acq.filters)
            for v in range(K):
                assert same_bits(frames[v][k], alone[v]), f"flag {flag:#x}: frame (view {v}, RF {k}) is not the views push of RF {k}"


def check_rung_3(bflib, name, which, mode):
    acq, rf, views, refs = prepared(name, which)
    L = bflib.library()
    L.beamformer_hip_set_das_path(mode)
    described = bflib.describe_burst_views(acq.bp, N, views, acq.filters)
    assert (described.rung, described.kernel_views, described.frame_kernel_views) == (3, 0, 0), described.reason
    frames = bflib.beamform_burst_views(acq.bp, rf, views, acq.filters)
    info = bflib.last_burst_views_info()
    assert info.route.rung == 3 and info.route.das_launches == described.das_launches and info.route.reason == described.reason
    check_parity(name, frames, refs, "single-frame launches")
    for v in range(len(views)):
        for k in range(N):
            acq_vk = refs[v][k][0]
            one = bflib.beamform(acq_vk.bp, rf[k], acq_vk.filters)
            assert same_bits(one, frames[v][k]), f"frame (view {v}, RF {k}) is not the single push of RF {k} on the block with that grid"


@pytest.mark.parametrize("name", KERNEL_CASES)
def test_flag_0x800_runs_every_frame_as_its_single_push(name, bflib):
    check_rung_3(bflib, name, "kernel", mode_for(name, NO_VIEWS))


@pytest.mark.parametrize("name", PER_VIEW_CASES)
def test_blocks_no_views_kernel_takes_run_every_frame_as_its_single_push(name, bflib):
    check_rung_3(bflib, name, "per_view", 0)


def test_a_mixed_push(bflib):
    """views the fused kernel takes and views it does not: the others are their single push bit for bit, per RF frame"""
    from tests.das_push import mixed_views
    acq = cases.make("rca_flash_none_tx")
    rf = noise_frames(acq, N, 6200)
    views = mixed_views(acq)
    frames = bflib.beamform_burst_views(acq.bp, rf, views, acq.filters)
    info = bflib.last_burst_views_info()
    assert (info.route.rung, info.route.kernel_views, info.route.das_launches) == (1, 2, 1 + 2 * N), info.route.reason
    for k in range(N):
        assert same_bits(frames[1][k], frames[3][k])
        for v in (1, 3):
            acq_v = on_grid(acq, views[v], rf[k])
            assert same_bits(bflib.beamform(acq_v.bp, rf[k], acq.filters), frames[v][k]), (v, k)
    # the taken ones: what the push of those two views alone gives
    alone = bflib.beamform_burst_views(acq.bp, rf, [views[0], views[2]], acq.filters)
    for k in range(N):
        assert same_bits(alone[0][k], frames[0][k]) and same_bits(alone[1][k], frames[2][k]), k


@pytest.mark.parametrize("interp", ["linear", "cubic"])
def test_rows_that_end_inside_the_views(interp, bflib):
    """settle_index in the fused kernel: the whole plane (whose oracle flip set is not empty: checked first, on the CPU) and the strip
    around the row ends meet compare()'s rule, the flip-set rule included; the strip past the ends is zeros, exactly"""
    name = f"row_ends_{interp}"
    acq, rf, views, refs = prepared(name)
    acq_v, ref, _, flags = refs[0][0]
    verdict = compare(ref.copy(), ref, acq_v, flags, path=-1, label=f"{name}/oracle")
    assert verdict.flip_voxels >= 1, "the oracle's flip set is empty on the whole-plane view"
    assert int(bflib.describe_das(acq.bp, acq.filters)[4].row_ends) == 1
    frames = bflib.beamform_burst_views(acq.bp, rf, views, acq.filters)
    route = bflib.last_burst_views_info().route
    assert (route.rung, route.kernel_views) == (1, 3), route.reason
    check_parity(name, frames[:2], refs[:2], "fused kernel")
    for k in range(N):
        assert not refs[2][k][1].any() and np.array_equal(frames[2][k], refs[2][k][1])


@pytest.mark.parametrize("flag", [0, NO_BURST, NO_VIEWS], ids=["rung1", "rung2", "rung3"])
def test_ids_layout_timings_and_info(flag, bflib):
    L = bflib.library()
    acq, rf, views, _ = prepared("config1_small")
    K = len(views)
    bflib.beamform_burst(acq.bp, rf, acq.filters)
    burst_info = bflib.last_burst_info()
    burst_input = [bflib.das_input(acq.bp, frame=k).copy() for k in range(N)]
    before = frame_id(L).frame_id
    L.beamformer_hip_set_das_path(flag)
    described = bflib.describe_burst_views(acq.bp, N, views, acq.filters)
    frames = bflib.beamform_burst_views(acq.bp, rf, views, acq.filters)
    info = bflib.last_burst_views_info()
    # view-major, consecutive ids; the frame info describes the last view's last RF frame
    assert (info.first_frame_id, info.frame_count, info.view_count) == (before + 1, N, K)
    last = frame_id(L)
    assert last.frame_id == before + N * K and list(last.points) == list(views[-1].output_points)
    # the info call agrees with the description
    for field in ("rung", "kernel_views", "frame_kernel_views", "das_launches", "stage_launches", "frames_per_thread", "min_frames", "reason"):
        assert getattr(info.route, field) == getattr(described, field), field
    assert list(info.route.path[:K]) == list(described.path[:K]) and info.decide_us > 0
    # every pre-DAS stage once for the whole push: the stage list of a burst of the same RF
    kinds = [int(info.stage_kind[i]) for i in range(info.stage_count)]
    assert kinds == [int(burst_info.stage_kind[i]) for i in range(burst_info.stage_count)]
    assert kinds[0] == 0xFFFF and kinds[-1] == int(P.ShaderKind.DAS) and len(set(kinds)) == len(kinds) and info.push_ms > 0
    assert info.route.stage_launches == burst_info.route.stage_launches == 1
    # get_last_frames(N K): oldest first, view-major, each at its own 64-byte-rounded size, contiguous
    flat = [frames[v][k] for v in range(K) for k in range(N)]
    sizes = [(f.nbytes + 63) // 64 * 64 for f in flat]
    raw = np.full(sum(sizes) // 4 + 16, -7.0, np.float32)
    assert L.beamformer_get_last_frames(raw.ctypes.data_as(C.c_void_p), sum(sizes), N * K)
    at = 0
    for f, size in zip(flat, sizes):
        assert np.array_equal(raw[at // 4: at // 4 + f.size * (f.itemsize // 4)].view(np.uint32), f.reshape(-1).view(np.uint32))
        at += size
    assert (raw[at // 4:] == -7.0).all()
    # in the ring a view's ensemble is N equal frames at a fixed stride, the views' runs one behind the other
    assert int(last.size_bytes) == sizes[-1]
    # every frame's row of the timing table: a 1 / (N K) share of every stage of the push
    table = P.ComputeStatsTable()
    assert L.beamformer_compute_timings(C.byref(table), -1)
    planned = [(kinds[i], float(info.stage_ms[i])) for i in range(info.stage_count) if kinds[i] not in (0xFFFF, 0xFFFE)]
    assert table.shader_count == len(planned)
    for col, (kind, ms) in enumerate(planned):
        assert table.shader_ids[col] == kind
        rows = [table.times[(info.first_frame_id + j) % 32][col] for j in range(N * K)]
        assert ms > 0 and abs(sum(rows) - ms * 1e-3) <= 1e-5 * ms * 1e-3 + 1e-12, (kind, sum(rows), ms)
        assert max(rows) - min(rows) <= 1e-6 * max(rows)
    t = P.HipFrameTimings()
    assert L.beamformer_hip_get_last_frame_timings(C.byref(t)) and t.das_voxels == int(np.prod(list(views[-1].output_points)))
    assert abs(t.frame_ms * N * K - info.push_ms) <= 1e-5 * info.push_ms
    # copy_das_input_frame(k) serves RF frame k: what a burst of the same RF gives
    for k in range(N):
        assert same_bits(bflib.das_input(acq.bp, frame=k), burst_input[k]), k
    assert not L.beamformer_hip_copy_das_input_frame(N, burst_input[0].ctypes.data_as(C.c_void_p), burst_input[0].nbytes)


def test_pair_counting_runs_once_per_view(bflib):
    L = bflib.library()
    acq, rf, views, refs = prepared("rca_cubic_real")
    t = P.HipFrameTimings()
    try:
        L.beamformer_hip_enable_pair_counting(1)
        bflib.beamform_burst_views(acq.bp, rf, views[:3], acq.filters)
        assert L.beamformer_hip_get_last_frame_timings(C.byref(t))
        pairs = int(t.das_pairs)
        bflib.beamform(refs[2][0][0].bp, rf[0], acq.filters)
        assert L.beamformer_hip_get_last_frame_timings(C.byref(t))
        assert pairs == int(t.das_pairs) > 0
    finally:
        L.beamformer_hip_enable_pair_counting(0)


def test_a_run_that_wraps_the_ring_starts_again_at_0():
    """a 1 MiB frame ring in a process of its own (the ring is sized once per process): tests/burst_views_wrap_worker.py"""
    run_ring_worker("burst_views_wrap_worker", 1 << 20, expect=("wrapped",), timeout=600)


@pytest.mark.parametrize("flag", [0, NO_BURST], ids=["rung1", "rung2"])
def test_no_frame_reads_what_the_push_did_not_write(flag, bflib, hooks):
    """SCRATCH_POISON: both stage buffers and the run's ring slots hold NaN bytes before the push writes them -- a frame that read
    another slice than its RF frame's, or an element nobody wrote, shows as NaN or as other bits"""
    acq, rf, views, refs = prepared("config1_small")
    L = bflib.library()
    L.beamformer_hip_set_das_path(flag)
    plain = bflib.beamform_burst_views(acq.bp, rf, views, acq.filters)
    hooks.set("SCRATCH_POISON")
    frames = bflib.beamform_burst_views(acq.bp, rf, views, acq.filters)
    for v in range(len(views)):
        for k in range(N):
            assert not np.isnan(frames[v][k]).any(), (v, k)
            assert same_bits(frames[v][k], plain[v][k]), (v, k)
    if flag == 0:
        check_parity("config1_small", frames, refs, "fused kernel under SCRATCH_POISON")
