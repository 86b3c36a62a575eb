"""Views pushes through the C ABI (beamformer_hip_push_data_views_with_compute) on the device: one RF frame beamformed on K grids.
Every view is an ordinary frame of the reference's das.glsl on its own das_voxel_transform / output_points, so view k is judged exactly
as a single frame is: tests/parity.py compare() against the CPU oracle run on the block WITH THAT GRID, with cases.tolerance -- nothing
is loosened.  The RF is seeded noise of the case's shape and dtype.

The views kernel (csrc/das_views.hip) takes the views whose single frames run the general kernel (csrc/das_select.cpp decide_views);
das path flag 0x1000 makes it take them however few their tiles.  rca_nearest_real has three transmits and its single frames run the
factored kernel: it is run under das path 1 (the general kernel for every frame), where the views kernel takes it -- the nearest x
real instantiation.  Under flag 0x800, and for blocks the views kernel does not take, every view runs its single-frame kernel on the
shared DAS input and must be the single push of the block with that grid, bit for bit."""
import ctypes as C

import numpy as np
import pytest

from ogl_beamforming_amd import params as P
from tests import cases
from tests.das_push import compare, DISPATCH_CASES, KERNEL_CASES, mode_for, noise_frames, on_grid, prepared, same_bits, single_push
from tests.parity import reference
from tests.push_kinds import frame_id
from tests.scaffold import automatic_path  # noqa: F401

pytestmark = pytest.mark.gpu
E = P.LibError

PER_VIEW_CASES = ["forces", "hercules_wide_cw", "rca_staged_auto", "config5_literal_order"]
PREFER, NO_KERNEL = P.HIP_DAS_PATH_PREFER_VIEWS_KERNEL, P.HIP_DAS_PATH_NO_VIEWS_KERNEL


def check_parity(name, frames, refs, what):
    worst = 0.0
    for k, (frame, (acq_v, ref, _, flags)) in enumerate(zip(frames, refs)):
        v = compare(frame, ref, acq_v, flags, label=f"{name}/{what}/{k}")
        worst = max(worst, v.max_rel_err)
    print(f"{name}: {len(frames)} views on the {what}: worst max_rel_err {worst:.3e}")


@pytest.mark.parametrize("name", KERNEL_CASES)
def test_views_kernel(name, bflib):
    """parity of every view; identical views are bit-equal; permuted views come back permuted, a subset alone gives the same bits;
    every view within the case's tolerance of the single push of the block carrying that grid"""
    L = bflib.library()
    acq, rf, views, refs = prepared(name)
    L.beamformer_hip_set_das_path(mode_for(name, PREFER))
    described = bflib.describe_views(acq.bp, views, acq.filters)
    assert described.kernel_views == len(views) and described.das_launches == 1, described.reason
    frames = bflib.beamform_views(acq.bp, rf, views, acq.filters)
    info = bflib.last_views_info()
    assert info.view_count == len(views) and info.route.kernel_views == len(views) and info.route.das_launches == 1, info.route.reason
    check_parity(name, frames, refs, "views kernel")
    # 2. the two identical views
    twins = [(a, b) for a in range(len(views)) for b in range(a + 1, len(views)) if bytes(views[a]) == bytes(views[b])]
    assert twins
    for a, b in twins:
        assert same_bits(frames[a], frames[b]), (a, b)
    # 3. permuted
    perm = [int(i) for i in np.random.default_rng(5100).permutation(len(views))]
    again = bflib.beamform_views(acq.bp, rf, [views[i] for i in perm], acq.filters)
    for i, p in enumerate(perm):
        assert same_bits(again[i], frames[p]), f"view {i} of the permuted push is not view {p}"
    # 4. subsets alone: every second view, and each view on its own
    subset = list(range(0, len(views), 2))
    for i, frame in zip(subset, bflib.beamform_views(acq.bp, rf, [views[i] for i in subset], acq.filters)):
        assert same_bits(frame, frames[i]), i
    for i in range(len(views)):
        assert same_bits(bflib.beamform_views(acq.bp, rf, [views[i]], acq.filters)[0], frames[i]), i
    # 5. against the single push of the block with that grid
    L.beamformer_hip_set_das_path(mode_for(name, 0))
    tol = cases.tolerance(acq)
    identical = 0
    for k, (acq_v, _, _, flags) in enumerate(refs):
        one = bflib.beamform(acq_v.bp, rf, acq_v.filters).copy()
        assert np.array_equal(np.isnan(one), np.isnan(frames[k]))
        ok = ~np.isnan(one)
        scale = np.abs(one[ok]).max()
        slack = tol * scale
        if flags is not None:
            # nearest: a tap within float rounding of k + 1/2 may fall either way in either kernel: the oracle's per-voxel budget, once each
            slack = slack + 2.02 * flags["budget"][ok]
        err = np.abs(one[ok] - frames[k][ok])
        assert (err <= slack).all(), f"view {k}: views kernel and single push differ by {err.max() / scale:.3e} of the frame maximum"
        identical += same_bits(one, frames[k])
    print(f"{name}: {identical} of {len(views)} views of the views kernel equal their single push bit for bit")


@pytest.mark.parametrize("name", DISPATCH_CASES)
def test_views_kernel_instances_no_other_case_dispatches(name, bflib):
    """parity of every view on the views kernel, as test_views_kernel's first step: the same views, reference and bars"""
    acq, rf, views, refs = prepared(name)
    bflib.library().beamformer_hip_set_das_path(mode_for(name, PREFER))
    described = bflib.describe_views(acq.bp, views, acq.filters)
    assert described.kernel_views == len(views) and described.das_launches == 1, described.reason
    frames = bflib.beamform_views(acq.bp, rf, views, acq.filters)
    info = bflib.last_views_info()
    assert info.view_count == len(views) and info.route.kernel_views == len(views) and info.route.das_launches == 1, info.route.reason
    check_parity(name, frames, refs, "views kernel")


def check_per_view(bflib, name, which, mode):
    """every view the single push of the block with that grid, bit for bit (same kernel, same DAS input), and parity"""
    L = bflib.library()
    acq, rf, views, refs = prepared(name, which)
    L.beamformer_hip_set_das_path(mode)
    described = bflib.describe_views(acq.bp, views, acq.filters)
    assert described.kernel_views == 0, described.reason
    frames = bflib.beamform_views(acq.bp, rf, views, acq.filters)
    info = bflib.last_views_info()
    assert info.route.kernel_views == 0 and info.route.das_launches == described.das_launches
    assert list(info.route.path[: len(views)]) == list(described.path[: len(views)])
    check_parity(name, frames, refs, "per-view route")
    for k, (acq_v, _, _, _) in enumerate(refs):
        one = bflib.beamform(acq_v.bp, rf, acq_v.filters)
        assert same_bits(one, frames[k]), f"view {k} is not the single push of the block with its grid"


@pytest.mark.parametrize("name", KERNEL_CASES)
def test_flag_0x800_runs_every_view_as_its_single_push(name, bflib):
    check_per_view(bflib, name, "kernel", mode_for(name, NO_KERNEL))


@pytest.mark.parametrize("name", PER_VIEW_CASES)
def test_blocks_the_views_kernel_does_not_take(name, bflib):
    check_per_view(bflib, name, "per_view", 0)


def test_a_mixed_push(bflib):
    """views the views kernel takes and views it does not, in one push: parity of all, the others their single push bit for bit"""
    from tests.das_push import mixed_views
    from oracle import binding
    acq = cases.make("rca_flash_none_tx")
    rf = noise_frames(acq, 1, 5300)[0]
    views = mixed_views(acq)
    bflib.library().beamformer_hip_set_das_path(PREFER)
    frames = bflib.beamform_views(acq.bp, rf, views, acq.filters)
    info = bflib.last_views_info()
    assert info.route.kernel_views == 2 and info.route.das_launches == 3, info.route.reason
    refs = [(on_grid(acq, v, rf),) + tuple(reference(binding, on_grid(acq, v, rf))) for v in views]
    check_parity(acq.name, frames, refs, "mixed route")
    assert same_bits(frames[1], frames[3])
    for k in (1, 3):
        assert same_bits(bflib.beamform(refs[k][0].bp, rf, acq.filters), frames[k]), k


@pytest.mark.parametrize("interp", ["linear", "cubic"])
def test_rows_that_end_inside_the_views(interp, bflib):
    """settle_index in the views kernel: on a plane whose oracle flip set is not empty (checked first, on the CPU) and on its deepest
    strip every view meets compare()'s rule, the flip-set rule included"""
    name = f"row_ends_{interp}"
    acq, rf, views, refs = prepared(name)
    acq_v, ref, _, flags = refs[0]
    v = compare(ref.copy(), ref, acq_v, flags, path=-1, label=f"{name}/oracle")          # the oracle against itself: counts its flip set
    assert v.flip_voxels >= 1, "the oracle's flip set is empty on the whole-plane view"
    assert int(bflib.describe_das(acq.bp, acq.filters)[4].row_ends) == 1
    bflib.library().beamformer_hip_set_das_path(PREFER)
    frames = bflib.beamform_views(acq.bp, rf, views, acq.filters)
    assert bflib.last_views_info().route.kernel_views == 3
    check_parity(name, frames[:2], refs[:2], "views kernel")
    assert not refs[2][1].any() and np.array_equal(frames[2], refs[2][1])          # past the ends of the rows: zeros, exactly


def test_ids_layout_and_info(bflib):
    L = bflib.library()
    acq, rf, views, _ = prepared("rca_cubic_real")
    single_push_acq = bflib.beamform(acq.bp, rf, acq.filters)
    before = frame_id(L).frame_id
    L.beamformer_hip_set_das_path(PREFER)
    described = bflib.describe_views(acq.bp, views, acq.filters)
    frames = bflib.beamform_views(acq.bp, rf, views, acq.filters)
    info = bflib.last_views_info()
    # consecutive ids in view order; the frame info describes the last view
    assert info.first_frame_id == before + 1 and info.view_count == len(views)
    last = frame_id(L)
    assert last.frame_id == before + len(views) and list(last.points) == list(views[-1].output_points)
    # last_views_info agrees with describe_views
    assert (info.route.kernel_views, info.route.das_launches, info.route.min_tiles) == (described.kernel_views, described.das_launches, described.min_tiles)
    assert list(info.route.path[: len(views)]) == list(described.path[: len(views)]) and info.route.reason == described.reason
    assert info.stage_kind[0] == 0xFFFF and info.stage_kind[info.stage_count - 1] == int(P.ShaderKind.DAS) and info.views_ms > 0
    # get_last_frames(K): oldest first, each at its own 64-byte-rounded size, contiguous
    sizes = [(f.nbytes + 63) // 64 * 64 for f in frames]
    raw = np.full(sum(sizes) // 4 + 16, -7.0, np.float32)
    assert L.beamformer_get_last_frames(raw.ctypes.data_as(C.c_void_p), sum(sizes), len(views))
    at = 0
    for f, size in zip(frames, sizes):
        assert np.array_equal(raw[at // 4: at // 4 + f.size].view(np.uint32), f.reshape(-1).view(np.uint32))
        at += size
    assert (raw[at // 4:] == -7.0).all()
    # every view's row of the timing table: the push's stage times divided by K
    table = P.ComputeStatsTable()
    assert L.beamformer_compute_timings(C.byref(table), -1)
    das = [i for i in range(info.stage_count) if info.stage_kind[i] == int(P.ShaderKind.DAS)][0]
    col = [i for i in range(table.shader_count) if table.shader_ids[i] == int(P.ShaderKind.DAS)][0]
    total = sum(table.times[(info.first_frame_id + k) % 32][col] for k in range(len(views)))
    assert abs(total - info.stage_ms[das] * 1e-3) <= 1e-5 * info.stage_ms[das] * 1e-3 + 1e-12
    t = P.HipFrameTimings()
    assert L.beamformer_hip_get_last_frame_timings(C.byref(t)) and t.das_voxels == int(np.prod(list(views[-1].output_points)))
    # a single push afterwards: the newest push is no views push any more
    L.beamformer_hip_set_das_path(0)
    assert same_bits(bflib.beamform(acq.bp, rf, acq.filters), single_push_acq)
    assert not L.beamformer_hip_get_last_views_info(C.byref(P.HipViewsInfo())) and bflib.last_error()[0] == E.InvalidAccess


def test_views_pushes_interleaved_with_single_pushes_and_a_burst_come_back_oldest_first(bflib):
    L = bflib.library()
    acq, _, views, _ = prepared("rca_cubic_real")
    views = views[1:4]
    rf = noise_frames(acq, 4, 5200)
    L.beamformer_hip_set_das_path(PREFER)
    own = [bflib.beamform_views(acq.bp, rf[k], views, acq.filters) for k in (0, 3)]
    singles = [single_push(bflib, acq, rf[k]) for k in range(4)]
    burst = bflib.beamform_burst(acq.bp, rf[1:3], acq.filters).copy()
    # single, views, burst of two, views: the union, oldest first
    array = (P.HipView * len(views))(*views)
    single_push(bflib, acq, rf[0])
    first = frame_id(L).frame_id
    assert L.beamformer_hip_push_data_views_with_compute(rf[0].ctypes.data_as(C.c_void_p), rf[0].nbytes, array, len(views), 0), bflib.last_error()
    assert L.beamformer_hip_push_data_burst_with_compute(rf[1:3].ctypes.data_as(C.c_void_p), rf[0].nbytes, 2, 0, 0), bflib.last_error()
    assert L.beamformer_hip_push_data_views_with_compute(rf[3].ctypes.data_as(C.c_void_p), rf[3].nbytes, array, len(views), 0), bflib.last_error()
    assert frame_id(L).frame_id == first + 2 * len(views) + 2
    expected = [singles[0]] + own[0] + [burst[0], burst[1]] + own[1]
    sizes = [(f.nbytes + 63) // 64 * 64 for f in expected]
    raw = np.zeros(sum(sizes) // 4, np.float32)
    assert L.beamformer_get_last_frames(raw.ctypes.data_as(C.c_void_p), raw.nbytes, len(expected))
    at = 0
    for k, (f, size) in enumerate(zip(expected, sizes)):
        assert np.array_equal(raw[at // 4: at // 4 + f.size].view(np.uint32), f.reshape(-1).view(np.uint32)), k
        at += size


def test_pair_counting_runs_per_view(bflib):
    L = bflib.library()
    acq, rf, views, refs = prepared("rca_cubic_real")
    t = P.HipFrameTimings()
    try:
        L.beamformer_hip_enable_pair_counting(1)
        L.beamformer_hip_set_das_path(PREFER)
        bflib.beamform_views(acq.bp, rf, views[:3], acq.filters)
        assert L.beamformer_hip_get_last_frame_timings(C.byref(t))
        pairs = int(t.das_pairs)
        L.beamformer_hip_set_das_path(0)
        bflib.beamform(refs[2][0].bp, rf, acq.filters)
        assert L.beamformer_hip_get_last_frame_timings(C.byref(t))
        assert pairs == int(t.das_pairs) > 0
    finally:
        L.beamformer_hip_enable_pair_counting(0)
