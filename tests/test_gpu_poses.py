"""DAS parity off the axes: the named cases under the ten poses of tests/poses.py -- tilted, spun, mirrored, turned and sheared grids,
a tilted array and one mounted the other way round -- through the C ABI against the CPU oracle on the same parameter block.  Reference
and bars are the existing ones (tests/parity.py reference() and compare(), cases.tolerance): no new tolerance.  Every test asserts
that the DAS path that ran is the one beamformer_hip_describe_das announced; tests/test_poses_host.py holds what that decision must
be, and the conditions under which a posed case is worth beamforming.

GENERAL poses (no exact zero survives): the "any position" kernels -- das.hip, das_factored.hip, das_tile.hip -- on tilted frames.
SPECIAL poses (the exact zeros survive): the gather, LDS-staged, HERCULES and block-staged kernels on the geometry their gates still
admit, with delays that fall where they used to rise.  Then the aperture count, the four fused multi-frame kernels (which restate
voxel-to-point) and 32 random poses of random draws."""
import dataclasses
import functools

import numpy as np
import pytest

from ogl_beamforming_amd import lib as bf
from ogl_beamforming_amd import params as P
from tests import cases, draws, poses
from tests import variants_cases as vc
from tests.das_kernel_cases import FACTORED, HERCULES, STAGED, TILE
from tests.das_push import box, check_burst, compare, inner, last_timings, noise_frames, on_grid, REACHED_DEPTH
from tests.parity import reference
from tests.scaffold import automatic_path  # noqa: F401

pytestmark = pytest.mark.gpu
I = P.InterpolationMode
NAMES = sorted(cases.CASES)


def pairs(pose_names, names):
    out = [(pose, name) for pose in pose_names for name in names]
    return dict(argnames="pose,name", argvalues=out, ids=[f"{pose}-{name}" for pose, name in out])


@functools.lru_cache(maxsize=None)
def posed_reference(name, pose):
    """(posed acquisition, oracle frame, oracle pair count, nearest flags) -- computed once per (case, pose), shared, left unchanged"""
    from oracle import binding
    binding.library()
    acq = poses.posed(name, pose)
    return (acq,) + tuple(reference(binding, acq))


@pytest.fixture(autouse=True)
def pair_counting_off(automatic_path, bflib):
    yield
    bflib.library().beamformer_hip_enable_pair_counting(0)


def check(bflib, name, pose, mode, want=None, label=None):
    """one frame of the posed case under a das path mode: the path that ran is the one described (and `want`, where given), the
    frame is the oracle's.  Returns the frame's timings."""
    acq, ref, _, flags = posed_reference(name, pose)
    L = bflib.library()
    L.beamformer_hip_set_das_path(mode)
    try:
        path, kernel, _, reasons, _ = bflib.describe_das(acq.bp, acq.filters)
        gpu = np.asarray(bflib.beamform(acq.bp, acq.rf, acq.filters)).copy()
        t = last_timings(bflib)
    finally:
        L.beamformer_hip_set_das_path(0)
    assert int(t.das_path) == path, (kernel, reasons)
    if want is not None:
        assert path == want, (kernel, reasons)
    compare(gpu, ref, acq, flags, path=path, label=label)
    return t


# ---- the automatic path: every case under every pose

@pytest.mark.parametrize(**pairs(poses.ALL, NAMES))
def test_automatic_path(pose, name, bflib):
    check(bflib, name, pose, 0)


# ---- the "any position" kernels under the GENERAL poses

@pytest.mark.parametrize(**pairs(poses.GENERAL, NAMES))
def test_general_kernel_one_thread_per_voxel(pose, name, bflib):
    check(bflib, name, pose, 0x11, want=0)


@pytest.mark.parametrize("split", [True, False], ids=["split", "whole"])
@pytest.mark.parametrize(**pairs(poses.GENERAL, FACTORED))
def test_factored_kernel(pose, name, split, bflib):
    check(bflib, name, pose, 0x04 if split else 0x14, want=3)


def check_block_staged(bflib, name, pose):
    t = check(bflib, name, pose, 0x14 | 0x100, want=5)
    assert int(t.tile_staged_chunks) + int(t.tile_gather_chunks) > 0


@pytest.mark.parametrize(**pairs(poses.GENERAL, TILE))
def test_block_staged_kernel_on_tilted_frames(pose, name, bflib):
    check_block_staged(bflib, name, pose)


# ---- the fast paths under the SPECIAL poses

@pytest.mark.parametrize(**pairs(poses.SPECIAL, sorted(STAGED)))
def test_lds_staged_kernel_checked_loop(pose, name, bflib, hooks):
    """mode 3 with every term range-checked: a position outside its staged window is counted"""
    hooks.set("STAGED_CHECKED")
    t = check(bflib, name, pose, 3, want=1 if name in cases.ROW_END_EVERY_PLANE else 2)
    assert int(t.staged_window_violations) == 0, "a term left its staged window: plan_staged's bound is wrong"


@pytest.mark.parametrize(**pairs(poses.SPECIAL, sorted(STAGED)))
def test_lds_staged_kernel_unchecked_loop(pose, name, bflib):
    """mode 3 as the library runs it: the waves the host bound clears run the loop without range checks"""
    check(bflib, name, pose, 3, want=1 if name in cases.ROW_END_EVERY_PLANE else 2)


@pytest.mark.parametrize("shape", ["5,4,5", "4,5,5", "6,4,5", "5,5,5", "4,6,5", "5,4,6", "4,5,6", "6,4,6", "5,5,6", "4,6,6"])
@pytest.mark.parametrize(**pairs(("flip_x", "combo"), ["rca_staged_auto", "rca_staged_cubic_short_rows"]))
def test_lds_staged_kernel_every_tile_and_window_shape(pose, name, shape, bflib, hooks):
    hooks.set("STAGED_SHAPE", shape)
    hooks.set("STAGED_CHECKED")
    t = check(bflib, name, pose, 3)
    assert int(t.das_path) in (1, 2) and int(t.staged_window_violations) == 0
    if name in cases.STAGED_SHAPES_TAKEN and shape in cases.STAGED_SHAPES_TAKEN[name]:
        assert int(t.das_path) == 2, "a mirror changes no spread: the shapes the unposed case takes are taken"
    if name == "rca_staged_auto" and shape in ("5,4,6", "4,5,6", "5,5,6", "4,6,6"):
        assert int(t.das_path) == 2          # as unposed: a 64-sample window holds its spread for tiles up to 32 voxels along the receive axis


@pytest.mark.parametrize(**pairs(poses.SPECIAL, sorted(STAGED)))
def test_gather_kernel(pose, name, bflib):
    """mode 2: automatic, but never staged -- the separable-delay gather kernel for linear interpolation, the factored one for cubic"""
    linear = posed_reference(name, pose)[0].bp.interpolation_mode == int(I.Linear)
    t = check(bflib, name, pose, 2, want=1 if linear else None)
    assert int(t.das_path) in (1, 3)


HERCULES_FORCED = {name: group for group in ("hercules_planes", "hercules_volumes") for name in poses.EXPECTED_FORCED[group]["cases"]}


@pytest.mark.parametrize(**pairs(poses.SPECIAL, HERCULES))
def test_hercules_aligned_kernel(pose, name, bflib):
    """mode 6: das_hercules.hip wherever its gate admits the pose (poses.EXPECTED_FORCED), the general kernel on the sheared volumes"""
    check(bflib, name, pose, 6, want=poses.expected_forced(HERCULES_FORCED[name], pose))


@pytest.mark.parametrize(**pairs(poses.SPECIAL, TILE))
def test_block_staged_kernel_on_mirrored_turned_and_sheared_frames(pose, name, bflib):
    check_block_staged(bflib, name, pose)


def test_block_staged_kernel_is_deterministic_under_a_pose(bflib):
    """forty frames of tile_near_field under `combo`, bit for bit (staged and gathered chunks)"""
    acq = posed_reference("tile_near_field", "combo")[0]
    L = bflib.library()
    L.beamformer_hip_set_das_path(0x14 | 0x100)
    first = np.asarray(bflib.beamform(acq.bp, acq.rf, acq.filters)).copy()
    assert int(last_timings(bflib).das_path) == 5
    for k in range(39):
        again = np.asarray(bflib.beamform(acq.bp, acq.rf, acq.filters))
        assert np.array_equal(first.view(np.uint32), again.view(np.uint32)), f"frame {k + 2} differs from the first"


# ---- the aperture test is geometry too

@pytest.mark.parametrize(**pairs(("tilt_both", "combo"), ["config4_small", "rca_vls_cw", "hercules_real", "forces"]))
def test_pair_count_matches_oracle(pose, name, bflib):
    acq, _, pairs_ref, _ = posed_reference(name, pose)
    L = bflib.library()
    L.beamformer_hip_enable_pair_counting(1)
    try:
        bflib.beamform(acq.bp, acq.rf, acq.filters)
        t = last_timings(bflib)
    finally:
        L.beamformer_hip_enable_pair_counting(0)
    assert pairs_ref > 0
    assert abs(int(t.das_pairs) - pairs_ref) <= max(4, 2e-4 * pairs_ref), (int(t.das_pairs), pairs_ref)


# ---- the fused multi-frame kernels restate voxel-to-point: one posed acquisition each

FUSED_POSES = ("tilt_both", "combo")
FUSED_CASE = "rca_cubic_real"          # of BURST_KERNEL_CASES and of tests/das_push.py's KERNEL_CASES: single frames run the general kernel
PREFER_VIEWS, NO_VIEWS = P.HIP_DAS_PATH_PREFER_VIEWS_KERNEL, P.HIP_DAS_PATH_NO_VIEWS_KERNEL


def fused_acquisition(pose):
    acq = poses.posed(FUSED_CASE, pose)
    acq.name = f"{FUSED_CASE}@{pose}"
    return acq


def oblique_views(acq):
    """the posed case's own grid, and through the UNPOSED case's volume: a plane spun about its vertical axis and shifted off axis
    (poses' spin_plane), a tilted sub-volume (tilt_grid) and a mirrored, sheared plane (flip_x, shear) -- all inside the depth range
    the case's RF rows reach"""
    lo, hi = box(cases.make(FUSED_CASE).bp)
    d = REACHED_DEPTH[FUSED_CASE]
    spun = bf.view((33, 1, 17), *inner(lo, hi, (0.1, 0.5, 0.1 * d), (0.9, 0.5, 0.9 * d)))
    tilted = bf.view((9, 6, 5), *inner(lo, hi, (0.2, 0.3, 0.3 * d), (0.8, 0.7, 0.8 * d)))
    mirrored = bf.view((5, 1, 7), *inner(lo, hi, (0.3, 0.5, 0.2 * d), (0.6, 0.5, 0.7 * d)))
    for view, pieces in ((spun, poses.POSES["spin_plane"]), (tilted, poses.POSES["tilt_grid"]), (mirrored, poses.POSES["flip_x"] + poses.POSES["shear"])):
        V = poses.matrix(view.das_voxel_transform)
        for piece in pieces:
            V, _ = piece(view, V, None)
        poses.store(view.das_voxel_transform, V)
    return [bf.view_of(acq.bp), spun, tilted, mirrored]


@functools.lru_cache(maxsize=None)
def prepared_views(pose, n):
    """(acquisition, n noise RF frames, views, refs[v][k]: the acquisition on view v's grid with RF k and the oracle's reference)"""
    from oracle import binding
    binding.library()
    acq = fused_acquisition(pose)
    rf = noise_frames(acq, n, 8000)
    views = oblique_views(acq)
    refs = []
    for v in views:
        row = []
        for k in range(n):
            acq_vk = on_grid(acq, v, rf[k])
            ref, _, flags = reference(binding, acq_vk)
            ok = np.isfinite(ref)
            assert ok.any() and np.abs(ref[ok]).max() > 0, "an oblique view is an empty image"
            row.append((acq_vk, ref, flags))
        refs.append(row)
    return acq, rf, views, refs


@pytest.mark.parametrize("pose", FUSED_POSES)
def test_burst_kernel(pose, bflib, oracle):
    check_burst(bflib, oracle, fused_acquisition(pose), 5, seed=8100, expect_kernel=True)


@pytest.mark.parametrize("route", ["views kernel", "per-view route"])
@pytest.mark.parametrize("pose", FUSED_POSES)
def test_views_push_with_oblique_views(pose, route, bflib):
    acq, rf, views, refs = prepared_views(pose, 1)
    kernel = route == "views kernel"
    bflib.library().beamformer_hip_set_das_path(PREFER_VIEWS if kernel else NO_VIEWS)
    described = bflib.describe_views(acq.bp, views, acq.filters)
    assert described.kernel_views == (len(views) if kernel else 0), described.reason
    frames = bflib.beamform_views(acq.bp, rf[0], views, acq.filters)
    info = bflib.last_views_info()
    assert info.route.kernel_views == described.kernel_views and info.route.das_launches == described.das_launches == (1 if kernel else len(views))
    for v, frame in enumerate(frames):
        acq_v, ref, flags = refs[v][0]
        compare(frame, ref, acq_v, flags, label=f"{acq.name}/{route}/view{v}")


@pytest.mark.parametrize("pose", FUSED_POSES)
def test_burst_views_push_with_oblique_views(pose, bflib):
    n = 5
    acq, rf, views, refs = prepared_views(pose, n)
    K = len(views)
    described = bflib.describe_burst_views(acq.bp, n, views, acq.filters)
    assert (described.rung, described.kernel_views, described.das_launches) == (1, K, 1), described.reason
    frames = bflib.beamform_burst_views(acq.bp, rf, views, acq.filters)
    info = bflib.last_burst_views_info()
    assert (info.frame_count, info.view_count, info.route.rung, info.route.kernel_views, info.route.das_launches) == (n, K, 1, K, 1), info.route.reason
    for v in range(K):
        for k in range(n):
            acq_vk, ref, flags = refs[v][k]
            compare(frames[v][k], ref, acq_vk, flags, label=f"{acq.name}/burst views fused kernel/view{v}/rf{k}")


@pytest.mark.parametrize("pose", FUSED_POSES)
def test_variants_push(pose, bflib, oracle):
    """tests/variants_cases.py's cubic IQ block with coherency weighting, posed: three candidates on the variants kernel"""
    acq = poses.apply(vc.block("cubic", iq=True, cw=True), pose)
    acq.name = f"{acq.name}@{pose}"
    variants = vc.candidates(acq.bp)
    bflib.library().beamformer_hip_set_das_path(vc.PREFER)
    described = bflib.describe_variants(acq.bp, variants, acq.filters)
    assert described.kernel_variants == 3 and described.das_launches == 1, described.reason
    frames = bflib.beamform_variants(acq.bp, acq.rf, variants, acq.filters).copy()
    info = bflib.last_variants_info()
    assert info.route.kernel_variants == 3 and info.route.fused_launches == 1 and info.route.das_launches == 1, info.route.reason
    for k, v in enumerate(variants):
        acq_v = dataclasses.replace(acq, bp=bf.with_variant(acq.bp, v))
        ref, _, flags = reference(oracle, acq_v)
        ok = np.isfinite(ref)
        assert ok.any() and np.abs(ref[ok]).max() > 0
        compare(frames[k], ref, acq_v, flags, label=f"{acq.name}/variants kernel/{k}")


# ---- random poses of random draws

RANDOM_PATHS = []          # (seed, kind of pose, das path mode, das path)


@pytest.mark.parametrize("seed", draws.POSED_SEEDS)
def test_random_pose(seed, bflib, oracle):
    """tests/draws.py draw_posed: the automatic path, the kernel a full-size frame of the kind gets with block staging asked for
    (0x110: no channel split), and the general kernel -- against the oracle, as tests/test_gpu_random.py compares its draws"""
    acq, _, what = draws.draw_posed(seed, describe=True)
    ref, _, flags = reference(oracle, acq)
    ok = np.isfinite(ref)
    assert ok.any() and np.abs(ref[ok]).max() > 0, "tests/test_poses_host.py keeps the seeds non-empty"
    L = bflib.library()
    seen = set()
    for mode in (0, 0x110, 1):
        L.beamformer_hip_set_das_path(mode)
        try:
            path = bflib.describe_das(acq.bp, acq.filters)[0]
            gpu = np.asarray(bflib.beamform(acq.bp, acq.rf, acq.filters)).copy()
            t = last_timings(bflib)
        finally:
            L.beamformer_hip_set_das_path(0)
        assert int(t.das_path) == path, (what, hex(mode))
        if (path, mode & 0x10) in seen:
            continue
        seen.add((path, mode & 0x10))
        RANDOM_PATHS.append((seed, what[1], mode, path))
        compare(gpu, ref, acq, flags, path=path, label=f"draw_posed/random_{what[1]}/{seed}/{mode:#x}")


def test_random_poses_reach_the_kernels_they_aim_at():
    """rotated draws run the general and the factored kernel; draws in special position reach a fast path as well"""
    if len({seed for seed, *_ in RANDOM_PATHS}) < len(draws.POSED_SEEDS):
        pytest.skip("needs the draws of this module in the same session")
    rotated = {p for _, kind, _, p in RANDOM_PATHS if kind == "rotation"}
    special = {p for _, kind, _, p in RANDOM_PATHS if kind == "special"}
    assert {0, 3} <= rotated and not rotated & {1, 2, 4}, sorted(RANDOM_PATHS)
    assert {0, 3} <= special and special & {1, 2, 4, 5}, sorted(RANDOM_PATHS)
