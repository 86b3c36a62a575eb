"""The named cases under the ten poses of tests/poses.py, on the CPU: what csrc/das_select.cpp decides for tilted, mirrored, turned and
sheared grids and arrays (beamformer_hip_describe_das needs no device), checked against the CPU oracle where the decision makes a claim
about the frame (row ends), and the conditions that keep the posed cases worth beamforming (a non-empty image, no collapse of the live
share).  tests/test_gpu_poses.py then compares the kernels' frames of the same (case, pose) pairs with the oracle."""
import functools

import numpy as np
import pytest

from ogl_beamforming_amd import lib
from ogl_beamforming_amd import params as P
from tests import cases, poses, staged_window

I = P.InterpolationMode
PAIRS = [(pose, name) for pose in poses.ALL for name in sorted(cases.CASES)]
PAIR_IDS = [f"{pose}-{name}" for pose, name in PAIRS]


@functools.lru_cache(maxsize=None)
def described(name, pose, mode=0):
    """(path, reasons, description struct) of the posed case under a das path mode"""
    acq = poses.posed(name, pose)
    L = lib.library()
    L.beamformer_hip_set_das_path(mode)
    try:
        path, _, _, reasons, d = lib.describe_das(acq.bp, acq.filters)
    finally:
        L.beamformer_hip_set_das_path(0)
    return path, reasons, d


@functools.lru_cache(maxsize=None)
def oracle_summary(name, pose):
    """(max |ref| over the finite voxels, live share, per z-plane: whether the oracle marks a term at a row end -- None for nearest) --
    computed once per pair, shared by the row-end and the vacuity tests"""
    from oracle import binding
    acq = poses.posed(name, pose)
    flags = {}
    ref, _ = binding.beamform(acq.bp, acq.rf, acq.filters, flags=flags)
    ok = np.isfinite(ref)
    marks = None
    if acq.bp.interpolation_mode != int(I.Nearest):
        marks = np.asarray(flags["near_half"]).reshape(ref.shape).any(axis=(1, 2))
    return (float(np.abs(ref[ok]).max()) if ok.any() else 0.0), poses.live_share(ref), marks


# ---- (a) selection

@pytest.mark.parametrize("pose,name", PAIRS, ids=PAIR_IDS)
def test_automatic_selection_under_a_pose(pose, name):
    """GENERAL: no separable, staged or aligned-grid kernel, each with its reason -- the factored kernel where the unposed case ran
    the gather, the staged or the factored kernel, the general kernel elsewhere.  SPECIAL: the unposed case's path, but for HERCULES
    volumes under a sheared z column (no transducer axis is a function of the output row alone there): the general kernel"""
    unposed = described(name, None)[0]
    path, reasons, _ = described(name, pose)
    if pose in poses.GENERAL:
        assert path == (3 if unposed in (1, 2, 3) else 0), (unposed, path, reasons)
        assert reasons[1] and reasons[2] and reasons[4], reasons
    else:
        volume = int(cases.make(name).bp.output_points[2]) > 1
        want = 0 if unposed == 4 and volume and pose in ("shear", "combo") else unposed
        assert path == want, (unposed, path, reasons)
    assert not reasons[path]


FORCED = [(group, pose, name) for group in sorted(poses.EXPECTED_FORCED) for pose in poses.ALL for name in poses.EXPECTED_FORCED[group]["cases"]]


@pytest.mark.parametrize("group,pose,name", FORCED, ids=[f"{g}-{p}-{n}" for g, p, n in FORCED])
def test_forced_selection_under_a_pose(group, pose, name):
    mode = poses.EXPECTED_FORCED[group]["mode"]
    path, reasons, _ = described(name, pose, mode)
    assert path == poses.expected_forced(group, pose), (hex(mode), path, reasons)


def test_the_forced_expectations_cover_their_families():
    """the case lists of poses.EXPECTED_FORCED are written down; this keeps them complete: every tile_* case the block-staged kernel
    takes unposed, every HERCULES-family case, every case of the staged parity tests"""
    from tests import das_kernel_cases
    E = poses.EXPECTED_FORCED
    assert set(E["tile"]["cases"]) == {n for n in cases.CASES if n.startswith("tile_") and described(n, None, 0x114)[0] == 5}
    assert set(E["hercules_planes"]["cases"]) | set(E["hercules_volumes"]["cases"]) == set(das_kernel_cases.HERCULES)
    assert all(int(cases.make(n).bp.output_points[2]) == 1 for n in E["hercules_planes"]["cases"])
    assert all(int(cases.make(n).bp.output_points[2]) > 1 for n in E["hercules_volumes"]["cases"])
    assert set(E["staged"]["cases"]) | set(E["staged_every_plane_rerouted"]["cases"]) == set(das_kernel_cases.STAGED)
    assert set(E["staged_every_plane_rerouted"]["cases"]) == set(cases.ROW_END_EVERY_PLANE)


@pytest.mark.parametrize("mode", [0, 3])
@pytest.mark.parametrize("pose", ["flip_x", "flip_y", "array_half_turn"])
def test_a_mirror_changes_no_staged_plan(pose, mode):
    """tile shape and window of every staged plan are the unposed case's: a mirror changes no delay spread"""
    seen = 0
    for name in sorted(cases.CASES):
        path, _, d = described(name, None, mode)
        if path != 2:
            continue
        seen += 1
        posed_path, reasons, e = described(name, pose, mode)
        assert posed_path == 2, (name, reasons)
        assert (int(e.u_shift), int(e.v_shift), int(e.window_samples)) == (int(d.u_shift), int(d.v_shift), int(d.window_samples)), name
    assert seen >= (9 if mode == 0 else 12)


# ---- (b) row ends

# (nearest interpolation: the oracle marks rounding boundaries there, not row ends)
INTERPOLATED = {name for name in cases.CASES if cases.make(name).bp.interpolation_mode != int(I.Nearest)}
INTERPOLATED_PAIRS = [(pose, name) for pose, name in PAIRS if name in INTERPOLATED]


@pytest.mark.parametrize("pose,name", INTERPOLATED_PAIRS, ids=[f"{pose}-{name}" for pose, name in INTERPOLATED_PAIRS])
def test_no_row_end_code_only_where_the_oracle_marks_no_row_end(pose, name):
    """soundness of plane_index_bounds off the axes: row_ends == 0 removes the row-end code from the launch, so the oracle then marks
    a term within float rounding of an end of its RF row at no voxel (the bound is conservative: it also holds on the planes the
    row-end rule hands to the kernel behind a staged one)"""
    if int(described(name, pose)[2].row_ends) == 0:
        marked = np.flatnonzero(oracle_summary(name, pose)[2])
        assert marked.size == 0, f"row_ends 0, yet the oracle marks row-end terms on planes {marked.tolist()}"


@pytest.mark.parametrize("pose", poses.ALL)
def test_short_row_cases_keep_their_row_end_code(pose):
    """every *_short_rows case: where the unposed description says row_ends == 1 the posed one says so; where the unposed case hands
    its row-end planes to the kernel behind the staged one (row_ends 0 on the staged launch, row_end_planes > 0), the posed case does
    that or runs row-end code itself"""
    names = [n for n in sorted(cases.CASES) if n.endswith("_short_rows")]
    assert len(names) == 6
    for name in names:
        d0, d = described(name, None)[2], described(name, pose)[2]
        assert int(d0.row_ends) == 1 or int(d0.row_end_planes) > 0, name
        if int(d0.row_ends) == 1:
            assert int(d.row_ends) == 1, name
        else:
            assert int(d.row_ends) == 1 or int(d.row_end_planes) > 0, name


@pytest.mark.parametrize("pose", poses.SPECIAL)
def test_row_end_planes_survive_the_special_poses(pose):
    for name in sorted(cases.EXPECTED_ROW_END_PLANES):
        path0 = described(name, None)[0]
        path, _, d = described(name, pose)
        if path == path0:
            assert int(d.row_end_planes) > 0, name


# ---- (c) staged windows

@functools.lru_cache(maxsize=None)
def window_run(seed, pose):
    acq, cubic = staged_window.property_draw(seed)
    poses.apply(acq, pose)
    try:
        held, reason = staged_window.window_holds(acq, cubic)
    except AssertionError as e:
        return "failed", str(e)
    return ("held" if held else "declined"), reason


WINDOW_SEEDS = range(12)


@pytest.mark.parametrize("pose", poses.SPECIAL)
@pytest.mark.parametrize("seed", WINDOW_SEEDS)
def test_staged_window_holds_every_tile_under_a_special_pose(seed, pose):
    outcome, text = window_run(seed, pose)
    assert outcome != "failed", text


def test_the_staged_window_property_is_not_passed_by_declining():
    taken = sum(window_run(seed, pose)[0] == "held" for seed in WINDOW_SEEDS for pose in poses.SPECIAL)
    assert taken >= 40, f"the staged kernel was taken in {taken} of {len(WINDOW_SEEDS) * len(poses.SPECIAL)} (seed, pose) runs"


# ---- (d) the poses are not vacuous

@pytest.mark.parametrize("pose,name", PAIRS, ids=PAIR_IDS)
def test_a_posed_case_is_worth_beamforming(pose, name):
    """a condition on the inputs, not a tolerance: the oracle's frame is not empty and its live share (finite, non-zero voxels) is at
    most 0.2 below the unposed case's.  A pose that breaks this is changed, not the cap."""
    peak, share, _ = oracle_summary(name, pose)
    assert peak > 0
    assert share >= oracle_summary(name, None)[1] - 0.2, (share, oracle_summary(name, None)[1])


def test_draw_posed_seeds_are_worth_beamforming():
    """the 32 seeds of tests/test_gpu_poses.py's random poses meet the same condition against their unposed draw, and cover both kinds
    of pose and all three generators"""
    from oracle import binding
    from tests import draws
    kinds = set()
    for seed in draws.POSED_SEEDS:
        acq, base, what = draws.draw_posed(seed, describe=True)
        ref = binding.beamform(acq.bp, acq.rf, acq.filters)[0]
        ref0 = binding.beamform(base.bp, base.rf, base.filters)[0]
        ok = np.isfinite(ref)
        assert ok.any() and np.abs(ref[ok]).max() > 0, (seed, what)
        assert poses.live_share(ref) >= poses.live_share(ref0) - 0.2, (seed, what, poses.live_share(ref), poses.live_share(ref0))
        kinds.add(what[:2])
    assert len(draws.POSED_SEEDS) == 32 and len(set(draws.POSED_SEEDS)) == 32
    assert {k[0] for k in kinds} == {"draw", "draw_plane", "draw_tile"} and {k[1] for k in kinds} == {"rotation", "special"}, kinds
