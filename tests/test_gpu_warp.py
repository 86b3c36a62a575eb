"""The warp on the device (beamformer_hip_warp_last_frames; csrc/warp.hip) and the loop it closes: correlate -> displacements -> warp ->
gram.  The ensembles and grids are those of tests/test_gpu_ensemble.py and the NaN plane of the metrics tests, and two grids more:
"deep", 37 x 19 x 11 -- the kernel's tile in a volume is 8 x 8 x 4 voxels (tests/warp_ref.py: tile_of), so this one spans at least two
tiles and a ragged remainder of 5, 3 and 3 voxels on x, y and z -- and "wide", a plane of 96 x 1 x 96, 6 x 6 tiles of 16 x 16.  Both
hold more voxels than the 4096 of the kernel's LDS budget: a tile's source box is cut to the frame, so only on such grids can a box
exceed the budget and the block fall back to the direct path by itself.  On the other grids every tile is staged whatever the field
(the square's 4096 voxels ARE the budget), and the direct path is reached through das path flag WarpDirect alone.  Which tiles take
which path is worked out from the field (tests/warp_ref.py: tile_boxes) and asserted, not left to a seed.  The expected values are
the numpy reference (tests/warp_ref.py) applied to the downloaded source frames.

The bar is derived, not measured: tests/warp_ref.py returns it with the values and its docstring has the derivation.  Ids, grids,
kinds, tags and every case the definition makes exact are asked exactly.  Every test prints what it measured -- the worst error as a
share of its bound -- before it asserts.

WORST SHARE of the bound over this file on an MI355X: see DESIGN.md 3.7g."""
import numpy as np
import pytest

from ogl_beamforming_amd import lib as bf
from ogl_beamforming_amd import params as P
from tests import warp_ref as ref
from tests.frame_info import newest_info
from tests.ring_frames import warp_block_of as block_of, check_warp, CLAMP, CUBIC, ensemble, LINEAR, OWN, WARP_ZERO as ZERO
from tests.scaffold import automatic_path  # noqa: F401

pytestmark = pytest.mark.gpu
MODES = [(LINEAR, ZERO), (LINEAR, CLAMP), (CUBIC, ZERO), (CUBIC, CLAMP)]
GRIDS = ["plane", "square", "volume", "real", "nan", "deep", "wide"]


def frames_of(which, K):
    """K frames of the grid (tests/ring_frames.py's ensemble; "deep", "wide": the same by this file's blocks): (frames (K, Z, Y, X), ids)"""
    if which not in OWN:
        return ensemble(which, K)
    acq = block_of(which)
    rf = np.random.default_rng(7600 + K).normal(0.0, 1.0, (K,) + acq.rf.shape).astype(acq.rf.dtype)
    frames = bf.beamform(acq.bp, rf[0], acq.filters).copy()[None] if K == 1 else bf.beamform_burst(acq.bp, rf, acq.filters).copy()
    newest = int(newest_info(bf.library()).frame_id)
    return frames, list(range(newest - K + 1, newest + 1))


def extent_of(frames):
    return frames.shape[3], frames.shape[2], frames.shape[1]


# ---- the fields of the parity cases: dict(field (K, Nz, Ny, Nx, 3), nodes, node_first, node_step) ----

def rigid(frames, seed, reach=3.0, beyond=True, deeper=0.0):
    """a sub-voxel shift per frame, multiples of 1/8, different per frame; beyond: every third frame (from the second on) lies beyond
    the frame along one axis, so that its whole output is edge; deeper: added to every z component"""
    K, extent = len(frames), extent_of(frames)
    rng = np.random.default_rng(seed)
    d = rng.integers(int(-8 * reach), int(8 * reach) + 1, (K, 3)) / 8.0
    d[:, 2] += deeper
    for n in range(1, K if beyond else 0, 3):
        axis = (0, 2, 1)[(n // 3) % 3]
        if extent[axis] > 1:
            d[n, axis] = (extent[axis] + 2.625) * (1 if n % 2 else -1)
    return dict(field=d.astype(np.float32).reshape(K, 1, 1, 1, 3), nodes=(1, 1, 1), node_first=(0, 0, 0), node_step=(1, 1, 1))


def lattice(frames, seed, exact=False, deeper=0.0):
    """two nodes on every axis of more than one point, inside the frame: outside them the field is constant.  exact: a step of 8 voxels
    from an integer, values in multiples of 1/8 -- every position is then a float32 number and the reference's floor is the device's;
    deeper: added to every z component"""
    K, extent = len(frames), extent_of(frames)
    rng = np.random.default_rng(seed)
    nodes = tuple(2 if e > 1 else 1 for e in extent)
    if exact:
        first, step = tuple(float(e // 4) for e in extent), tuple(8.0 for e in extent)
        field = rng.integers(-8, 9, (K, nodes[2], nodes[1], nodes[0], 3)) / 8.0
        field[..., 2] += deeper
    else:
        first, step = tuple(0.25 * e + 0.3 for e in extent), tuple(max(1.0, 0.45 * e) for e in extent)
        field = rng.uniform(-2.0, 2.0, (K, nodes[2], nodes[1], nodes[0], 3))
    return dict(field=field.astype(np.float32), nodes=nodes, node_first=first, node_step=step)


def steep(frames, seed):
    """three nodes an axis of +- 40 voxels.  (On the square every tile is staged all the same: a box is cut to the frame, and the
    square's 4096 voxels are the budget.)"""
    K, extent = len(frames), extent_of(frames)
    rng = np.random.default_rng(seed)
    nodes = tuple(3 if e > 1 else 1 for e in extent)
    field = rng.uniform(-40.0, 40.0, (K, nodes[2], nodes[1], nodes[0], 3))
    return dict(field=field.astype(np.float32), nodes=nodes, node_first=(0, 0, 0), node_step=tuple(max(1.0, (e - 1) / 2.0) for e in extent))


def wild(frames, seed):
    """a field that sends some tiles of a launch down the direct path and leaves others staged: nodes a tile apart from voxel 0, the
    two node planes at the low end of x within +- 1 voxel, the others alternating between +- A voxels (+- 2) from node to node on
    every axis -- between two such nodes the displacement sweeps 2 A voxels across one tile, so the tile's reads span the frame.
    A = 40 in a volume; 90 on a plane, where the frame is 96 voxels an axis and a sweep of 80 leaves boxes on both sides of the budget"""
    K, extent = len(frames), extent_of(frames)
    rng = np.random.default_rng(seed)
    tile = ref.tile_of(extent)
    nodes = tuple(-(-e // t) + 1 if e > 1 else 1 for e, t in zip(extent, tile))
    iz, iy, ix = np.meshgrid(np.arange(nodes[2]), np.arange(nodes[1]), np.arange(nodes[0]), indexing="ij")
    sign = np.where((ix + iy + iz) % 2 == 0, 1.0, -1.0)[None, ..., None]
    field = sign * (40.0 if min(extent) > 1 else 90.0) + rng.uniform(-2.0, 2.0, (K, nodes[2], nodes[1], nodes[0], 3))
    field[:, :, :, :2, :] = rng.uniform(-1.0, 1.0, (K, nodes[2], nodes[1], 2, 3))
    return dict(field=field.astype(np.float32), nodes=nodes, node_first=(0, 0, 0), node_step=tuple(float(t) for t in tile))


def paths_of(frames, case, interpolation):
    """(staged, direct): the tiles of the call whose source box is clear of the budget on either side, all frames together; no box may
    lie within a voxel an axis of the budget, where the device's float32 positions could decide otherwise than the reference's"""
    staged = direct = 0
    for n in range(len(frames)):
        boxes = ref.tile_boxes(frames[n].shape, case["field"][n], case["nodes"], case["node_first"], case["node_step"], interpolation)
        assert not ((boxes > 0.8 * ref.BOX_VOXELS) & (boxes < 1.2 * ref.BOX_VOXELS)).any(), boxes
        staged, direct = staged + int((boxes <= ref.BOX_VOXELS).sum()), direct + int((boxes > ref.BOX_VOXELS).sum())
    return staged, direct


def rotations_of(K, seed):
    rng = np.random.default_rng(seed)
    r = np.exp(-1j * rng.uniform(-np.pi, np.pi, K)) * rng.uniform(0.5, 1.5, K)
    return r.astype(np.complex64)


# ---- parity: every grid x both interpolations x both edges at K = 1, 3, 17 ----

@pytest.mark.parametrize("interpolation,edge", MODES)
@pytest.mark.parametrize("K", [1, 3, 17])
@pytest.mark.parametrize("which", GRIDS)
def test_values_against_the_reference(which, K, interpolation, edge, bflib):
    seed = 9600 + 7 * K + 2 * interpolation + edge
    cplx = which != "real"
    worst, shares = 0.0, []
    nan = which == "nan"
    frames, ids = frames_of(which, K)
    # a rigid sub-voxel shift per frame.  (The NaN plane's holes are its flanks, a wedge that narrows with depth and leaves 0.58 of
    # the voxels finite; every tap under a hole poisons an output, the cubic's four taps three columns of a row.  There the shifts stay
    # below a voxel sideways, none lies beyond the frame -- a clamped flank is a frame of NaN --, and all read 12 voxels deeper, where
    # the wedge is narrower: the reference is then finite on 0.56 to 0.73 of the floats, worked out from the geometry beforehand)
    case = rigid(frames, seed, 0.875, beyond=False, deeper=12.0) if nan else rigid(frames, seed)
    _, _, w, s = check_warp(which, frames, ids, case, None, interpolation, edge, tag=3, what=which + " rigid", same_masks=True)
    worst, shares = max(worst, w), shares + [s]
    # a lattice inside the frame, with rotations on the complex grids (real frames: real factors)
    frames, ids = frames_of(which, K)
    rot = rotations_of(K, seed) if cplx else rotations_of(K, seed).real.astype(np.complex64)
    _, _, w, s = check_warp(which, frames, ids, lattice(frames, seed + 1, exact=nan, deeper=12.0 if nan else 0.0), rot, interpolation, edge, tag=4, what=which + " lattice, rotated", same_masks=nan)
    worst, shares = max(worst, w), shares + [s]
    if which == "square":
        frames, ids = frames_of(which, K)
        _, _, w, s = check_warp(which, frames, ids, steep(frames, seed + 2), None, interpolation, edge, what=which + " 3 nodes an axis of +- 40 (staged)")
        worst, shares = max(worst, w), shares + [s]
    if which in ("deep", "wide"):
        # the automatic fallback: in every frame of the launch some tiles' boxes exceed the budget and others do not
        frames, ids = frames_of(which, K)
        case = wild(frames, seed + 2)
        staged, direct = paths_of(frames, case, interpolation)
        print(f"  {which} wild: {staged} tiles staged, {direct} direct")
        assert staged >= K and direct >= K
        _, _, w, s = check_warp(which, frames, ids, case, None, interpolation, edge, what=which + " wild (staged and direct tiles in one launch)")
        worst, shares = max(worst, w), shares + [s]
    print(f"  {which}, K {K}: worst share of the bound {worst:.4f}; compared shares {['%.3f' % s for s in shares]}")
    # the comparison leaves out only floats where the reference itself is not finite: none on the finite grids
    assert all(s > 0.5 for s in shares) if nan else all(s == 1.0 for s in shares)


# ---- what the definition makes exact ----

@pytest.mark.parametrize("which", ["plane", "volume", "real", "deep"])
def test_a_zero_field_returns_the_sources(which, bflib):
    for interpolation, edge in MODES:
        frames, ids = frames_of(which, 3)
        case = dict(field=np.zeros((3, 1, 1, 1, 3), np.float32), nodes=(1, 1, 1), node_first=(0, 0, 0), node_step=(1, 1, 1))
        out, _, _, _ = check_warp(which, frames, ids, case, None, interpolation, edge, what=which + " zero field")
        assert np.array_equal(out, frames)                              # as float values: -0 may come back +0


@pytest.mark.parametrize("which,shift", [("plane", (3, 0, -2)), ("deep", (-5, 2, 1)), ("real", (-1, 0, 1)), ("square", (17, 0, -16))])
def test_an_integer_shift_moves_the_interior_exactly(which, shift, bflib):
    for interpolation in (LINEAR, CUBIC):
        frames, ids = frames_of(which, 2)
        case = dict(field=np.array([shift, [-s for s in shift]], np.float32).reshape(2, 1, 1, 1, 3), nodes=(1, 1, 1), node_first=(0, 0, 0), node_step=(1, 1, 1))
        out, _, _, _ = check_warp(which, frames, ids, case, None, interpolation, ZERO, what=f"{which} moved by {shift}")
        Z, Y, X = frames.shape[1:]
        for n, sign in ((0, 1), (1, -1)):
            dx, dy, dz = (sign * s for s in shift)
            # the voxels whose whole support lies inside the frame: taps -1 .. +2 around v + d
            x0, x1 = max(0, 1 - dx), min(X, X - 2 - dx)
            z0, z1 = max(0, 1 - dz), min(Z, Z - 2 - dz)
            y0, y1 = (0, 1) if Y == 1 else (max(0, 1 - dy), min(Y, Y - 2 - dy))
            assert x1 > x0 and y1 > y0 and z1 > z0
            moved = frames[n, z0 + dz:z1 + dz, y0 + dy:y1 + dy, x0 + dx:x1 + dx]
            assert np.array_equal(out[n, z0:z1, y0:y1, x0:x1], moved)


@pytest.mark.parametrize("which", ["square", "deep"])
def test_a_constant_lattice_gives_the_bytes_of_the_rigid_call_and_y_means_nothing_on_a_plane(which, bflib):
    rng = np.random.default_rng(9700)
    d = (rng.integers(-20, 21, (3, 3)) / 8.0).astype(np.float32)
    for interpolation, edge in MODES:
        frames, ids = frames_of(which, 3)
        case = dict(field=d.reshape(3, 1, 1, 1, 3), nodes=(1, 1, 1), node_first=(0, 0, 0), node_step=(1, 1, 1))
        one, _, _, _ = check_warp(which, frames, ids, case, None, interpolation, edge, what=which + " rigid")
        frames2, ids2 = frames_of(which, 3)
        assert frames2.tobytes() == frames.tobytes()
        nodes = (3, 1, 2) if which == "square" else (3, 2, 2)
        field = np.broadcast_to(d.reshape(3, 1, 1, 1, 3), (3, nodes[2], nodes[1], nodes[0], 3)).copy()
        case = dict(field=field, nodes=nodes, node_first=(2.5, 1.0, 3.25), node_step=(7.3, 2.0, 1.9))
        many, _, _, _ = check_warp(which, frames2, ids2, case, None, interpolation, edge, what=which + " constant lattice")
        assert many.tobytes() == one.tobytes()
        if which == "square":
            frames3, ids3 = frames_of(which, 3)
            other = d.copy()
            other[:, 1] = [7.5, -300.0, 65536.0]
            case = dict(field=other.reshape(3, 1, 1, 1, 3), nodes=(1, 1, 1), node_first=(0, 0, 0), node_step=(1, 1, 1))
            plane, _, _, _ = check_warp(which, frames3, ids3, case, None, interpolation, edge, what=which + " another y component")
            assert plane.tobytes() == one.tobytes()


# ---- determinism: an output depends on its own source, field and rotation alone ----

@pytest.mark.parametrize("which", ["square", "deep", "wide"])
def test_an_output_does_not_depend_on_count_on_a_repeat_or_on_the_path(which, bflib):
    L = bflib.library()
    for interpolation, edge in ((LINEAR, CLAMP), (CUBIC, ZERO)):
        frames, ids = frames_of(which, 5)
        case = lattice(frames, 9800)
        rot = rotations_of(5, 9801)
        five, _, _, _ = check_warp(which, frames, ids, case, rot, interpolation, edge, what=which + ", five")
        frames2, ids2 = frames_of(which, 5)
        assert frames2.tobytes() == frames.tobytes()
        alone = dict(case, field=case["field"][4:])
        one, _, _, _ = check_warp(which, frames2[4:], ids2[4:], alone, rot[4:], interpolation, edge, what=which + ", the newest alone")
        assert one[0].tobytes() == five[4].tobytes()
        frames3, ids3 = frames_of(which, 5)
        again, _, _, _ = check_warp(which, frames3, ids3, case, rot, interpolation, edge, what=which + ", again")
        assert again.tobytes() == five.tobytes()
        # every tile down the direct path: the same bytes
        frames4, ids4 = frames_of(which, 5)
        L.beamformer_hip_set_das_path(P.HIP_DAS_PATH_WARP_DIRECT)
        direct, _, _, _ = check_warp(which, frames4, ids4, case, rot, interpolation, edge, what=which + ", direct")
        L.beamformer_hip_set_das_path(0)
        differing = int((direct.view(np.uint32) != five.view(np.uint32)).sum())
        print(f"  staged against direct: {differing} of {five.view(np.uint32).size} words differ")
        assert direct.tobytes() == five.tobytes()


def test_a_voxel_keeps_its_bytes_when_the_field_of_its_tile_neighbours_changes(bflib):
    """The wide plane (96 x 1 x 96, 6 x 6 tiles) under a lattice of 7 x 1 x 7 nodes 16 voxels apart.  Field A is smooth: every tile's box
    is far below the budget, every tile staged.  Field B is wild()'s: it keeps A's nodes at x = 0 and x = 16 and alternates between
    +- 90 voxels from x = 32 on.  The voxels with x <= 16 see the same displacement under both -- at x = 16 the lerp's fraction is 0
    --, but the column x = 16 belongs to the tiles of x = 16 .. 31, whose source boxes under B exceed the budget: staged under A,
    direct under B (both worked out from the fields and asserted), the same bytes."""
    rng = np.random.default_rng(9900)
    for interpolation, edge in MODES:
        frames, ids = frames_of("wide", 2)
        case_b = wild(frames, 9901 + interpolation)
        assert case_b["nodes"] == (7, 1, 7) and case_b["node_step"] == (16.0, 1.0, 16.0)
        A = rng.uniform(-1.5, 1.5, case_b["field"].shape).astype(np.float32)
        A[:, :, :, :2, :] = case_b["field"][:, :, :, :2, :]
        case_a = dict(case_b, field=A)
        for n in range(2):
            boxes_a = ref.tile_boxes(frames[n].shape, A[n], case_a["nodes"], case_a["node_first"], case_a["node_step"], interpolation)
            boxes_b = ref.tile_boxes(frames[n].shape, case_b["field"][n], case_b["nodes"], case_b["node_first"], case_b["node_step"], interpolation)
            assert boxes_a.max() < 0.8 * ref.BOX_VOXELS                                        # A: every tile staged
            assert boxes_b[:, 0, 0].max() < 0.8 * ref.BOX_VOXELS                               # B: the tiles of x = 0 .. 15 staged,
            assert boxes_b[:, 0, 1:].min() > 1.2 * ref.BOX_VOXELS                              # ... every other tile direct
        smooth, _, _, _ = check_warp("wide", frames, ids, case_a, None, interpolation, edge, what="smooth: staged")
        frames2, ids2 = frames_of("wide", 2)
        assert frames2.tobytes() == frames.tobytes()
        mixed, _, _, _ = check_warp("wide", frames2, ids2, case_b, None, interpolation, edge, what="wild from x = 32: direct from x = 16")
        assert np.ascontiguousarray(mixed[..., :17]).tobytes() == np.ascontiguousarray(smooth[..., :17]).tobytes()
        assert mixed[..., 32:].tobytes() != smooth[..., 32:].tobytes()


# ---- the loop closes: correlate -> displacements -> warp -> gram ----

def test_the_motion_loop_closes(bflib):
    acq = block_of("square")
    frames, ids = frames_of("square", 1)
    # frame 1 is frame 0 moved by d = (2, 0, -1) on the device: g[v] = ref[v - d], so g[v + d] = ref[v] -- taps (0, 0, 0, 0, 1) move a
    # frame by +2 voxels along x, taps (1, 0, 0) by -1 along z
    d = (2, 0, -1)
    bflib.convolve_last_frames(1, [np.array([0, 0, 0, 0, 1], np.float32), None, np.array([1, 0, 0], np.float32)])
    pair = bflib.get_last_frames(acq.bp, 2).copy()
    assert np.array_equal(pair[0], frames[0]) and np.array_equal(pair[1, 0:-1, :, 2:], pair[0, 1:, :, :-2])
    box = bflib.frame_region((8, 0, 8), (48, 1, 48))
    before, _, _ = bflib.gram_last_frames(2, box)
    tables, info, _ = bflib.correlate_last_frames(2, 0, (3, 0, 3))
    found = bflib.displacements_from_correlation(tables, (3, 0, 3))[0]
    print(f"  displacements {found['displacement'].tolist()}, shifts {found['shift'].tolist()}, coefficients {found['coefficient'].tolist()}")
    assert found["shift"].tolist() == [[0, 0, 0], list(d)]
    # the integer peaks, as they are: the warped frame IS the reference away from the edges
    first, _ = bflib.warp_last_frames(2, found["shift"].astype(np.float32), interpolation=CUBIC, edge=CLAMP)
    warped = bflib.get_last_frames(acq.bp, 2).copy()
    assert np.array_equal(warped[0], pair[0]) and np.array_equal(warped[1, 4:-4, :, 4:-4], pair[0, 4:-4, :, 4:-4])
    exact, _, _ = bflib.gram_last_frames(2, box)
    # the displacements with their sub-voxel fit, as they are, on the pair again (the four newest frames: pair, warped pair)
    bflib.mix_last_frames(4, np.array([[1, 0, 0, 0], [0, 1, 0, 0]], np.complex64))
    assert np.array_equal(bflib.get_last_frames(acq.bp, 2), pair)
    bflib.warp_last_frames(2, found["displacement"], rotations=np.exp(-1j * found["phase"]), interpolation=CUBIC, edge=CLAMP)
    after, _, _ = bflib.gram_last_frames(2, box)
    c = [abs(G[0, 1]) / np.sqrt(G[0, 0].real * G[1, 1].real) for G in (before, exact, after)]
    print(f"  |G01| / sqrt(G00 G11) over the interior: {c[0]:.4f} before, {c[1]:.6f} by the integer peaks, {c[2]:.4f} by the fitted displacements")
    assert c[1] > 0.999999 and c[2] > c[0] and c[1] > c[0]


# ---- ring bookkeeping ----

def test_the_outputs_are_ordinary_frames(bflib):
    frames, ids = frames_of("square", 3)
    case = dict(field=np.array([[0.5, 0, -1.25], [-2.125, 0, 0.375], [1, 0, 1]], np.float32).reshape(3, 1, 1, 1, 3), nodes=(1, 1, 1),
                node_first=(0, 0, 0), node_step=(1, 1, 1))
    out, first, _, _ = check_warp("square", frames, ids, case, rotations_of(3, 9951), CUBIC, CLAMP, tag=6, what="square")
    rows, _ = bflib.score_last_frames(3)
    for n in range(3):
        assert np.array_equal(bflib.copy_frame(first + n).view(np.uint32), out[n].view(np.uint32))
        assert int(rows[n].frame_id) == first + n and int(rows[n].image_plane_tag) == 6
        assert abs(float(rows[n].max_abs) - float(np.abs(out[n]).max())) <= 1e-5 * float(np.abs(out[n]).max())
    peaks, records, _ = bflib.find_peaks_last_frames(3, [0.5 * float(r.max_abs) for r in rows], 16)
    assert [int(p.frame_id) for p in peaks] == [first, first + 1, first + 2] and all(int(p.found) >= 1 for p in peaks)
    # the call does not synchronise when it is not timed; what follows on the stream sees the frames
    frames, ids = frames_of("square", 3)
    first, ms = bflib.warp_last_frames(3, case["field"], timed=False)
    assert ms == 0 and first == ids[-1] + 1
    values = [ref.warp(frames[n], case["field"][n]) for n in range(3)]
    got = bflib.get_last_frames(block_of("square").bp, 3)
    assert all(ref.share_of_bound(got[n], *values[n])[1] for n in range(3))
