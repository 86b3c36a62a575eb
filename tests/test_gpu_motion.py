"""The shift correlation on the device (beamformer_hip_correlate_last_frames; csrc/correlate.hip) and the host helper behind it.  Frames
are produced by ordinary pushes of the small blocks tests/test_gpu_ensemble.py defines and downloaded with beamformer_get_last_frames;
the expected values are the numpy reference (tests/motion_ref.py) applied to those downloaded arrays.

The bars are derived, not measured (tests/motion_ref.py returns them with the values): the products of widened floats are exact, a term
is one rounding and the running sum `terms` more: (terms + 2) 2^-53 sum (|r| + |i|)(|r| + |i|) over the terms, the two factors those of
the product.  `terms`, ids, grids and every zero the definition promises are asked exactly.  Every test prints what it measured before
it asserts."""
import numpy as np
import pytest

from ogl_beamforming_amd import params as P
from tests import motion_ref as ref
from tests.ring_frames import block, BOXES, check_correlate as check_call, DOUBLES, ensemble, GRIDS, regions_of
from tests.scaffold import automatic_path  # noqa: F401

pytestmark = pytest.mark.gpu
NAN_POINTS = (24, 1, 40)
INTERIOR = dict(BOXES, nan=((1, 0, 3), (21, 1, 35)))


def points_of(which):
    return NAN_POINTS if which == "nan" else GRIDS[which][0]


def corner_box(which):
    """a box that touches the frame's far corner, of odd extents"""
    px, py, pz = points_of(which)
    count = (min(px, 13), min(py, 3), min(pz, 5))
    return (px - count[0], py - count[1], pz - count[2]), count


def windows_of(which):
    if which == "volume":
        return [(2, 2, 1)]
    return [(1, 0, 1), (4, 0, 2), (1, 1, 1)] + ([(16, 0, 16)] if which == "plane" else [])


@pytest.mark.parametrize("K", [1, 2, 3, 17])
@pytest.mark.parametrize("which", ["plane", "square", "volume", "real", "nan"])
def test_parity(which, K, bflib):
    frames, ids = ensemble(which, K)
    assert frames.shape[1:] == points_of(which)[::-1]
    for window in windows_of(which):
        for reference in sorted({0, K // 2, K - 1}):
            whole, _, _ = check_call(frames, ids, reference, window, None, what=which)
            boxed, _, _ = check_call(frames, ids, reference, window, [INTERIOR[which], corner_box(which)], what=which + " boxes")
            if window == (1, 1, 1) and points_of(which)[1] == 1:
                # a plane has no neighbour along y: every sy != 0 entry is 40 zero bytes
                for t in (whole, boxed):
                    assert not t[:, :, :, (0, 2), :].tobytes().strip(b"\0") and t["terms"][:, :, :, 1, :].any()
            if K > 1:
                # the frames are far more than any tolerance apart: a kernel that reads one frame for every table fails above
                k = (reference + 1) % K
                zero = tuple(window[::-1])
                assert abs(whole["re"][(0, k) + zero] - whole["re"][(0, reference) + zero]) > 0.1 * whole["re"][(0, reference) + zero]


def test_repeat_and_independence(bflib):
    frames, ids = ensemble("square", 17)
    window = (4, 0, 2)
    first, _, _ = bflib.correlate_last_frames(17, 15, window)
    again, _, _ = bflib.correlate_last_frames(17, 15, window)
    assert first.tobytes() == again.tobytes() and first["terms"].all()
    # frame k's table against the same reference frame does not depend on the count: the two newest frames, alone and among 17
    pair, info, _ = bflib.correlate_last_frames(2, 0, window)
    assert int(info.reference_frame_id) == ids[15]
    print(f"  counts 2 and 17: {pair[0, 1]['re'][2, 0, 4]!r} and {first[0, 16]['re'][2, 0, 4]!r} at s = 0")
    assert pair[0, 0].tobytes() == first[0, 15].tobytes() and pair[0, 1].tobytes() == first[0, 16].tobytes()
    assert pair[0, 1].tobytes() != first[0, 15].tobytes()
    # a region's tables do not depend on its company: alone, first and last of five that overlap and differ in size
    box = INTERIOR["square"]
    others = [((0, 0, 0), (64, 1, 64)), ((10, 0, 10), (9, 1, 33)), ((2, 0, 40), (40, 1, 7)), ((30, 0, 30), (1, 1, 1))]
    alone, _, _ = bflib.correlate_last_frames(17, 3, window, regions_of([box]))
    leads, _, _ = bflib.correlate_last_frames(17, 3, window, regions_of([box] + others))
    trails, _, _ = bflib.correlate_last_frames(17, 3, window, regions_of(others + [box]))
    assert alone.shape[0] == 1 and leads.shape[0] == trails.shape[0] == 5
    assert alone[0].tobytes() == leads[0].tobytes() == trails[4].tobytes()
    assert leads[1:].tobytes() == trails[:4].tobytes()
    check_call(frames, ids, 3, window, others + [box], what="five regions")


def test_nan_voxels_are_left_out(bflib):
    frames, ids = ensemble("nan", 3)
    bad = ~(np.isfinite(frames.real) & np.isfinite(frames.imag))
    print(f"  {int(bad.any(axis=0).sum())} of {bad[0].size} voxels not finite in some frame")
    assert bad[1].sum() >= 64 and 4 * (~bad[1]).sum() >= bad[1].size
    window = (2, 0, 2)
    for boxes in (None, [INTERIOR["nan"]]):
        table, expected, _ = check_call(frames, ids, 1, window, boxes, what="nan")
        volume = frames[0].size if boxes is None else int(np.prod(boxes[0][1]))
        at_zero = table["terms"][0, :, 2, 0, 2]
        print(f"  terms at s = 0: {at_zero} of {volume}")
        assert (at_zero < volume).all() and (at_zero > 0).all()
        assert all(np.isfinite(table[name]).all() for name in DOUBLES)
    # a box of one voxel that is not finite in the reference: no term anywhere, a table of zero bytes
    z, x = np.argwhere(bad[1][:, 0, :])[0]
    table, _, _ = check_call(frames, ids, 1, window, [((int(x), 0, int(z)), (1, 1, 1))], what="one NaN voxel")
    assert not table.tobytes().strip(b"\0")


def test_structure(bflib):
    frames, ids = ensemble("square", 3)
    window = (4, 0, 2)
    table, expected, bars = check_call(frames, ids, 1, window, None, what="square")
    own = table[0, 1]
    centre = own[2, 0, 4]
    print(f"  the reference's own entry at s = 0: {centre}")
    assert centre["im"] == 0.0 and centre["re"].tobytes() == centre["energy_reference"].tobytes() == centre["energy_frame"].tobytes()
    assert centre["re"] > 0 and centre["terms"] == 64 * 64
    # the autocorrelation of the whole frame: C[-s] = conj(C[s]), over the same terms
    mirror = own[::-1, ::-1, ::-1]
    bar = bars[0, 1, ..., 0] + bars[0, 1, ::-1, ::-1, ::-1, 0]
    over = np.maximum(np.abs(own["re"] - mirror["re"]), np.abs(own["im"] + mirror["im"]))
    print(f"  C[-s] against conj(C[s]): worst {over.max():.3e}, {float((over / bar).max()):.3f} of the two bars")
    assert np.array_equal(own["terms"], mirror["terms"]) and (over <= bar).all()
    assert (np.abs(own["energy_reference"] - mirror["energy_frame"]) <= bars[0, 1, ..., 1] + bars[0, 1, ::-1, ::-1, ::-1, 2]).all()
    # real frames: no imaginary part anywhere (check_call asks it), here over boxes too
    real, real_ids = ensemble("real", 3)
    check_call(real, real_ids, 2, window, [INTERIOR["real"], corner_box("real")], what="real")
    # the eight octants of the volume sum to the whole: a term belongs to the box of its v, wherever v + s lies
    frames, ids = ensemble("volume", 3)
    window = (2, 2, 1)
    octants = [((x0, y0, z0), (nx, ny, nz)) for z0, nz in ((0, 3), (3, 3)) for y0, ny in ((0, 2), (2, 3)) for x0, nx in ((0, 4), (4, 5))]
    whole, _, whole_bars = check_call(frames, ids, 0, window, None, what="volume")
    parts, _, part_bars = check_call(frames, ids, 0, window, octants, what="octants")
    assert np.array_equal(parts["terms"].sum(axis=0), whole["terms"][0])
    for name, bar in zip(DOUBLES, (0, 0, 1, 2)):
        over = np.abs(parts[name].sum(axis=0) - whole[name][0])
        allowed = whole_bars[0, ..., bar] + part_bars[..., bar].sum(axis=0)
        print(f"  octants against the whole, {name}: worst {over.max():.3e}, {float((over / np.maximum(allowed, 1e-300)).max()):.3f} of the bars")
        assert (over <= allowed).all()


def test_a_known_shift(bflib):
    acq = block("square")
    frames, ids = ensemble("square", 1)
    # +2 along x, -1 along z: a true convolution, taps {0, 0, 0, 0, 1} read f[i - 2] and taps {1, 0, 0} read f[i + 1]
    first, _ = bflib.convolve_last_frames(1, ([0, 0, 0, 0, 1], None, [1, 0, 0]), mode=P.HipSpatialMode.Zero)
    assert first == ids[0] + 1
    pair = bflib.get_last_frames(acq.bp, 2).copy()
    assert np.array_equal(pair[0].view(np.uint32), frames[0].view(np.uint32))
    assert np.array_equal(pair[1][:-1, :, 2:], pair[0][1:, :, :-2])
    box, window = INTERIOR["square"], (4, 0, 4)
    table, expected, _ = check_call(pair, [ids[0], first], 0, window, [box], what="moved by (2, 0, -1)")
    rows = bflib.displacements_from_correlation(table, window, normalised=True)
    want, found = ref.displacements(table, window, True)
    r = rows[0, 1]
    print(f"  window {window}: shift {tuple(r['shift'])}, displacement {tuple(r['displacement'])}, coefficient {float(r['coefficient'])!r}, "
          f"phase {float(r['phase'])!r}, fitted {int(r['fitted']):03b}, at the edge {int(r['at_window_edge']):03b}; restated {want[0, 1]}")
    assert found and rows.shape == (1, 2)
    assert tuple(r["shift"]) == (2, 0, -1) and int(r["at_window_edge"]) == 0 and abs(float(r["coefficient"]) - 1.0) <= 1e-6
    for name in ("shift", "fitted", "at_window_edge"):
        assert np.array_equal(rows[name], want[name]), name
    for name in ("displacement", "coefficient", "phase"):
        assert np.allclose(rows[name], want[name], rtol=2.0 ** -22, atol=2.0 ** -22), name
    # the reference's own table peaks at 0 with coefficient 1
    assert tuple(rows[0, 0]["shift"]) == (0, 0, 0) and abs(float(rows[0, 0]["coefficient"]) - 1.0) <= 1e-6
    # a window that does not reach the shift along x: first the reference alone, on the downloaded frames ...
    narrow = (1, 0, 4)
    expected, _ = ref.correlate(list(pair), 0, narrow, [box])
    alone = ref.displacements(expected, narrow, True)[0][0, 1]
    print(f"  window {narrow}, the reference alone: shift {tuple(alone['shift'])}, coefficient {float(alone['coefficient'])!r}, "
          f"at the edge {int(alone['at_window_edge']):03b}")
    assert float(alone["coefficient"]) < 0.99
    # ... then the library
    table, _, _ = check_call(pair, [ids[0], first], 0, narrow, [box], what="window too narrow")
    r = bflib.displacements_from_correlation(table, narrow, normalised=True)[0, 1]
    print(f"  window {narrow}: shift {tuple(r['shift'])}, coefficient {float(r['coefficient'])!r}, at the edge {int(r['at_window_edge']):03b}")
    assert float(r["coefficient"]) < 0.99
    assert tuple(r["shift"]) == tuple(alone["shift"]) and int(r["at_window_edge"]) == int(alone["at_window_edge"])
