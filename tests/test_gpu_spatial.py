"""The spatial filter on the device (beamformer_hip_convolve_last_frames; csrc/spatial.hip) and the two loops it completes: ... mix ->
Gaussian -> peaks, and ... autocorrelate -> box average of the lag frames.  The ensembles and grids are those of
tests/test_gpu_ensemble.py, and one grid more: "rows", 273 x 3 x 5 -- spatial_row_kernel stages 256 voxels of a row and a halo of 16
either side at 33 taps, so a row of 256 + 16 + 1 voxels is one voxel longer than a block's tile and its halo: two segments, the second
of 17 voxels, with odd y and z.  The expected values are the numpy reference (tests/spatial_ref.py) applied to the downloaded source
frames.

The bar is derived, not measured: tests/spatial_ref.py returns it with the values and its docstring has the derivation.  Ids, grids,
kinds, tags, finite masks and every case the definition makes exact are asked exactly.  Every test prints what it measured -- the worst
error as a share of its bound -- before it asserts."""
import numpy as np
import pytest

from ogl_beamforming_amd import lib as bf
from tests import frame_peaks_ref
from tests import spatial_ref as ref
from tests.frame_info import newest_info
from tests.ring_frames import (spatial_block_of as block_of, burst_info_unchanged, check_peaks as check_call, check_convolve, ensemble,
                               loop_case, NORMALISED, SPATIAL_ZERO as ZERO)
from tests.scaffold import automatic_path  # noqa: F401

pytestmark = pytest.mark.gpu


def frames_of(which, K):
    """K frames of the grid (tests/ring_frames.py's ensemble; "rows", "column": the same by this file's blocks): (frames (K, Z, Y, X), ids)"""
    if which not in ("rows", "column"):
        return ensemble(which, K)
    acq = block_of(which)
    rf = np.random.default_rng(7600 + K).normal(0.0, 1.0, (K,) + acq.rf.shape).astype(acq.rf.dtype)
    frames = bf.beamform(acq.bp, rf[0], acq.filters).copy()[None] if K == 1 else bf.beamform_burst(acq.bp, rf, acq.filters).copy()
    newest = int(newest_info(bf.library()).frame_id)
    return frames, list(range(newest - K + 1, newest + 1))


def taps_of(counts, seed, positive=False):
    """asymmetric taps, negative ones among them unless `positive`: one array (or None) an axis"""
    rng = np.random.default_rng(seed)
    out = []
    for n in counts:
        if not n:
            out.append(None)
            continue
        h = rng.uniform(0.1, 1.0, n) if positive else rng.standard_normal(n)
        out.append((h * np.linspace(1.0, 2.0, n)).astype(np.float32))
    return out


# (grid, K, tap counts x / y / z): every count of 1, 3, 9, 33 on every kind of axis, mixed per axis; counts larger than the axis's
# extent -- 33 over 7, 6 and 5 points, 9 over 5, 3 and 9 over the plane's single y point --; one pass, two and three; the row kernel
# with 16 rows a block (9 and 33 voxels), 1 row (273: two segments), and on the y axis of a grid of one x point
CASES = [("plane", 1, (9, 0, 3)), ("plane", 3, (33, 0, 9)), ("plane", 3, (1, 3, 33)), ("plane", 1, (0, 9, 0)),
         ("volume", 3, (3, 9, 33)), ("volume", 1, (9, 3, 1)), ("volume", 3, (0, 0, 3)), ("volume", 1, (33, 33, 0)),
         ("real", 3, (9, 0, 3)), ("real", 1, (33, 1, 9)),
         ("rows", 3, (33, 3, 9)), ("rows", 1, (9, 1, 3)), ("rows", 1, (0, 3, 0)), ("column", 3, (3, 9, 5))]


@pytest.mark.parametrize("which,K,counts", CASES)
def test_values_in_zero_mode_with_asymmetric_and_negative_taps(which, K, counts, bflib):
    frames, ids = frames_of(which, K)
    before = bflib.last_burst_info() if K > 1 else None
    taps = taps_of(counts, 9200 + sum(counts))
    assert any((h < 0).any() for h in taps if h is not None and len(h) > 1) or max(counts) == 1
    out, _ = check_convolve(which, frames, ids, taps, tag=5, what=which)
    if K > 1:
        burst_info_unchanged(bflib.last_burst_info(), before)      # fewer than 32 outputs: the newest burst's info is unchanged
        # the outputs are far more than any tolerance apart: a kernel that read one frame for every output fails above
        assert np.abs(out[1] - out[0]).max() > 0.1 * np.abs(out[0]).max()


@pytest.mark.parametrize("which", ["plane", "volume", "real", "rows"])
def test_taps_of_one_reproduce_the_sources(which, bflib):
    frames, ids = frames_of(which, 3)
    out, _ = check_convolve(which, frames, ids, [np.ones(1, np.float32)] * 3, what=which + " identity")
    assert np.array_equal(out, frames)                               # as float values (fmaf(1, -0, +0) is +0)


def moved(frames, axis):
    """the frames moved by +1 voxel along the numpy axis, +0 in the vacated plane, as fmaf(1, f, +0) gives them"""
    out = np.zeros_like(frames)
    dst, src = [slice(None)] * 4, [slice(None)] * 4
    dst[axis], src[axis] = slice(1, None), slice(None, -1)
    out[tuple(dst)] = frames[tuple(src)]
    return out + np.zeros((), frames.dtype)


@pytest.mark.parametrize("which,axis", [("plane", 0), ("rows", 0), ("real", 0), ("volume", 0), ("volume", 1), ("volume", 2), ("plane", 2)])
def test_taps_0_0_1_move_the_frame_by_one_voxel_bit_for_bit(which, axis, bflib):
    frames, ids = frames_of(which, 3)
    taps = [None, None, None]
    taps[axis] = np.array([0, 0, 1], np.float32)
    out, _ = check_convolve(which, frames, ids, taps, what=f"{which} +1 along axis {axis}")
    expected = moved(frames, 3 - axis)
    differing = int((out.view(np.uint32) != expected.view(np.uint32)).sum())
    print(f"  {differing} of {out.view(np.uint32).size} words differ from the moved frames")
    assert out.tobytes() == expected.tobytes()
    vacated = [slice(None)] * 4
    vacated[3 - axis] = 0
    assert not np.ascontiguousarray(out[tuple(vacated)]).view(np.uint32).any()             # +0: no bit set


@pytest.mark.parametrize("which", ["volume", "rows"])
def test_one_call_equals_three_calls_byte_for_byte(which, bflib):
    taps = taps_of((9, 3, 5), 9300)
    frames, ids = frames_of(which, 3)
    fused, _ = check_convolve(which, frames, ids, taps, what=which + " x, y, z in one call")
    frames2, ids2 = frames_of(which, 3)
    assert np.array_equal(frames2.view(np.uint32), frames.view(np.uint32))
    split, first = frames2, None
    for axis in range(3):
        only = [taps[a] if a == axis else None for a in range(3)]
        split, first = check_convolve(which, split, ids2 if first is None else list(range(first, first + 3)), only, what=f"{which} axis {axis} alone")
    differing = int((fused.view(np.uint32) != split.view(np.uint32)).sum())
    print(f"  one call against three: {differing} of {fused.view(np.uint32).size} words differ")
    assert fused.tobytes() == split.tobytes()


@pytest.mark.parametrize("which,mode", [("rows", ZERO), ("volume", NORMALISED)])
def test_an_output_depends_on_its_source_alone(which, mode, bflib):
    taps = taps_of((9, 3, 3), 9400, positive=True)
    frames, ids = frames_of(which, 3)
    three, _ = check_convolve(which, frames, ids, taps, mode, what=which + ", one of three")
    # the oldest source as the newest frame, by a mix that copies it: filtered alone
    frames2, ids2 = frames_of(which, 3)
    assert np.array_equal(frames2.view(np.uint32), frames.view(np.uint32))
    first, _ = bflib.mix_last_frames(3, np.array([[1, 0, 0]], np.complex64))
    copy = bflib.get_last_frames(block_of(which).bp, 1).copy()
    assert np.array_equal(copy.view(np.uint32), frames[:1].view(np.uint32))
    alone, _ = check_convolve(which, copy, [first], taps, mode, what=which + ", alone")
    assert alone[0].tobytes() == three[0].tobytes()
    # and the same call again
    frames3, ids3 = frames_of(which, 3)
    again, _ = check_convolve(which, frames3, ids3, taps, mode, what=which + ", again")
    assert again.tobytes() == three.tobytes()


# ---- frames with NaN: the coherency-weighted plane of the frame metrics tests ----

def dilated(mask, axis, r):
    """the mask spread by r voxels either way along the numpy axis, inside the frame (np.roll would wrap)"""
    out = mask.copy()
    for d in range(1, r + 1):
        to, frm = [slice(None)] * mask.ndim, [slice(None)] * mask.ndim
        to[axis], frm[axis] = slice(d, None), slice(None, -d)
        out[tuple(to)] |= mask[tuple(frm)]
        out[tuple(frm)] |= mask[tuple(to)]
    return out


def test_nan_in_zero_mode_poisons_the_whole_support(bflib):
    frames, ids = frames_of("nan", 3)
    nan = np.isnan(frames.real) | np.isnan(frames.imag)
    assert nan.sum() >= 64 and 4 * (~nan).sum() >= nan.size
    # zero taps at both ends: their positions are poisoned all the same (check_convolve asks the finite masks of the reference exactly)
    taps = [np.array([0, 0.5, 0.25, 0, 0], np.float32), None, np.array([0, 1, 0], np.float32)]
    out, _ = check_convolve("nan", frames, ids, taps, what="nan, zero taps among them")
    poisoned = np.isnan(out.real)
    print(f"  {int(nan.sum())} voxels NaN in the sources, {int(poisoned.sum())} in the outputs")
    assert poisoned.sum() > nan.sum() and np.array_equal(poisoned, np.isnan(out.imag))
    # the whole support, worked out apart from the reference: 2 voxels either way along x, then 1 either way along z
    assert np.array_equal(poisoned, dilated(dilated(nan, 3, 2), 1, 1))


def test_nan_in_normalised_mode_fills_the_holes(bflib):
    frames, ids = frames_of("nan", 3)
    nan = np.isnan(frames.real) | np.isnan(frames.imag)
    taps = [ref.gaussian(9, 1.5), None, ref.gaussian(5, 1.0)]
    out, _ = check_convolve("nan", frames, ids, taps, NORMALISED, tag=9, what="nan, normalised")
    # finite exactly where D > 0 (asked by check_convolve through the reference's NaN); here: holes with a finite voxel under the taps
    D_field = ref.passes((~nan[0]).astype(np.float64)[..., None], taps)[..., 0]
    filled = nan[0] & (D_field > 0)
    print(f"  frame 0: {int(nan[0].sum())} NaN voxels, {int(filled.sum())} of them filled, {int((D_field == 0).sum())} voxels without a finite neighbour")
    assert filled.sum() >= 32 and np.isfinite(out[0].real[filled]).all() and np.isfinite(out[0].imag[filled]).all()
    assert np.array_equal(np.isfinite(out[0].real), D_field > 0)
    # Zero mode under the same taps darkens the edges and spreads the NaN; Normalised does neither
    frames2, ids2 = frames_of("nan", 3)
    zero, _ = check_convolve("nan", frames2, ids2, taps, ZERO, what="nan, zero mode")
    assert np.isnan(zero.real).sum() > nan.sum() > np.isnan(out.real).sum()


def test_a_constant_frame_stays_constant_up_to_the_edges_in_normalised_mode(bflib):
    """A frame cannot be uploaded, so the constant is beamformed: the real plane's block with f-number 0 (every channel passes with
    weight 1) on RF of ones sums 16 channels x 2 transmits of 1 into every voxel -- 32.0 exactly, which the test asks first.  (The NaN
    plane has no such input: its frames are complex and demodulated.  Its own constant is 0: the test below.)"""
    acq = block_of("real")
    bp = type(acq.bp).from_buffer_copy(acq.bp)
    bp.f_number = 0.0
    frames = bflib.beamform(bp, np.ones_like(acq.rf), acq.filters).copy()[None]
    assert frames.dtype == np.float32 and (frames == 32.0).all()
    ids = [int(newest_info(bflib.library()).frame_id)]
    taps = [ref.gaussian(9, 2.0), None, ref.gaussian(33, 6.0)]             # 33 taps over 7 points: no voxel has its whole support inside
    out, first = check_convolve("real", frames, ids, taps, NORMALISED, what="constant 32")
    _, bound = ref.convolve(frames[0], taps, NORMALISED)
    off = np.abs(out[0].astype(np.float64) - 32.0)
    print(f"  |out - 32| at the most {off.max():.3e}, {float((off / bound).max()):.4f} of the bound; the bound at the most {bound.max():.3e}")
    assert (off <= bound).all() and bound.max() < 32.0 * 3 * ref.rho_of(taps)      # (the bound is about 2 rho |c|: no loose one)
    # Zero mode on that output's source darkens every voxel, the corners most
    frames2 = bflib.beamform(bp, np.ones_like(acq.rf), acq.filters).copy()[None]
    zero, _ = check_convolve("real", frames2, [int(newest_info(bflib.library()).frame_id)], taps, ZERO, what="constant 32, zero mode")
    assert zero.max() < 0.9 * 32.0 and zero[0, 0, 0, 0] == zero.min() < zero.max()      # (the values themselves: asked by check_convolve)


def test_a_zero_frame_with_holes_stays_zero_and_the_holes_are_filled(bflib):
    """the zero-weight mix of the NaN plane's frames is +0 where all of them are finite and NaN elsewhere: a constant with holes"""
    frames, ids = frames_of("nan", 3)
    nan = (np.isnan(frames.real) | np.isnan(frames.imag)).any(axis=0)
    first, _ = bflib.mix_last_frames(3, np.zeros((3, 3), np.complex64))
    zeros = bflib.get_last_frames(block_of("nan").bp, 3).copy()
    assert np.array_equal(np.isnan(zeros.real), np.broadcast_to(nan, zeros.shape)) and not zeros[:, ~nan].any()
    taps = [ref.gaussian(9, 2.0), None, ref.gaussian(33, 6.0)]
    out, _ = check_convolve("nan", zeros, list(range(first, first + 3)), taps, NORMALISED, what="zeros with holes")
    finite = np.isfinite(out.real)
    print(f"  {int(nan.sum())} holes a frame, {int((~finite[0]).sum())} left")
    assert (~finite[0]).sum() < nan.sum() and not out[finite].any()     # 0 / D = 0 up to the edges and in the filled holes


# ---- the two loops, without a download between the steps ----

def test_the_ulm_loop_with_the_gaussian_in_front_of_the_peaks(bflib):
    acq, rf = loop_case()
    bflib.beamform_burst(acq.bp, rf, acq.filters)
    G, info, _ = bflib.gram_last_frames(8)
    W, values = bflib.clutter_projector(G, 1)
    first, _ = bflib.mix_last_frames(8, W)
    taps = [ref.gaussian(9, 1.5), None, ref.gaussian(9, 1.5)]
    smooth_first, ms = bflib.convolve_last_frames(8, taps)
    assert (first, smooth_first) == (int(info.first_frame_id) + 8, int(info.first_frame_id) + 16)
    # the thresholds from the device's own scores, the peaks found where the smoothed frames lie: nothing has been downloaded yet
    scores, _ = bflib.score_last_frames(8)
    thresholds = [0.25 * float(row.max_abs) for row in scores]
    rows, peaks, _ = bflib.find_peaks_last_frames(8, thresholds, 64, None)
    # only now the downloads: the smoothed frames, and the mixed ones behind them
    both = bflib.get_last_frames(acq.bp, 16).copy()
    mixed, smooth = both[:8], both[8:]
    worst = 0.0
    for n in range(8):
        values, bound = ref.convolve(mixed[n], taps)
        w, inside = ref.share_of_bound(smooth[n], values, bound)
        worst = max(worst, w)
        assert inside
    print(f"  the 8 smoothed frames: worst error {worst:.4f} of its bound, {ms * 1e3:.1f} us")
    # the peak lists are those of the reference on the downloaded smoothed frames (check_call asks every field), and those found above
    again_rows, again, found = check_call(list(smooth), thresholds, cap=64, what="smoothed")
    assert bytes(again) == bytes(peaks) and [int(r.found) for r in again_rows] == [int(r.found) for r in rows]
    # the speckle maxima the Gaussian removes: the unsmoothed frames' peaks by the numpy reference
    rough = [frame_peaks_ref.peaks(f, 0.25 * float(np.abs(f).max()), None, None, cap=4096)["found"] for f in mixed]
    print(f"  peaks above a quarter of the maximum: {[f['found'] for f in found]} smoothed, {rough} unsmoothed")
    assert all(f["found"] >= 1 for f in found) and sum(f["found"] for f in found) < sum(rough)


def test_the_doppler_loop_with_the_box_average_of_the_lag_frames(bflib):
    acq, rf = loop_case()
    bflib.beamform_burst(acq.bp, rf, acq.filters)
    G, info, _ = bflib.gram_last_frames(8)
    W, _ = bflib.clutter_projector(G, 1)
    first, _ = bflib.autocorrelate_last_frames(8, W, 2)
    box = [np.full(5, 0.2, np.float32), None, np.full(9, 1.0 / 9, np.float32)]
    averaged_first, ms = bflib.convolve_last_frames(2, box, tag=4)
    assert averaged_first == first + 2
    both = bflib.get_last_frames(acq.bp, 4).copy()
    lags, averaged = both[:2], both[2:]
    worst = 0.0
    for n in range(2):
        values, bound = ref.convolve(lags[n], box)
        w, inside = ref.share_of_bound(averaged[n], values, bound)
        worst = max(worst, w)
        assert inside
    print(f"  the two averaged lag frames: worst error {worst:.4f} of its bound, {ms * 1e3:.1f} us")
    assert not averaged[0].imag.any()                                  # lag 0's imaginary part is +0, and an average of +0 is +0
    # the Kasai angle of the averaged lag 1 is smoother than that of the raw one: what the average is for
    rough, smooth = np.angle(lags[1]), np.angle(averaged[1])
    assert np.abs(np.diff(smooth, axis=2)).mean() < np.abs(np.diff(rough, axis=2)).mean()
