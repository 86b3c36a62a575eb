"""The ensemble filter on the device (beamformer_hip_gram_last_frames, beamformer_hip_mix_last_frames; csrc/ensemble.hip) and the loop
burst -> gram -> projector -> mix -> peaks -> views.  Frames are produced by ordinary pushes and downloaded with
beamformer_get_last_frames; the expected values are the numpy reference (tests/ensemble_ref.py) applied to those downloaded arrays --
parity of the frames themselves is other tests' business.

The bars are derived, not measured (tests/ensemble_ref.py returns them with the values).  Gram: the products of widened floats are
exact, a voxel term is one rounding and the running sum V more: (V + 2) 2^-53 sum (|r_j| + |i_j|)(|r_k| + |i_k|), for each of the two
parts of an entry.  Mix: an output float is a float32 fmaf chain of 2K terms: (2K + 2) 2^-24 sum_k (|Wre| + |Wim|)(|re_k| + |im_k|).
Counts, ids, grids, the Hermitian mirror and every zero the definition promises are asked exactly.  Every test prints what it measured
before it asserts."""
import ctypes as C

import numpy as np
import pytest

from ogl_beamforming_amd import params as P
from tests import ensemble_ref as ref
from tests.frame_info import newest_info
from tests.ring_frames import BOXES, check_peaks as check_call, check_gram, check_mix, ensemble, GRIDS, loop_case, LOOP_POINTS, region_of, weights
from tests.scaffold import automatic_path  # noqa: F401

pytestmark = pytest.mark.gpu
E = P.LibError


@pytest.mark.parametrize("K", [1, 2, 3, 17, 65])
@pytest.mark.parametrize("which", ["plane", "square", "volume", "real"])
def test_gram_of_a_burst(which, K, bflib):
    frames, ids = ensemble(which, K)
    assert frames.shape[0] == K and frames.shape[1:] == GRIDS[which][0][::-1] and np.iscomplexobj(frames) == GRIDS[which][3]
    G, _ = check_gram(frames, ids, what=which)
    check_gram(frames, ids, BOXES[which], what=which + " box")
    # the frames are far more than any tolerance apart: a kernel that reads one frame for every row fails above
    if K > 1:
        assert abs(G[0, 1]) < 0.9 * np.sqrt(G[0, 0].real * G[1, 1].real)
    # the same call twice: equal bytes
    again, _, _ = bflib.gram_last_frames(K)
    assert G.tobytes() == again.tobytes()


def test_gram_leaves_out_the_voxels_that_are_not_finite_in_some_frame(bflib):
    frames, ids = ensemble("nan", 3)
    nan = np.isnan(frames).any(axis=0)
    print(f"  {int(nan.sum())} of {nan.size} voxels NaN in some frame")
    assert nan.sum() >= 64 and 4 * (~nan).sum() >= nan.size
    G, _ = check_gram(frames, ids, what="nan")
    assert np.isfinite(G.real).all() and np.isfinite(G.imag).all()
    check_gram(frames, ids, ((1, 0, 3), (21, 1, 35)), what="nan box")
    # a box of NaN voxels only: no voxel, a zero matrix
    z, x = np.argwhere(nan[:, 0, :])[0]
    box = ((int(x), 0, int(z)), (1, 1, 1))
    G, info, _ = bflib.gram_last_frames(3, region_of(box))
    assert (int(info.voxels), int(info.non_finite)) == (0, 1) and not G.any()


def test_gram_of_the_octants_sums_to_the_whole(bflib):
    frames, ids = ensemble("volume", 3)
    whole, bound = check_gram(frames, ids, what="volume")
    total = np.zeros_like(whole)
    for z0, nz in ((0, 3), (3, 3)):
        for y0, ny in ((0, 2), (2, 3)):
            for x0, nx in ((0, 4), (4, 5)):
                part, _, _ = bflib.gram_last_frames(3, region_of(((x0, y0, z0), (nx, ny, nz))))
                total += part
    over = np.maximum(np.abs(total.real - whole.real), np.abs(total.imag - whole.imag))
    print(f"  octants against the whole: worst {over.max():.3e}, {float((over / bound).max()):.3f} of the bound")
    assert (over <= 2 * bound).all()


# ---- mix ----


@pytest.mark.parametrize("K,M", [(1, 1), (3, 3), (17, 5), (5, 17), (65, 65)])
def test_mix_of_a_burst(K, M, bflib):
    frames, ids = ensemble("plane", K)
    before = bytes(bflib.last_burst_info()) if K > 1 else None
    out, first = check_mix("plane", frames, ids, weights(M, K, 7700 + K), tag=3, what="plane")
    if K > 1 and M < 32:
        # the newest burst's info is unchanged behind the outputs
        assert bytes(bflib.last_burst_info()) == before
    # the same call twice: two runs of equal bytes (the K newest frames are now the outputs: mix the sources again by pushing them again)
    frames2, ids2 = ensemble("plane", K)
    assert np.array_equal(frames2.view(np.uint32), frames.view(np.uint32))
    again, _ = check_mix("plane", frames2, ids2, weights(M, K, 7700 + K), tag=3, what="plane again")
    assert out.tobytes() == again.tobytes()


def test_mix_of_real_frames(bflib):
    frames, ids = ensemble("real", 5)
    assert frames.dtype == np.float32
    check_mix("real", frames, ids, weights(3, 5, 7801, real=True), what="real")
    # a nonzero imaginary weight on real frames is refused, and nothing changes
    frames, ids = ensemble("real", 5)
    W = weights(3, 5, 7801, real=True)
    W[2, 4] += 1e-30j
    first, ms = C.c_uint32(77), C.c_float(-1.0)
    assert not bflib.library().beamformer_hip_mix_last_frames(5, W.ctypes.data_as(C.POINTER(C.c_float)), 3, 0, C.byref(first), C.byref(ms))
    assert bflib.last_error()[0] == E.InvalidAccess and first.value == 77 and ms.value == -1.0
    assert int(newest_info(bflib.library()).frame_id) == ids[-1]


def test_mix_by_a_permutation_by_zero_and_over_nan_voxels(bflib):
    frames, ids = ensemble("nan", 5)
    nan = np.isnan(frames).any(axis=0)
    assert nan.sum() >= 64
    order = [3, 0, 4, 1, 2]
    out, _ = check_mix("nan", frames, ids, np.eye(5, dtype=np.complex64)[order], what="permutation")
    for j, k in enumerate(order):
        assert np.array_equal(out[j][~nan], frames[k][~nan])                       # by value (-0 may come back +0)
    assert np.isnan(out.real[:, nan]).all() and np.isnan(out.imag[:, nan]).all()  # no weight is skipped: 0 * NaN
    frames, ids = ensemble("nan", 5)
    out, _ = check_mix("nan", frames, ids, np.zeros((2, 5), np.complex64), what="zero")
    assert not out[:, ~nan].any() and np.isnan(out.real[:, nan]).all()


# ---- the loop: burst -> gram -> projector -> mix -> peaks -> views ----


def test_the_clutter_filter_loop(bflib):
    acq, rf = loop_case()
    burst = bflib.beamform_burst(acq.bp, rf, acq.filters).copy()
    assert burst.shape == (8, 48, 1, 32) and np.iscomplexobj(burst) and np.isfinite(burst.real).all()
    source_energy = [float(r.sum_abs2) for r in bflib.score_last_frames(8)[0]]
    G, info, _ = bflib.gram_last_frames(8)
    W, values = bflib.clutter_projector(G, 1)
    print(f"  eigenvalues {values}")
    assert values[0] > 1e3 * values[1] > 0
    first, _ = bflib.mix_last_frames(8, W)
    assert first == int(info.first_frame_id) + 8
    mixed = bflib.get_last_frames(acq.bp, 8).copy()
    expected, bound = ref.mix(list(burst), W)
    over = np.maximum(np.abs(mixed.real - expected.real), np.abs(mixed.imag - expected.imag))
    print(f"  mixed frames: worst error {over.max():.3e}, {float((over / bound).max()):.3f} of its bound")
    assert (over <= bound).all()
    rows, _ = bflib.score_last_frames(8)
    mixed_energy = [float(r.sum_abs2) for r in rows]
    print(f"  energy: sources {source_energy}, mixed {mixed_energy}")
    assert max(mixed_energy) < min(source_energy)
    thresholds = [0.5 * float(r.max_abs) for r in rows]
    peak_rows, peaks, found = check_call(list(mixed), thresholds, cap=64, what="mixed")
    assert all(r["found"] >= 1 for r in found)
    few = [peaks[int(peak_rows[7].first) + k] for k in range(min(3, int(peak_rows[7].stored)))]
    views = bflib.peaks_to_views(list(acq.bp.das_voxel_transform), LOOP_POINTS, few, (17, 1, 17), (4.0, 0.0, 4.0), use_offsets=True)
    patches = bflib.beamform_burst_views(acq.bp, rf, views, acq.filters)
    assert len(patches) == len(few) and all(len(p) == 8 and p[0].shape == (17, 1, 17) for p in patches)
    assert int(newest_info(bflib.library()).frame_id) - int(bflib.last_burst_views_info().first_frame_id) + 1 == 8 * len(few)
