"""The slow-time autocorrelation on the device (beamformer_hip_autocorrelate_last_frames; csrc/autocorr.hip) and the loop burst -> gram ->
projector -> autocorrelate -> peaks.  The ensembles, grids and weights are those of tests/test_gpu_ensemble.py; the expected values are
the numpy reference (tests/autocorr_ref.py) applied to the downloaded source frames.

The bar is derived, not measured: tests/autocorr_ref.py returns it with the values and its docstring has the derivation -- the rounding
of a float32 fmaf chain of 2N terms over products of the filtered samples, plus what mix's own bound on those samples carries into the
sum.  Ids, grids, kinds, tags, the zeros the definition promises and the finite masks are asked exactly.  Every test prints what it
measured -- the worst error as a share of its bound -- before it asserts."""
import ctypes as C

import numpy as np
import pytest

from ogl_beamforming_amd import params as P
from tests import autocorr_ref as ref
from tests import frame_peaks_ref
from tests.frame_info import newest_info
from tests.ring_frames import (block, burst_info_unchanged, AUTOCORR_CASES as CASES, check_autocorr, check_peaks as check_call, ensemble, finite_of,
                               loop_case, share_of_bound, weights)
from tests.scaffold import automatic_path  # noqa: F401

pytestmark = pytest.mark.gpu
E = P.LibError


@pytest.mark.parametrize("K,rows,lags", CASES)
@pytest.mark.parametrize("which", ["plane", "volume"])
def test_autocorrelation_of_a_filtered_burst(which, K, rows, lags, bflib):
    frames, ids = ensemble(which, K)
    before = bflib.last_burst_info() if K > 1 else None
    out, _ = check_autocorr(which, frames, ids, weights(rows, K, 8100 + 100 * K + rows), lags, tag=5, what=which)
    if K > 1:
        burst_info_unchanged(bflib.last_burst_info(), before)      # fewer than 32 outputs: the newest burst's info is unchanged
    if lags > 1:
        # the lags are far more than any tolerance apart: a kernel that stored one chain for every lag fails above
        assert np.abs(out[1] - out[0]).max() > 0.1 * np.abs(out[0]).max()


@pytest.mark.parametrize("which", ["plane", "volume"])
def test_the_identity_form(which, bflib):
    frames, ids = ensemble(which, 17)
    before = bflib.last_burst_info()
    check_autocorr(which, frames, ids, None, 4, tag=6, what=which + " identity")
    burst_info_unchanged(bflib.last_burst_info(), before)


def test_the_time_reversed_rows_give_the_conjugate_of_lag_one(bflib):
    W = weights(17, 5, 8200)
    frames, ids = ensemble("plane", 5)
    forward, _ = check_autocorr("plane", frames, ids, W, 2, what="forward")
    frames, ids = ensemble("plane", 5)
    # the reversed rows are the same floats y_n in the other order: only the order of the chain differs, so twice the bound
    values, bound = ref.autocorrelate(list(frames), W, 2)
    backward, _ = check_autocorr("plane", frames, ids, W[::-1].copy(), 2, what="reversed, against conj", factor=2.0,
                                 expected=(np.conj(values), bound))
    over = np.maximum(np.abs(backward[1].real - forward[1].real), np.abs(backward[1].imag + forward[1].imag))
    print(f"  R_1 reversed against conj(R_1): worst {float((over / (2 * bound[1])).max()):.4f} of twice the bound")
    assert (over <= 2 * bound[1]).all() and np.abs(forward[1].imag).max() > 100 * bound[1].max()


def test_composition_with_mix_is_bit_for_bit(bflib):
    K = 17
    W = weights(K, K, 8300)
    frames, ids = ensemble("volume", K)
    fused, _ = check_autocorr("volume", frames, ids, W, 4, what="fused")
    frames2, _ = ensemble("volume", K)
    assert np.array_equal(frames2.view(np.uint32), frames.view(np.uint32))
    first, _ = bflib.mix_last_frames(K, W)
    mixed = bflib.get_last_frames(block("volume").bp, K).copy()
    split, _ = check_autocorr("volume", mixed, list(range(first, first + K)), None, 4, what="mix, then the identity form")
    differing = int((fused.view(np.uint32) != split.view(np.uint32)).sum())
    print(f"  fused against mix + identity: {differing} of {fused.view(np.uint32).size} words differ")
    assert fused.tobytes() == split.tobytes()


def test_the_same_call_twice_gives_equal_bytes(bflib):
    W = weights(33, 17, 8400)
    frames, ids = ensemble("plane", 17)
    out, _ = check_autocorr("plane", frames, ids, W, 4, tag=3, what="plane")
    frames2, ids2 = ensemble("plane", 17)
    assert np.array_equal(frames2.view(np.uint32), frames.view(np.uint32))
    again, _ = check_autocorr("plane", frames2, ids2, W, 4, tag=3, what="plane again")
    assert out.tobytes() == again.tobytes()


def test_real_frames(bflib):
    frames, ids = ensemble("real", 5)
    assert frames.dtype == np.float32
    out, _ = check_autocorr("real", frames, ids, weights(17, 5, 8500, real=True), 4, what="real")
    assert out.dtype == np.float32
    frames, ids = ensemble("real", 5)
    check_autocorr("real", frames, ids, None, 3, what="real identity")
    # a nonzero imaginary weight on real frames is refused, and nothing changes
    frames, ids = ensemble("real", 5)
    W = weights(3, 5, 8501, real=True)
    W[2, 4] += 1e-30j
    first, ms = C.c_uint32(77), C.c_float(-1.0)
    assert not bflib.library().beamformer_hip_autocorrelate_last_frames(5, W.ctypes.data_as(C.POINTER(C.c_float)), 3, 2, 0, C.byref(first), C.byref(ms))
    assert bflib.last_error()[0] == E.InvalidAccess and first.value == 77 and ms.value == -1.0
    assert int(newest_info(bflib.library()).frame_id) == ids[-1]


def test_nan_voxels_and_zero_weights(bflib):
    frames, ids = ensemble("nan", 5)
    nan = np.isnan(frames).any(axis=0)
    print(f"  {int(nan.sum())} of {nan.size} voxels NaN in some frame")
    assert nan.sum() >= 64 and 4 * (~nan).sum() >= nan.size
    out, _ = check_autocorr("nan", frames, ids, weights(17, 5, 8600), 4, what="nan")
    assert np.isnan(out.real[:, nan]).all() and np.isnan(out.imag[:, nan]).all() and np.isfinite(out.real[:, ~nan]).all()
    frames, ids = ensemble("nan", 5)
    out, _ = check_autocorr("nan", frames, ids, None, 2, what="nan identity")
    assert np.isnan(out.real[:, nan]).all() and np.isnan(out.imag[:, nan]).all()
    frames, ids = ensemble("nan", 5)
    out, _ = check_autocorr("nan", frames, ids, np.zeros((3, 5), np.complex64), 2, what="zero weights")
    assert not out[:, ~nan].any() and np.isnan(out.real[:, nan]).all() and np.isnan(out.imag[:, nan]).all()   # no weight is skipped: 0 * NaN


# ---- the loop: burst -> gram -> projector -> autocorrelate -> peaks ----

def test_the_power_doppler_loop(bflib):
    acq, rf = loop_case()
    burst = bflib.beamform_burst(acq.bp, rf, acq.filters).copy()
    G, info, _ = bflib.gram_last_frames(8)
    W, values = bflib.clutter_projector(G, 1)
    assert values[0] > 1e3 * values[1] > 0
    first, ms = bflib.autocorrelate_last_frames(8, W, 2)
    assert first == int(info.first_frame_id) + 8
    lag = bflib.get_last_frames(acq.bp, 2).copy()
    expected, bound = ref.autocorrelate(list(burst), W, 2)
    worst, inside = share_of_bound(lag, expected, bound, finite_of(expected))
    print(f"  lags 0 and 1 of the filtered burst: worst error {worst:.4f} of its bound, {ms * 1e3:.1f} us")
    assert inside and not lag[0].imag.any()
    # the peaks of the power image, found where it lies: lag 0 is the older of the two newest frames
    thresholds = [0.25 * float(np.abs(f).max()) for f in lag]
    _, _, found = check_call(list(lag), thresholds, cap=64, what="lags")
    assert found[0]["found"] >= 1
    # the same burst again, mixed: the power image is the sum of |mix outputs|^2 -- of the very floats the mix stores, so within the bound
    # of the identity form --, and its peaks are that sum's
    bflib.beamform_burst(acq.bp, rf, acq.filters)
    bflib.mix_last_frames(8, W)
    mixed = bflib.get_last_frames(acq.bp, 8).copy()
    power = (mixed.real.astype(np.float64) ** 2 + mixed.imag.astype(np.float64) ** 2).sum(axis=0)
    _, identity_bound = ref.autocorrelate(list(mixed), None, 1)
    over = np.abs(lag[0].real - power)
    print(f"  lag 0 against the sum of |mix outputs|^2: worst {float((over / identity_bound[0]).max()):.4f} of the identity form's bound")
    assert (over <= identity_bound[0]).all()
    of_the_sum = frame_peaks_ref.peaks(power.astype(np.float32).astype(np.complex64), thresholds[0], None, None, cap=64)
    assert of_the_sum["found"] == found[0]["found"] and np.array_equal(of_the_sum["index"], found[0]["index"])
