"""The slow-time autocorrelation's definition (include/ogl_beamformer_hip.h: beamformer_hip_autocorrelate_last_frames) restated in
numpy, in float64: what the host and device tests judge the library against, with the bound the tests use.  Frames are numpy arrays of
shape (z, y, x), complex64 or float32, index 0 of a list the oldest frame, as in tests/ensemble_ref.py -- whose mix() makes the filtered
samples here, so that the two definitions cannot drift apart."""
import numpy as np

from tests import ensemble_ref

U = 2.0 ** -24                     # the unit roundoff of float32
TINY = 2.0 ** -150                 # half the spacing of the float32 subnormals: what one rounding below 2^-126 can be off by


def filtered(frames, W):
    """(y, e): the filtered slow-time samples y_n = sum over k of W[n, k] f_k in float64, shape (rows, voxels), and mix's bound e_n on
    each float of the float32 y_n (ensemble_ref.mix); W None: the frames themselves, e = 0"""
    stack = np.stack([np.asarray(f) for f in frames])
    if W is None:
        y = stack.reshape(len(stack), -1).astype(np.complex128 if np.iscomplexobj(stack) else np.float64)
        return y, np.zeros(y.shape, np.float64)
    y, e = ensemble_ref.mix(frames, W)
    return y.reshape(y.shape[0], -1), e.reshape(e.shape[0], -1)


def lag_products(y, lags, conj_second=False, shift=0):
    """R[L] = sum over n = 0 .. rows - 1 - (L + shift) of conj(y_n) y_(n + L + shift), shape (lags, voxels), with plain IEEE propagation:
    the four real products of every term, so that a NaN or an infinity in some y_n reaches both parts of every lag, lag 0's imaginary
    part included (it is 0 * the real part, as the header defines it).  conj_second and shift are the two mistakes the host test shows
    the bound to tell apart from the definition: the conjugate on the other operand, the lag off by one."""
    rows = y.shape[0]
    yr, yi = np.real(y), np.imag(y)
    out = np.zeros((lags,) + y.shape[1:], y.dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for L in range(lags):
            n, m = slice(0, rows - L - shift), slice(L + shift, rows)
            re = (yr[n] * yr[m] + yi[n] * yi[m]).sum(axis=0)
            if not np.iscomplexobj(y):
                out[L] = re
                continue
            im = (yr[n] * yi[m] - yi[n] * yr[m]).sum(axis=0)
            if conj_second:
                im = -im
            if L + shift == 0:
                im = 0.0 * re
            out[L] = re + 1j * im
    return out


def float32_range(out, y, lags):
    """`out` with the floats that leave the float32 range made what the float32 chain makes of them: the header's chains are float32
    chains under plain IEEE, so a product or a sum beyond FLT_MAX is an infinity (or, met by its opposite, a NaN) in the device's
    frame although its exact value is a finite double.  The narrow chain rounds the product and the sum apart, which moves no
    overflow but one within an ulp of FLT_MAX."""
    with np.errstate(invalid="ignore", over="ignore"):
        narrow = lag_products(y.astype(np.complex64 if np.iscomplexobj(y) else np.float32), lags)
    if not np.iscomplexobj(out):
        return np.where(np.isfinite(narrow), out, narrow.astype(out.dtype))
    return np.where(np.isfinite(narrow.real), out.real, narrow.real) + 1j * np.where(np.isfinite(narrow.imag), out.imag, narrow.imag)


def autocorrelate(frames, W, lags):
    """(out, bound): out[L] = R_L in complex128 (float64 for real frames), bound[L] on each float of the device's R_L, both of shape
    (lags,) + the frames'.

    THE BOUND, derived.  u = 2^-24.  The device holds y^_n, the float32 chain of mix; each of its floats lies within
        e_n = (2K + 2) u sum over k of (|Wre| + |Wim|)(|re_k| + |im_k|)
    of the exact y_n (the dot-product bound of a chain of 2K terms; 0 for the identity form, which copies).  With a_n = |yr_n| + |yi_n|
    and m = n + L, N = rows - L, the device's float R^_L differs from the exact one by at most (i) what its own chain rounds plus (ii)
    what the errors of the y^ carry into the exact sum.
      (i)  A chain of 2N fmaf from 0 is a dot product of 2N terms: its error is at most gamma_2N = 2N u / (1 - 2N u) <= (2N + 2) u
           (N <= 256) times the sum of the terms' magnitudes.  The two terms of one n are |y^r_n y^r_m| + |y^i_n y^i_m| for the real
           part and |y^r_n y^i_m| + |y^i_n y^r_m| for the imaginary one; with |y^r_n| <= |yr_n| + e_n and so on, either is at most
           a_n a_m + a_n e_m + a_m e_n + 2 e_n e_m = (a_n + e_n)(a_m + e_m) + e_n e_m.
      (ii) |y^r_n y^r_m - yr_n yr_m| <= |yr_n| e_m + |yr_m| e_n + e_n e_m, likewise for the other product of the part: together at most
           a_n e_m + a_m e_n + 2 e_n e_m, for either part.
    So  bound_L = (2N + 2) u sum_n [(a_n + e_n)(a_m + e_m) + e_n e_m]  +  sum_n [a_n e_m + a_m e_n + 2 e_n e_m].
    (The form first proposed for this bound had e_n e_m once in (ii) and not at all in (i): each part of a term is a sum of TWO
    products, each of which carries its own e_n e_m.  The difference is of second order.)  Real frames run N terms, not 2N, with
    a_n = |y_n|: the same expression bounds them.  This reference's own float64 rounding is 2^-29 of (i) and inside its "+ 2".
    Lag 0's imaginary part is exact (0, or NaN where the real part is not finite): the bound is not asked there.
    UNDERFLOW.  The relative bound of (i) holds for roundings of normal results; a chain link whose result lies below 2^-126 rounds to
    a multiple of 2^-149 and is off by up to 2^-150 whatever its size (the product of two subnormal voxels is 0 on the device): 2N links,
    2N x 2^-150 more.
    A float whose float32 chain leaves the float32 range is not finite in `out` (float32_range): the bound is not asked there either."""
    stack = np.stack([np.asarray(f) for f in frames])
    y, e = filtered(frames, W)
    rows = y.shape[0]
    out = float32_range(lag_products(y, lags), y, lags)
    a = np.abs(np.real(y)) + np.abs(np.imag(y))
    bound = np.zeros((lags,) + y.shape[1:], np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for L in range(lags):
            N = rows - L
            an, am, en, em = a[:N], a[L:], e[:N], e[L:]
            bound[L] = (2 * N + 2) * U * ((an + en) * (am + em) + en * em).sum(axis=0) + (an * em + am * en + 2 * en * em).sum(axis=0) + 2 * N * TINY
    return out.reshape((lags,) + stack.shape[1:]), bound.reshape((lags,) + stack.shape[1:])
