"""The spatial filter's definition (include/ogl_beamformer_hip.h: beamformer_hip_convolve_last_frames) restated in numpy, in float64:
what the host and device tests judge the library against, with the bound the tests use.  A frame is a numpy array of shape (z, y, x),
complex64 or float32; taps = (hx, hy, hz), each a sequence of an odd number of real taps or None (the axis is left alone).  The two
floats of a complex voxel are filtered apart (a real tap times a complex number in numpy would carry a NaN from one part into the
other): values and bounds of complex frames are complex arrays whose real and imaginary parts belong to the real and imaginary
floats."""
import numpy as np

U = 2.0 ** -24                     # the unit roundoff of float32
ZERO, NORMALISED = 0, 1


def floats_of(frame):
    """the frame's floats as float64, shape (z, y, x, parts), parts 2 for complex frames"""
    frame = np.asarray(frame)
    if np.iscomplexobj(frame):
        return np.stack([frame.real, frame.imag], axis=-1).astype(np.float64)
    return frame.astype(np.float64)[..., None]


def frame_of(floats):
    return floats[..., 0] + 1j * floats[..., 1] if floats.shape[-1] == 2 else floats[..., 0]


def one_pass(f, h, axis, dtype=np.float64, centre=0):
    """g[i] = sum over t = 0 .. n - 1, ascending, of h[t] f[i + r - t + centre] along the numpy axis `axis`, the terms whose source index
    lies outside the frame skipped; accumulated in `dtype` (float64: the definition's exact value up to 2^-53; float32: a restatement
    that rounds the product and the sum apart).  centre: the off-by-one mistake the host test plants."""
    h = np.asarray(h, dtype)
    n, extent = len(h), f.shape[axis]
    r = (n - 1) // 2
    f = np.moveaxis(f, axis, 0)
    g = np.zeros(f.shape, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(n):
            d = r - t + centre                   # g[i] takes f[i + d]
            lo, hi = max(0, -d), min(extent, extent - d)
            if lo < hi:
                g[lo:hi] = g[lo:hi] + h[t] * f[lo + d:hi + d].astype(dtype)
    return np.moveaxis(g, 0, axis)


def passes(f, taps, dtype=np.float64, flip=False, centre=0):
    """the passes x, y, z over the axes that have taps (numpy axes 2, 1, 0 of a (z, y, x, ...) array)"""
    for a in range(3):
        if taps[a] is not None and len(taps[a]):
            h = np.asarray(taps[a], np.float32)
            f = one_pass(f, h[::-1] if flip else h, 2 - a, dtype, centre)
    return f


def pass_bound(f, taps):
    """B of the last pass: B_a = (n_a + 2) u A_a(|g_(a-1)| + B_(a-1)) + A_a(B_(a-1)), A_a the pass under |h|, B_0 = 0, g_0 = f"""
    g, B = f, np.zeros(f.shape, np.float64)
    for a in range(3):
        if taps[a] is None or not len(taps[a]):
            continue
        h = np.asarray(taps[a], np.float32)
        absolute = np.abs(h)
        B = (len(h) + 2) * U * one_pass(np.abs(g) + B, absolute, 2 - a) + one_pass(B, absolute, 2 - a)
        g = one_pass(g, h, 2 - a)
    return B


def rho_of(taps):
    return 1.001 * sum((len(h) + 2) * U for h in taps if h is not None and len(h))


def convolve(frame, taps, mode=ZERO, flip=False, centre=0, plain_sum=False):
    """(values, bound): the filtered frame in complex128 (float64 for a real frame) and the bound on each float of the device's frame.
    flip, centre, plain_sum: the three mistakes the host test plants (correlation for convolution, the centre off by one, Normalised
    dividing by the plain tap sum); the bound is that of the definition whatever they say.

    THE BOUND, derived.  u = 2^-24; the taps are float32 numbers and exact.
    A PASS.  The device's field g^_a is the float32 fmaf chain over the device's g^_(a-1).  A chain of n fmaf from +0 is a dot product of
    n terms with one rounding each: it differs from the exact sum of ITS OWN operands by at most gamma_n = n u / (1 - n u) <= (n + 2) u
    (n <= 33) times the sum of the terms' magnitudes, A_a(|g^_(a-1)|), A_a the same pass under |h|; and |g^_(a-1)| <= |g_(a-1)| +
    B_(a-1).  The exact sum of its own operands differs from the exact g_a by the error carried in, at most A_a(B_(a-1)).  So
        B_a = (n_a + 2) u A_a(|g_(a-1)| + B_(a-1)) + A_a(B_(a-1)),   B_0 = 0:
    the form proposed holds as it stands.  (Underflow aside: a term below 2^-126 rounds with an absolute error of 2^-150, which no
    frame of the tests comes near.  This reference's own float64 rounding is 2^-29 of the first term and inside its "+ 2".)  Skipped
    terms -- outside the frame, or of a non-finite source voxel in Normalised mode -- are no terms: the same expressions with those
    voxels 0.
    NORMALISED.  N^ is within B_N of N by the above.  D's terms are all >= 0, so a chain's error is RELATIVE to its own exact sum:
    D^_a = conv(D^_(a-1)) (1 + e_a), |e_a| <= (n_a + 2) u, hence D^ = D (1 + theta), |theta| <= prod (1 + (n_a + 2) u) - 1 <= rho =
    1.001 sum_a (n_a + 2) u (the sum is below 2^-17: the product's excess over the sum is far inside the 0.001).  Then
        |N^/D^ - N/D| = |(N^ - N) D - N (D^ - D)| / (D^ D) <= (B_N + rho |N|) / (D (1 - rho)),
    and the division rounds once more: u |N^/D^| <= u (|N| + B_N) / (D (1 - rho)).  Together
        [B_N + rho |N| + u (|N| + B_N)] / (D (1 - rho))  <=  [B_N + (rho + u)(|N| + B_N)] / (D (1 - rho)):
    the form proposed is the right-hand side -- it holds, with rho B_N to spare, a term of second order -- and is what is returned,
    where D > 0 (elsewhere the quotient is 0 / 0 and the bound NaN).  D^ > 0 exactly where D > 0: a sum of non-negative terms rounds to
    0 only if it is 0 (underflow aside).
    A float whose float32 chain leaves the float32 range is not finite in `values` (float32_range): no bound is asked there."""
    f = floats_of(frame)
    definition = not (flip or centre or plain_sum)
    if mode == ZERO:
        values = passes(f, taps, flip=flip, centre=centre)
        return frame_of(float32_range(values, frame, taps, mode) if definition else values), frame_of(pass_bound(f, taps))
    finite = np.isfinite(f).all(axis=-1, keepdims=True)
    f0 = np.where(finite, f, 0.0)
    m = np.broadcast_to(finite.astype(np.float64), f.shape)
    N, D = passes(f0, taps, flip=flip, centre=centre), passes(m, taps, flip=flip, centre=centre)
    B_N, rho = pass_bound(f0, taps), rho_of(taps)
    divisor = D
    if plain_sum:
        divisor = np.full(D.shape, np.prod([np.asarray(h, np.float32).astype(np.float64).sum() for h in taps if h is not None and len(h)]))
    with np.errstate(invalid="ignore", divide="ignore"):
        values = np.where(D > 0, N / divisor, np.nan)
        bound = np.where(D > 0, (B_N + (rho + U) * (np.abs(N) + B_N)) / (D * (1.0 - rho)), np.nan)
    return frame_of(float32_range(values, frame, taps, mode) if definition else values), frame_of(bound)


def float32_range(values, frame, taps, mode):
    """`values` (z, y, x, parts) with the floats that leave the float32 range made what the float32 chain makes of them: the header's
    chains are float32 chains under plain IEEE, so a sum beyond FLT_MAX is an infinity (or, met by its opposite, a NaN) in the device's
    frame although its exact value is a finite double.  convolve_float32 rounds the product and the sum apart, which moves no overflow
    but one within an ulp of FLT_MAX."""
    with np.errstate(invalid="ignore", over="ignore"):
        narrow = floats_of(convolve_float32(frame, taps, mode))
    return np.where(np.isfinite(narrow), values, narrow)


def convolve_float32(frame, taps, mode=ZERO):
    """the definition restated in float32 numpy -- the product and the sum rounded apart, where the device fuses them: within the same
    bound (the classical dot-product bound needs no fma) --; what a host that filters a downloaded frame would compute"""
    frame = np.asarray(frame)
    f = floats_of(frame).astype(np.float32)
    if mode == ZERO:
        return frame_of(passes(f, taps, np.float32)).astype(frame.dtype)
    finite = np.isfinite(f).all(axis=-1, keepdims=True)
    f0 = np.where(finite, f, np.float32(0))
    m = np.broadcast_to(finite.astype(np.float32), f.shape)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = passes(f0, taps, np.float32) / passes(m, taps, np.float32)
    return frame_of(q).astype(frame.dtype)


def share_of_bound(got, values, bound, where=None):
    """(the worst |got - values| / bound over the floats where `values` is finite (and `where` holds), every one within its bound)"""
    worst, inside = 0.0, True
    for g, x, b in zip(*[(a.real, a.imag) if np.iscomplexobj(values) else (a,) for a in (np.asarray(got), values, bound)]):
        f = np.isfinite(x) if where is None else np.isfinite(x) & where
        over = np.abs(g[f].astype(np.float64) - x[f])
        if over.size:
            worst = max(worst, float((over / np.maximum(b[f], 1e-300)).max()))
            inside = inside and bool((over <= b[f]).all())
    return worst, inside


def gaussian(n, sigma):
    t = np.arange(n) - (n - 1) / 2
    h = np.exp(-0.5 * (t / sigma) ** 2)
    return (h / h.sum()).astype(np.float32)
