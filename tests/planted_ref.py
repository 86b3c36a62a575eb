"""Exact integer references for planted frames (tests/planted.py), and the hazards the planted tests plant."""
import numpy as np

from tests import planted


SHAPES = [planted.PLANE, planted.WAVE, planted.VOLUME]
PLATEAU_SHAPES = [planted.PLANE, planted.VOLUME]
HAZARDS = ([("specials", p, False) for p in SHAPES] + [("squares", p, True) for p in SHAPES] +
           [("plateaus", p, c) for p in PLATEAU_SHAPES for c in (False, True)] + [("radix", planted.VOLUME, False)] +
           [("integers", p, c) for p in PLATEAU_SHAPES for c in (False, True)])


def hazard(name, points, cplx):
    """the planted array (Z, Y, X) of one hazard frame (integers: the second of three)"""
    if name == "specials":
        return planted.specials(points)[0]
    if name == "squares":
        return planted.squares(points)[0]
    if name == "plateaus":
        return planted.plateaus(points, cplx=cplx)[0]
    if name == "radix":
        return planted.radix()[0]
    return planted.integers(3, points, cplx=cplx)[1]


def exact(a):
    """an integer-valued array as int64 (complex: (re, im))"""
    if np.iscomplexobj(a):
        assert (a.real == np.rint(a.real)).all() and (a.imag == np.rint(a.imag)).all()
        return a.real.astype(np.int64), a.imag.astype(np.int64)
    assert (a == np.rint(a)).all()
    return a.astype(np.int64), np.zeros(a.shape, np.int64)


def to_kind(re, im, cplx, dtype):
    return (re + 1j * im).astype(dtype) if cplx else re.astype(dtype)


def gram_int64(frames):
    re, im = exact(frames)
    K = len(re)
    r, i = re.reshape(K, -1), im.reshape(K, -1)
    return (r @ r.T + i @ i.T) + 1j * (r @ i.T - i @ r.T)


def mix_int64(frames, W):
    (fr, fi), (wr, wi) = exact(frames), exact(np.asarray(W))
    K = len(fr)
    r, i = fr.reshape(K, -1), fi.reshape(K, -1)
    shape = (W.shape[0],) + frames.shape[1:]
    return (wr @ r - wi @ i).reshape(shape), (wi @ r + wr @ i).reshape(shape)


def autocorr_int64(y_re, y_im, lags):
    rows = len(y_re)
    re = np.stack([(y_re[:rows - L] * y_re[L:] + y_im[:rows - L] * y_im[L:]).sum(axis=0) for L in range(lags)])
    im = np.stack([(y_re[:rows - L] * y_im[L:] - y_im[:rows - L] * y_re[L:]).sum(axis=0) for L in range(lags)])
    return re, im


def convolve_int64(frame, taps):
    """the ZERO mode passes x, y, z on integers: g[i] = sum over t of h[t] f[i + r - t], the terms outside the frame skipped"""
    re, im = exact(frame)
    out = []
    for f in (re, im):
        for axis, h in zip((2, 1, 0), taps):
            if h is None:
                continue
            h = [int(v) for v in h]
            r = (len(h) - 1) // 2
            g = np.zeros_like(f)
            for t, tap in enumerate(h):
                d = r - t
                lo, hi = max(0, -d), min(f.shape[axis], f.shape[axis] - d)
                if lo < hi:
                    target, source = [slice(None)] * 3, [slice(None)] * 3
                    target[axis], source[axis] = slice(lo, hi), slice(lo + d, hi + d)
                    g[tuple(target)] += tap * f[tuple(source)]
            f = g
        out.append(f)
    return out


def correlate_int64(frames, reference, window):
    """the whole-frame table on integers: (re, im, energy_reference, energy_frame, terms), each (K, 2 Sz + 1, 2 Sy + 1, 2 Sx + 1)"""
    re, im = exact(frames)
    K, pz, py, px = re.shape
    Sx, Sy, Sz = window
    out = np.zeros((5, K, 2 * Sz + 1, 2 * Sy + 1, 2 * Sx + 1), np.int64)
    for sz in range(-Sz, Sz + 1):
        for sy in range(-Sy, Sy + 1):
            for sx in range(-Sx, Sx + 1):
                here = tuple(slice(max(0, -s), min(p, p - s)) for s, p in ((sz, pz), (sy, py), (sx, px)))
                if any(s.start >= s.stop for s in here):
                    continue
                there = (slice(None),) + tuple(slice(s.start + d, s.stop + d) for s, d in zip(here, (sz, sy, sx)))
                rr, ri, fr, fi = re[reference][here][None], im[reference][here][None], re[there], im[there]
                at = (slice(None), sz + Sz, sy + Sy, sx + Sx)
                out[0][at] = (rr * fr + ri * fi).sum(axis=(1, 2, 3))
                out[1][at] = (rr * fi - ri * fr).sum(axis=(1, 2, 3))
                out[2][at] = np.broadcast_to(rr * rr + ri * ri, fr.shape).sum(axis=(1, 2, 3))
                out[3][at] = (fr * fr + fi * fi).sum(axis=(1, 2, 3))
                out[4][at] = fr[0].size
    return out


WEIGHTS = {3: np.array([[1, -2, 1], [0, 2j, -1], [2 - 1j, 0, 1 + 2j]], np.complex64)}
TAPS = (np.array([1, -2, 3], np.float32), np.array([2, 0, -1, 1, 1], np.float32), np.array([-1, 4, 1], np.float32))


def integer_weights(M, K, cplx):
    if K in WEIGHTS and M == K:
        return WEIGHTS[K] if cplx else WEIGHTS[K].real.astype(np.complex64)
    rng = np.random.default_rng(9600 + 17 * M + K)
    W = rng.integers(-2, 3, (M, K)) + (1j * rng.integers(-2, 3, (M, K)) if cplx else 0)
    return W.astype(np.complex64)
