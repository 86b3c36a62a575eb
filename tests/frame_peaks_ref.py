"""The reference of beamformer_hip_find_peaks_last_frames: the definition of a frame's peak list (include/ogl_beamformer_hip.h) restated
in numpy.  A plain module: no test, no device, and it never calls the library.

Every decision is taken on ONE float32 a voxel, q: re * re + im * im on float32 arrays for a complex frame, abs for a real one -- no
square root decides anything, so every decision is basic IEEE arithmetic.  A voxel is finite when q is, eligible when it is finite and
q >= t (t: the threshold for real frames, its float32 square for complex ones).  A voxel at flat index i (x fastest) is a peak when it is
eligible, inside the box, and q > q_n for the finite voxels n of its 3 x 3 x 3 neighbourhood below i, q >= q_n for those above; the
neighbourhood is clipped to the FRAME.  A record carries the frame metrics' magnitude (sqrt(q) complex, q real) and, per axis whose two
neighbours lie in the frame and are finite and whose den = (m_minus + m_plus) - (m0 + m0) is negative, the float32 offset
0.5 * (m_minus - m_plus) / den clamped to [-0.5, 0.5]."""
import numpy as np

from tests import frame_metrics_ref


def decision(frame):
    """float32 decision values of a frame (Z, Y, X), float32 or complex64"""
    frame = np.asarray(frame)
    if np.iscomplexobj(frame):
        re, im = np.ascontiguousarray(frame.real, np.float32), np.ascontiguousarray(frame.imag, np.float32)
        with np.errstate(over="ignore", invalid="ignore"):
            q = re * re + im * im
    else:
        q = np.abs(frame.astype(np.float32, copy=False))
    assert q.dtype == np.float32
    return q


def level(frame, threshold):
    """what q is compared with: the float32 threshold, squared in float32 for a complex frame"""
    t = np.float32(threshold)
    return np.float32(t * t) if np.iscomplexobj(frame) else t


def _shifted(padded, dz, dy, dx, shape):
    pz, py, px = shape
    return padded[1 + dz:1 + dz + pz, 1 + dy:1 + dy + py, 1 + dx:1 + dx + px]


def peak_mask(frame, threshold, first=None, count=None, clip_to_box=False):
    """(peaks, eligible): boolean arrays (Z, Y, X) of the frame's peaks inside the box and of the box's eligible voxels.  clip_to_box:
    what a neighbourhood clipped to the BOX would give -- NOT the definition; tests use it to show that a case tells the two apart."""
    pz, py, px = frame.shape
    first = (0, 0, 0) if first is None else tuple(int(v) for v in first)
    count = (px, py, pz) if count is None else tuple(int(v) for v in count)
    assert all(c >= 1 for c in count) and all(f + c <= p for f, c, p in zip(first, count, (px, py, pz)))
    q = decision(frame)
    box = np.zeros(q.shape, bool)
    box[first[2]:first[2] + count[2], first[1]:first[1] + count[1], first[0]:first[0] + count[0]] = True
    finite = np.isfinite(q)
    with np.errstate(invalid="ignore"):
        eligible = finite & box & (q >= level(frame, threshold))
    seen = np.where(finite & box, q, np.float32(np.nan)) if clip_to_box else np.where(finite, q, np.float32(np.nan))
    padded = np.pad(seen, 1, constant_values=np.float32(np.nan))
    beaten = np.zeros(q.shape, bool)
    with np.errstate(invalid="ignore"):
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if (dz, dy, dx) == (0, 0, 0):
                        continue
                    n = _shifted(padded, dz, dy, dx, q.shape)
                    beaten |= (n >= q) if (dz, dy, dx) < (0, 0, 0) else (n > q)       # NaN compares false: it does not count
    return eligible & ~beaten, eligible


def _fit(m, lo, hi, valid):
    """per voxel of the 1-D selections: (offset float32, fitted bool)"""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        den = (lo + hi) - (m + m)
        fitted = valid & np.isfinite(lo) & np.isfinite(hi) & (den < 0)
        offset = np.float32(0.5) * (lo - hi) / den
    offset = np.clip(offset, np.float32(-0.5), np.float32(0.5))
    return np.where(fitted, offset, np.float32(0.0)).astype(np.float32), fitted


def peaks(frame, threshold, first=None, count=None, cap=None, clip_to_box=False):
    """The result of one frame as a dict: found, above_threshold, stored, and the stored records in ascending flat index as arrays --
    index (n, 3) x, y, z; magnitude (n,) float32; offset (n, 3) float32; fitted (n,) bit a for axis a."""
    mask, eligible = peak_mask(frame, threshold, first, count, clip_to_box)
    pz, py, px = frame.shape
    m = frame_metrics_ref.magnitude(frame)
    z, y, x = np.nonzero(mask)                       # C order: ascending flat index, x fastest
    found = len(x)
    if cap is not None:
        z, y, x = z[:cap], y[:cap], x[:cap]
    padded = np.pad(m, 1, constant_values=np.float32(np.nan))
    m0 = m[z, y, x]
    offsets, fitted = np.zeros((len(x), 3), np.float32), np.zeros(len(x), np.uint32)
    for axis, (at, points, step) in enumerate(((x, px, (0, 0, 1)), (y, py, (0, 1, 0)), (z, pz, (1, 0, 0)))):
        lo = padded[1 + z - step[0], 1 + y - step[1], 1 + x - step[2]]
        hi = padded[1 + z + step[0], 1 + y + step[1], 1 + x + step[2]]
        offsets[:, axis], ok = _fit(m0, lo, hi, (at >= 1) & (at + 1 < points))
        fitted |= ok.astype(np.uint32) << np.uint32(axis)
    return {"found": found, "above_threshold": int(eligible.sum()), "stored": len(x),
            "index": np.stack([x, y, z], axis=1).astype(np.uint32).reshape(-1, 3), "magnitude": m0.astype(np.float32), "offset": offsets,
            "fitted": fitted}
