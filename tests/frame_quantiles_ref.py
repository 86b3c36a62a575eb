"""The reference of beamformer_hip_quantiles_last_frames: the definition of a frame's order statistics (include/ogl_beamformer_hip.h)
restated in numpy.  A plain module: no test, no device, and it never calls the library.

The decision value q of a voxel is find_peaks' (tests/frame_peaks_ref.py: re * re + im * im on float32 arrays, abs for a real frame).
A voxel is finite when q is; the others count in non_finite and in nothing else.  q is never negative and never -0, so the order of the
values is the order of their uint32 bit patterns: the n finite values are sorted as uint32.  A fraction f has the rank
floor(f * (n - 1) + 0.5) in float64 and the value q_(rank); below and equal are counted by comparison.  The coarse histogram counts the
finite values by bits >> 20.  magnitude is sqrt(value) in float32 for complex frames, value for real ones; threshold is value for real
frames and for complex ones the largest float32 T >= 0 with fl(T * T) <= value.  Without a finite voxel every number is 0."""
import numpy as np

from tests import frame_peaks_ref

BINS = 2048


def ranks(fractions, n):
    """the ranks of the fractions among n >= 1 values: one float64 multiply, one add, one floor"""
    f = np.asarray(fractions, np.float64)
    return np.floor(f * np.float64(n - 1) + np.float64(0.5)).astype(np.uint64)


def finite_bits(frame, first=None, count=None):
    """(bits, non_finite): the uint32 patterns of the finite decision values of the box, in flat order, and how many are not finite"""
    pz, py, px = frame.shape
    first = (0, 0, 0) if first is None else tuple(int(v) for v in first)
    count = (px, py, pz) if count is None else tuple(int(v) for v in count)
    assert all(c >= 1 for c in count) and all(f + c <= p for f, c, p in zip(first, count, (px, py, pz)))
    q = frame_peaks_ref.decision(frame)[first[2]:first[2] + count[2], first[1]:first[1] + count[1], first[0]:first[0] + count[0]]
    q = np.ascontiguousarray(q).reshape(-1)
    finite = np.isfinite(q)
    bits = q[finite].view(np.uint32)
    assert not (bits >> np.uint32(31)).any()          # never negative, never -0
    return bits, int((~finite).sum())


def threshold_of(value, cplx):
    """the threshold of the peak calls for a decision value: the largest float32 T >= 0 with fl(T * T) <= value (complex), the value
    itself (real).  Bisection over the bit patterns of the non-negative floats: fl(T * T) is monotone in T."""
    value = np.float32(value)
    if not cplx:
        return value
    lo, hi = 0, 0x7F7FFFFF
    with np.errstate(over="ignore", under="ignore"):
        while lo < hi:
            mid = (lo + hi + 1) // 2
            t = np.array([mid], np.uint32).view(np.float32)[0]
            if np.float32(t * t) <= value:
                lo = mid
            else:
                hi = mid - 1
    return np.array([lo], np.uint32).view(np.float32)[0]


def quantiles(frame, fractions, first=None, count=None):
    """The result of one frame as a dict: points, region_first, region_count, voxels, non_finite, histogram (BINS uint32) and `rows`, one
    dict a fraction in the order given: fraction, rank, below, equal, value_bits, value, magnitude, threshold."""
    frame = np.asarray(frame)
    cplx = np.iscomplexobj(frame)
    pz, py, px = frame.shape
    bits, non_finite = finite_bits(frame, first, count)
    ordered = np.sort(bits)
    n = len(ordered)
    out = {"points": (px, py, pz), "region_first": (0, 0, 0) if first is None else tuple(int(v) for v in first),
           "region_count": (px, py, pz) if count is None else tuple(int(v) for v in count), "voxels": n, "non_finite": non_finite,
           "histogram": np.bincount(bits >> np.uint32(20), minlength=BINS).astype(np.uint32), "rows": []}
    assert len(out["histogram"]) == BINS
    fractions = [float(f) for f in np.atleast_1d(np.asarray(fractions, np.float64))]
    for f, r in zip(fractions, ranks(fractions, n) if n else [0] * len(fractions)):
        if n == 0:
            value_bits, below, equal = np.uint32(0), 0, 0
        else:
            value_bits = ordered[int(r)]
            below, equal = int((bits < value_bits).sum()), int((bits == value_bits).sum())
            assert below <= int(r) < below + equal
        value = np.array([value_bits], np.uint32).view(np.float32)[0]
        out["rows"].append({"fraction": f, "rank": int(r), "below": below, "equal": equal, "value_bits": int(value_bits), "value": value,
                            "magnitude": np.sqrt(value) if cplx else value, "threshold": threshold_of(value, cplx) if n else np.float32(0)})
    return out
