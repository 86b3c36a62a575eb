"""The reference of beamformer_hip_score_last_frames: the definition of a BeamformerHipFrameMetrics row (include/ogl_beamformer_hip.h)
restated in numpy.  A plain module: no test, no device, and it never calls the library.

The magnitude of a voxel is ONE float32 -- sqrt(re * re + im * im) on float32 arrays for a complex frame, abs for a real one; a voxel is
finite when that float is.  Everything else is formed in float64 from that float: the powers a, a * a, (a * a) * (a * a), the gradient
term d = |v[i + 1]| - |v[i]|, then d * d, summed over the pairs (i, i + 1 along the axis) whose two voxels lie inside the box and are
both finite.  A voxel that is not finite counts in non_finite and in nothing else."""
import numpy as np


def magnitude(frame):
    """float32 magnitudes of a frame (Z, Y, X), float32 or complex64"""
    frame = np.asarray(frame)
    if np.iscomplexobj(frame):
        re, im = np.ascontiguousarray(frame.real, np.float32), np.ascontiguousarray(frame.imag, np.float32)
        with np.errstate(over="ignore", invalid="ignore"):
            m = np.sqrt(re * re + im * im)
    else:
        m = np.abs(frame.astype(np.float32, copy=False))
    assert m.dtype == np.float32
    return m


def metrics(frame, first=None, count=None):
    """The row of `frame` (an array (Z, Y, X)) over the box first .. first + count (x, y, z; None: the whole frame) as a dict with the
    fields of BeamformerHipFrameMetrics that the device computes; `magnitude`: the box's float32 magnitudes, (z, y, x)."""
    pz, py, px = frame.shape
    first = (0, 0, 0) if first is None else tuple(int(v) for v in first)
    count = (px, py, pz) if count is None else tuple(int(v) for v in count)
    assert all(c >= 1 for c in count) and all(f + c <= p for f, c, p in zip(first, count, (px, py, pz)))
    m32 = magnitude(frame)[first[2]:first[2] + count[2], first[1]:first[1] + count[1], first[0]:first[0] + count[0]]
    finite = np.isfinite(m32)
    a = m32.astype(np.float64)
    inside = np.where(finite, a, 0.0)
    a2 = inside * inside
    row = {"points": (px, py, pz), "region_first": first, "region_count": count,
           "voxels": int(finite.sum()), "non_finite": int((~finite).sum()),
           "sum_abs": float(inside[finite].sum()), "sum_abs2": float(a2[finite].sum()), "sum_abs4": float((a2 * a2)[finite].sum()),
           "gradient_pairs": [], "gradient2": [], "magnitude": m32}
    for axis in (2, 1, 0):                        # x, y, z of the public struct are axes 2, 1, 0 of the array
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        pair = finite[lo] & finite[hi]
        d = inside[hi] - inside[lo]
        row["gradient_pairs"].append(int(pair.sum()))
        row["gradient2"].append(float((d * d)[pair].sum()))
    if row["voxels"]:
        masked = np.where(finite, m32, np.float32(-1.0))
        flat = int(np.argmax(masked))             # the first maximum in flat order (x fastest)
        z, rest = divmod(flat, count[1] * count[0])
        y, x = divmod(rest, count[0])
        row["max_abs"] = float(masked[z, y, x])
        row["max_index"] = (x + first[0], y + first[1], z + first[2])
    else:
        row["max_abs"], row["max_index"] = 0.0, (0, 0, 0)
    return row


def score(row, criterion):
    """beamformer_hip_rank_frames' criterion of one row (a dict as above, or anything with the same attribute names), in float64"""
    get = (lambda k: row[k]) if isinstance(row, dict) else (lambda k: getattr(row, k))
    voxels, s1, s2, s4 = int(get("voxels")), float(get("sum_abs")), float(get("sum_abs2")), float(get("sum_abs4"))
    if voxels == 0 or s2 == 0.0:
        return -np.inf
    g = [float(v) for v in get("gradient2")]
    return [s2, s1 / voxels, voxels * s4 / (s2 * s2), (g[0] + g[1] + g[2]) / s2][int(criterion)]
