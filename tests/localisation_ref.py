"""The reference of the localisation map (beamformer_hip_accumulate_peaks_last_frames, beamformer_hip_queue_localisation_map,
beamformer_hip_map_placement): the definition in include/ogl_beamformer_hip.h restated in numpy.  A plain module: no test, no device,
and it never calls the library.

A peak is what tests/frame_peaks_ref.py says (no cap).  Its position is p_a = float64(index[a]) + float64(offset[a]) (the offset dropped
without offsets); its map coordinate, per row r of the frame's row-major 3 x 4 float64 placement A,
m_r = ((A[r][3] + A[r][0] p_x) + A[r][1] p_y) + A[r][2] p_z -- every product and sum one float64 operation, which is what numpy does
with arrays --; its bin b_r = floor(m_r + 0.5).  Inside the map on all three axes: the uint32 count at (b_z, b_y, b_x) goes up by one
(wrapping at 2^32); else the peak counts as outside."""
import numpy as np

from tests import frame_peaks_ref


def bins(index, offset, placement, use_offsets=True):
    """(n, 3) float64 bins b (x, y, z) of the records' positions under one placement; index (n, 3) x, y, z; offset (n, 3) float32"""
    A = np.asarray(placement, np.float64).reshape(3, 4)
    p = np.asarray(index).astype(np.float64).reshape(-1, 3)
    if use_offsets:
        p = p + np.asarray(offset, np.float32).astype(np.float64).reshape(-1, 3)
    out = np.empty(p.shape, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        for r in range(3):
            m = ((A[r, 3] + A[r, 0] * p[:, 0]) + A[r, 1] * p[:, 1]) + A[r, 2] * p[:, 2]
            out[:, r] = np.floor(m + 0.5)
    return out


def deposit_records(counts, index, offset, placement, use_offsets=True):
    """adds the records to counts (uint32, (Z, Y, X)) in place; returns (deposited, outside)"""
    pz, py, px = counts.shape
    b = bins(index, offset, placement, use_offsets)
    with np.errstate(invalid="ignore"):
        inside = (b[:, 0] >= 0) & (b[:, 0] < px) & (b[:, 1] >= 0) & (b[:, 1] < py) & (b[:, 2] >= 0) & (b[:, 2] < pz)
    at = b[inside].astype(np.int64)
    flat = (at[:, 2] * py + at[:, 1]) * px + at[:, 0]
    np.add.at(counts.reshape(-1), flat, np.uint32(1))               # uint32: wraps
    return int(inside.sum()), int((~inside).sum())


def deposit(counts, frame, threshold, placement, use_offsets=True, first=None, count=None):
    """the peaks of one frame (Z, Y, X) deposited into counts in place; returns the row's numbers as a dict"""
    r = frame_peaks_ref.peaks(frame, threshold, first, count)
    deposited, outside = deposit_records(counts, r["index"], r["offset"], placement, use_offsets)
    return {"found": r["found"], "above_threshold": r["above_threshold"], "deposited": deposited, "outside": outside}


def accumulate(points, frames, thresholds, placements, use_offsets=True, first=None, count=None, counts=None):
    """the map of `points` = (x, y, z) after the frames' peaks: (counts (Z, Y, X) uint32, [row dicts]).  thresholds: one number or one a
    frame; placements: one 3 x 4 or one a frame; counts: a map to go on from (changed in place)"""
    if counts is None:
        counts = np.zeros((points[2], points[1], points[0]), np.uint32)
    levels = [thresholds] * len(frames) if np.ndim(thresholds) == 0 else list(thresholds)
    A = np.asarray(placements, np.float64).reshape(-1, 3, 4)
    rows = [deposit(counts, f, levels[k], A[0 if len(A) == 1 else k], use_offsets, first, count) for k, f in enumerate(frames)]
    return counts, rows


def queued_frame(counts, scale):
    """the frame beamformer_hip_queue_localisation_map queues: float32(count) rounded to nearest, times float32(scale) in float32"""
    return counts.astype(np.float32) * np.float32(scale)


def affine(transform, points):
    """(L S, t) float64 of a column-major 4 x 4 voxel transform and its grid: voxel i of an axis with P points sits at i / max(1, P - 1)"""
    M = np.asarray(transform, np.float32).astype(np.float64).reshape(4, 4).T            # column major -> M[row, column]
    S = np.diag([1.0 / max(1, int(n) - 1) for n in points])
    return M[:3, :3] @ S, M[:3, 3]


def map_placement(frame_transform, frame_points, map_transform, map_points):
    """(3, 4) float64: S_map^-1 L_map^-1 [L_frame S_frame | t_frame - t_map]"""
    Lf, tf = affine(frame_transform, frame_points)
    Lm, tm = affine(map_transform, map_points)
    return np.linalg.solve(Lm, np.concatenate([Lf, (tf - tm)[:, None]], axis=1))
