"""The reference of the peak pairs and the track map (beamformer_hip_pair_peaks_last_frames, beamformer_hip_track_map_copy,
beamformer_hip_queue_track_map): the definition in include/ogl_beamformer_hip.h restated in numpy.  A plain module: no test, no device,
and it never calls the library.

A frame's peaks are what tests/frame_peaks_ref.py says, capped at max_per_frame; a peak's rank is its place in that list.  Its position
is p_a = float64(index[a]) + float64(offset[a]) (the offset dropped without offsets), its map coordinate, per row r of the frame's
row-major 3 x 4 float64 placement A, m_r = ((A[r][3] + A[r][0] p_x) + A[r][1] p_y) + A[r][2] p_z; a peak with an m_r that is not
finite is unplaced (all three NaN here).  For a in frame n and b in frame n + 1: d_r = m_r(b) - m_r(a),
d2 = ((d_x d_x) + (d_y d_y)) + (d_z d_z); b is within reach of a when d2 <= R2 = float64(float32(max_distance)) ** 2.  f(a): the b
within reach of the least (d2, rank of b); g(b): the a within reach of the least (d2, rank of a); (a, b) is a pair when f(a) = b and
g(b) = a; a frame pair's list is in ascending a.  With deposit: c_r = 0.5 * (m_r(a) + m_r(b)), bin floor(c_r + 0.5); inside the map
the uint32 count goes up by one and the three int64 sums by floor(d_r * 2^20 + 0.5), both wrapping; else the pair counts as outside.
Every product and sum is one float64 operation, which is what numpy does with arrays."""
import numpy as np

from tests import frame_peaks_ref

NONE = -1
FIXED = 1048576.0
PAIR = np.dtype([("frame", "<u4"), ("a", "<u4"), ("b", "<u4"), ("deposited", "<u4"), ("displacement", "<f8", (3,)), ("distance2", "<f8")])
assert PAIR.itemsize == 48


def reach2(max_distance):
    r = np.float64(np.float32(max_distance))
    return r * r


def positions(index, offset, placement, use_offsets=True):
    """(n, 3) float64 map coordinates of the records under one placement, NaN all three where one is not finite; index (n, 3) x, y, z"""
    A = np.asarray(placement, np.float64).reshape(3, 4)
    p = np.asarray(index).astype(np.float64).reshape(-1, 3)
    if use_offsets:
        p = p + np.asarray(offset, np.float32).astype(np.float64).reshape(-1, 3)
    m = np.empty(p.shape, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        for r in range(3):
            m[:, r] = ((A[r, 3] + A[r, 0] * p[:, 0]) + A[r, 1] * p[:, 1]) + A[r, 2] * p[:, 2]
    m[~np.isfinite(m).all(axis=1)] = np.nan
    return m


def _choices(queries, candidates, r2, back):
    """per query the rank of the candidate within reach of the least (d2, rank), NONE without one; d = m(b) - m(a) in both directions"""
    out = np.full(len(queries), NONE, np.int64)
    if not len(candidates):
        return out
    with np.errstate(over="ignore", invalid="ignore"):
        for k, q in enumerate(queries):
            d = (q - candidates) if back else (candidates - q)
            d2 = ((d[:, 0] * d[:, 0]) + (d[:, 1] * d[:, 1])) + (d[:, 2] * d[:, 2])
            reachable = d2 <= r2                                      # (NaN: false)
            if reachable.any():
                out[k] = int(np.argmin(np.where(reachable, d2, np.inf)))          # the first of equal minima: the lowest rank
    return out


def link(ma, mb, max_distance):
    """the pairs of two frames' map coordinates (n, 3) and (k, 3): a dict -- f, g (int64, NONE: none), a, b (the pairs, ascending a),
    displacement (pairs, 3), distance2 (pairs,)"""
    ma, mb = np.asarray(ma, np.float64).reshape(-1, 3), np.asarray(mb, np.float64).reshape(-1, 3)
    r2 = reach2(max_distance)
    f, g = _choices(ma, mb, r2, back=False), _choices(mb, ma, r2, back=True)
    a = np.array([k for k in range(len(ma)) if f[k] != NONE and g[f[k]] == k], np.int64)
    b = f[a] if len(a) else np.zeros(0, np.int64)
    d = mb[b] - ma[a]
    d2 = ((d[:, 0] * d[:, 0]) + (d[:, 1] * d[:, 1])) + (d[:, 2] * d[:, 2])
    return {"f": f, "g": g, "a": a, "b": b, "displacement": d, "distance2": d2}


def fixed(d):
    """q = (int64)floor(d * 2^20 + 0.5)"""
    return np.floor(np.asarray(d, np.float64) * FIXED + 0.5).astype(np.int64)


def deposit(counts, sums, ma, mb, linked):
    """adds the pairs to counts (uint32 (Z, Y, X)) and sums (int64 (3, Z, Y, X)) in place; returns the pairs' `deposited` flags"""
    pz, py, px = counts.shape
    a, b = linked["a"], linked["b"]
    c = 0.5 * (ma[a] + mb[b])
    at = np.floor(c + 0.5)
    inside = (at[:, 0] >= 0) & (at[:, 0] < px) & (at[:, 1] >= 0) & (at[:, 1] < py) & (at[:, 2] >= 0) & (at[:, 2] < pz)
    where = at[inside].astype(np.int64)
    flat = (where[:, 2] * py + where[:, 1]) * px + where[:, 0]
    np.add.at(counts.reshape(-1), flat, np.uint32(1))                                   # uint32: wraps
    q = fixed(linked["displacement"][inside])
    with np.errstate(over="ignore"):
        for r in range(3):
            np.add.at(sums[r].reshape(-1), flat, q[:, r])                               # int64: wraps
    return inside


def pair_positions(coordinates, max_distance, counts=None, sums=None):
    """the call on the frames' map coordinates (a list of (n, 3) arrays, oldest first): (records, rows) -- the packed PAIR records and
    a dict a frame pair (first, pairs, deposited, outside, unplaced (2), unpaired (2), peaks (2), forward: f, backward: g).  counts
    and sums given: the track map, changed in place (deposit)."""
    records, rows, first = [], [], 0
    for n in range(len(coordinates) - 1):
        ma, mb = coordinates[n], coordinates[n + 1]
        linked = link(ma, mb, max_distance)
        k = len(linked["a"])
        inside = deposit(counts, sums, ma, mb, linked) if counts is not None else np.zeros(k, bool)
        mine = np.zeros(k, PAIR)
        mine["frame"], mine["a"], mine["b"], mine["deposited"] = n, linked["a"], linked["b"], inside
        mine["displacement"], mine["distance2"] = linked["displacement"], linked["distance2"]
        records.append(mine)
        unplaced = [int(np.isnan(m[:, 0]).sum()) for m in (ma, mb)]
        rows.append({"first": first, "pairs": k, "deposited": int(inside.sum()), "outside": k - int(inside.sum()) if counts is not None else 0,
                     "unplaced": unplaced, "unpaired": [len(ma) - unplaced[0] - k, len(mb) - unplaced[1] - k], "peaks": [len(ma), len(mb)],
                     "forward": linked["f"], "backward": linked["g"]})
        first += k
    return (np.concatenate(records) if records else np.zeros(0, PAIR)), rows


def each(value, count, shape=()):
    """one value for all frames, or one a frame"""
    v = np.asarray(value)
    return [v] * count if v.shape == shape else [v[k] for k in range(count)]


def pair_records(lists, placements, max_distance, use_offsets=True, counts=None, sums=None):
    """the call on the frames' find_peaks records: lists[n] = (index (k, 3), offset (k, 3))"""
    A = np.asarray(placements, np.float64).reshape(-1, 3, 4)
    return pair_positions([positions(i, o, A[0 if len(A) == 1 else n], use_offsets) for n, (i, o) in enumerate(lists)], max_distance, counts, sums)


def pair_frames(frames, thresholds, placements, max_distance, max_per_frame, use_offsets=True, first=None, count=None, counts=None, sums=None):
    """the call on real frames (Z, Y, X): (records, rows); the rows also carry found (2), find_peaks' numbers"""
    levels = each(thresholds, len(frames))
    found = [frame_peaks_ref.peaks(f, levels[k], first, count, cap=max_per_frame) for k, f in enumerate(frames)]
    records, rows = pair_records([(r["index"], r["offset"]) for r in found], placements, max_distance, use_offsets, counts, sums)
    for n, row in enumerate(rows):
        row["found"] = [found[n]["found"], found[n + 1]["found"]]
    return records, rows


def empty_map(points):
    """(counts, sums) of a track map of points = (x, y, z), zeroed"""
    shape = (points[2], points[1], points[0])
    return np.zeros(shape, np.uint32), np.zeros((3,) + shape, np.int64)


def queued_frame(counts, sums, component, scale, min_pairs=1):
    """the frame beamformer_hip_queue_track_map queues: float32 (Z, Y, X)"""
    scale = np.float32(scale)
    enough = counts >= max(1, int(min_pairs))
    n = np.where(enough, counts, 1).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        mean = [(sums[r].astype(np.float64) / FIXED) / n for r in range(3)]
        if component < 3:
            out = mean[component].astype(np.float32) * scale
        elif component == 3:
            out = counts.astype(np.float32) * scale
        else:
            out = ((mean[0] * mean[0] + mean[1] * mean[1]) + mean[2] * mean[2]).astype(np.float32) * scale
    return np.where(enough, out, np.float32(0.0)).astype(np.float32)
