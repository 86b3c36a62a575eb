"""The reference of the peak tracks (beamformer_hip_track_peaks_last_frames): the definition in include/ogl_beamformer_hip.h restated in
numpy on top of tests/tracks_ref.py, which has everything the pairs already define -- positions, reach, choices, pairs, the track map's
deposit.  A plain module: no test, no device, and it never calls the library.

LINK: a pair (a, b) of frame pair n links peak a of frame n to peak b of frame n + 1.  An unplaced peak (NaN coordinates) has no links
and lies in no track.  A HEAD is a placed peak without a link to the older frame; a track is a head and its links toward newer frames
until a peak has none (the TAIL): no gap closing.  KEPT: at least min_length peaks.  ORDER: the kept tracks in ascending (start frame,
rank of the head), a track's points oldest first, the runs packed in track order.  DEPOSIT, points: the bin floor(m_r + 0.5) of the
localisation map, inside it the uint32 count goes up by one (tests/localisation_ref.py's rule); links: tracks_ref.deposit, the pair
call's rule, on the kept links of each frame pair."""
import numpy as np

from tests import frame_peaks_ref, tracks_ref

NONE = tracks_ref.NONE
POINTS, LINKS = 1, 2
TRACK = np.dtype([("frame", "<u4"), ("rank", "<u4"), ("length", "<u4"), ("first", "<u4"), ("flags", "<u4"), ("reserved", "<u4"),
                  ("displacement", "<f8", (3,))])
POINT = np.dtype([("track", "<u4"), ("frame", "<u4"), ("rank", "<u4"), ("deposited", "<u4"), ("position", "<f8", (3,))])
assert TRACK.itemsize == 48 and POINT.itemsize == 40
COUNTERS = ("heads", "kept_heads", "kept_points", "kept_links", "points_deposited", "points_outside", "links_deposited", "links_outside")


def links_of(coordinates, max_distance):
    """(newer, older, pair_records, pair_rows): newer[n][a] the rank in frame n + 1 peak a of frame n is linked to, older[n][b] the rank
    in frame n - 1, NONE without one; the pair call's records and rows (no deposit) they were read from"""
    records, rows = tracks_ref.pair_positions(coordinates, max_distance)
    newer = [np.full(len(m), NONE, np.int64) for m in coordinates]
    older = [np.full(len(m), NONE, np.int64) for m in coordinates]
    for r in records:
        n, a, b = int(r["frame"]), int(r["a"]), int(r["b"])
        newer[n][a], older[n + 1][b] = b, a
    return newer, older, records, rows


def all_tracks(coordinates, newer, older):
    """every track, in ascending (start frame, rank of the head): a list of [(frame, rank), ...], oldest first"""
    out = []
    for s, m in enumerate(coordinates):
        for rank in range(len(m)):
            if np.isnan(m[rank, 0]) or older[s][rank] != NONE:
                continue
            run, n, k = [], s, rank
            while k != NONE:
                run.append((n, k))
                n, k = n + 1, int(newer[n][k])
            out.append(run)
    return out


def point_bins(m, shape):
    """(inside, flat) of coordinates (k, 3) in a map of shape (Z, Y, X): the localisation map's BIN rule"""
    pz, py, px = shape
    b = np.floor(m + 0.5)
    with np.errstate(invalid="ignore"):
        inside = (b[:, 0] >= 0) & (b[:, 0] < px) & (b[:, 1] >= 0) & (b[:, 1] < py) & (b[:, 2] >= 0) & (b[:, 2] < pz)
    at = np.where(inside[:, None], b, 0.0).astype(np.int64)
    return inside, (at[:, 2] * py + at[:, 1]) * px + at[:, 0]


def chain_positions(coordinates, max_distance, min_length, deposit=0, point_map=None, counts=None, sums=None):
    """the call on the frames' map coordinates (a list of (n, 3) arrays, oldest first): a dict -- tracks (TRACK records), points (POINT
    records), rows (a dict a frame: peaks, unplaced and the eight COUNTERS), lengths (of ALL tracks, in order), pairs and pair_rows
    (the pair call's, no deposit).  deposit & POINTS: point_map (uint32 (Z, Y, X)) is changed in place; deposit & LINKS: counts and sums
    (tracks_ref.empty_map) are."""
    K = len(coordinates)
    newer, older, pair_records, pair_rows = links_of(coordinates, max_distance)
    every = all_tracks(coordinates, newer, older)
    kept = [run for run in every if len(run) >= min_length]
    tracks, points = np.zeros(len(kept), TRACK), np.zeros(sum(len(run) for run in kept), POINT)
    rows = [{"peaks": len(m), "unplaced": int(np.isnan(m[:, 0]).sum()), **{c: 0 for c in COUNTERS}} for m in coordinates]
    for run in every:
        rows[run[0][0]]["heads"] += 1
    place_of, first = {}, 0
    for t, run in enumerate(kept):
        (s, rank), (e, tail) = run[0], run[-1]
        tracks[t]["frame"], tracks[t]["rank"], tracks[t]["length"], tracks[t]["first"] = s, rank, len(run), first
        tracks[t]["flags"] = (1 if s == 0 else 0) | (2 if e == K - 1 else 0)
        tracks[t]["displacement"] = coordinates[e][tail] - coordinates[s][rank]
        rows[s]["kept_heads"] += 1
        for j, (n, k) in enumerate(run):
            p = points[first + j]
            p["track"], p["frame"], p["rank"], p["position"] = t, n, k, coordinates[n][k]
            place_of[(n, k)] = first + j
            rows[n]["kept_points"] += 1
            rows[n]["kept_links"] += 1 if j + 1 < len(run) else 0
        first += len(run)
    if deposit & POINTS and len(points):
        inside, flat = point_bins(points["position"], point_map.shape)
        np.add.at(point_map.reshape(-1), flat[inside], np.uint32(1))                    # uint32: wraps
        points["deposited"] |= inside.astype(np.uint32)
        for p, within in zip(points, inside):
            rows[int(p["frame"])]["points_deposited" if within else "points_outside"] += 1
    if deposit & LINKS:
        for n in range(K - 1):
            a = np.array([k for k in range(len(coordinates[n])) if (n, k) in place_of and newer[n][k] != NONE], np.int64)
            if not len(a):
                continue
            b = newer[n][a]
            linked = {"a": a, "b": b, "displacement": coordinates[n + 1][b] - coordinates[n][a]}
            inside = tracks_ref.deposit(counts, sums, coordinates[n], coordinates[n + 1], linked)
            for k, within in zip(a, inside):
                points[place_of[(n, int(k))]]["deposited"] |= np.uint32(2 if within else 0)
            rows[n]["links_deposited"] += int(inside.sum())
            rows[n]["links_outside"] += int((~inside).sum())
    return {"tracks": tracks, "points": points, "rows": rows, "lengths": [len(run) for run in every], "pairs": pair_records, "pair_rows": pair_rows}


def chain_records(lists, placements, max_distance, min_length, use_offsets=True, **maps):
    """the call on the frames' find_peaks records: lists[n] = (index (k, 3), offset (k, 3))"""
    A = np.asarray(placements, np.float64).reshape(-1, 3, 4)
    coordinates = [tracks_ref.positions(i, o, A[0 if len(A) == 1 else n], use_offsets) for n, (i, o) in enumerate(lists)]
    return chain_positions(coordinates, max_distance, min_length, **maps)


def chain_frames(frames, thresholds, placements, max_distance, max_per_frame, min_length, use_offsets=True, first=None, count=None, **maps):
    """the call on real frames (Z, Y, X); the rows also carry found, find_peaks' number"""
    levels = tracks_ref.each(thresholds, len(frames))
    found = [frame_peaks_ref.peaks(f, levels[k], first, count, cap=max_per_frame) for k, f in enumerate(frames)]
    out = chain_records([(r["index"], r["offset"]) for r in found], placements, max_distance, min_length, use_offsets, **maps)
    for row, r in zip(out["rows"], found):
        row["found"] = r["found"]
    return out


def links_as_pairs(out):
    """the links of the listed tracks as (frame, a, b) triples in the pair call's order: ascending frame pair, then ascending a"""
    points, triples = out["points"], []
    for t in out["tracks"]:
        run = points[int(t["first"]):int(t["first"]) + int(t["length"])]
        triples += [(int(p["frame"]), int(p["rank"]), int(q["rank"])) for p, q in zip(run[:-1], run[1:])]
    return sorted(triples)


def one_sided(pair_rows):
    """forward choices that are not returned"""
    return sum(int((w["forward"] != NONE).sum()) - w["pairs"] for w in pair_rows)
