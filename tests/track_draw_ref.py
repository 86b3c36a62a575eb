"""The reference of the drawn tracks (beamformer_hip_draw_tracks_last_frames): the definition in include/ogl_beamformer_hip.h restated in
numpy on top of tests/track_chains_ref.py, which has everything up to the kept tracks' packed points.  A plain module: no test, no
device, and it never calls the library.

SMOOTH: s_i = (((m_j0 + m_j0+1) + ...) + m_j1) / n over the window i - w .. i + w clipped at the TRACK's ends, added in an explicit
loop (np.sum adds pairwise: another order).  LINK i joins s_i to s_i+1: d = s_i+1 - s_i, e = max |d_r|; !(e <= 4096) SKIPS it;
S = max(1, ceil(e)).  SAMPLE k: t = (k + 0.5) / S, c = s_i + d * t (numpy multiplies, then adds: two roundings), B = floor(c + 0.5).
REPEAT: B equal to the B of the sample before it on the same track (the last one of link i - 1 for k = 0, unless that link was
skipped).  DEPOSIT: every other sample, by B, into the localisation map (POINTS) and, with q = floor(d * 2^20 + 0.5), into the track
map (LINKS).  A link belongs to the frame of its older point."""
import numpy as np

from tests import tracks_ref
from tests import track_chains_ref as chains

POINTS, LINKS = chains.POINTS, chains.LINKS
MAX_SMOOTH, MAX_SAMPLES = 8, 4096.0
COUNTERS = ("kept_points", "kept_links", "lone", "links_skipped", "samples", "repeats", "points_deposited", "points_outside",
            "links_deposited", "links_outside")


def smooth(m, w):
    """the moving average of half-width w along one track's points m (L, 3), clipped at the track's ends; w = 0: m itself"""
    m = np.asarray(m, np.float64)
    if w == 0:
        return m.copy()
    out = np.empty_like(m)
    for i in range(len(m)):
        lo, hi = max(0, i - w), min(len(m) - 1, i + w)
        total = m[lo].copy()
        for j in range(lo + 1, hi + 1):
            total = total + m[j]
        out[i] = total / np.float64(hi - lo + 1)
    return out


def link_samples(a, b):
    """link a -> b: (d, B) -- B (S, 3) doubles, the samples' bins in order -- or (d, None) for a skipped link"""
    with np.errstate(invalid="ignore", over="ignore"):
        d = b - a
        e = np.max(np.abs(d))                                          # (np.max hands a NaN on)
    if not e <= MAX_SAMPLES:
        return d, None
    S = max(1, int(np.ceil(e)))
    t = (np.arange(S, dtype=np.float64) + 0.5) / np.float64(S)
    c = a[None, :] + d[None, :] * t[:, None]
    return d, np.floor(c + 0.5)


def draw_track(s):
    """one track's smoothed points s (L, 3): a list a link of (skipped, d, B, drawn) -- drawn (S,) bool, False for a repeat"""
    out, before = [], None
    for i in range(len(s) - 1):
        d, B = link_samples(s[i], s[i + 1])
        if B is None:
            out.append((True, d, None, None))
            before = None
            continue
        previous = np.concatenate([B[:1] if before is None else before[None, :], B[:-1]])
        drawn = (B != previous).any(axis=1)
        if before is None:
            drawn[0] = True
        out.append((False, d, B, drawn))
        before = B[-1]
    return out


def bins_inside(B, shape):
    """(inside, flat) of bins B (k, 3) doubles in a map of shape (Z, Y, X)"""
    pz, py, px = shape
    inside = (B[:, 0] >= 0) & (B[:, 0] < px) & (B[:, 1] >= 0) & (B[:, 1] < py) & (B[:, 2] >= 0) & (B[:, 2] < pz)
    at = np.where(inside[:, None], B, 0.0).astype(np.int64)
    return inside, (at[:, 2] * py + at[:, 1]) * px + at[:, 0]


def draw_chained(chained, w, deposit=0, point_map=None, counts=None, sums=None):
    """the draw pass on chain_positions' result: a dict -- rows (a dict a frame: peaks, unplaced and the ten COUNTERS), links (a list a
    kept track of draw_track's lists: what the property checks read).  deposit & POINTS: point_map (uint32 (Z, Y, X)) is changed in
    place; deposit & LINKS: counts and sums (tracks_ref.empty_map) are."""
    rows = [{"peaks": r["peaks"], "unplaced": r["unplaced"], **{c: 0 for c in COUNTERS}} for r in chained["rows"]]
    for row, r in zip(rows, chained["rows"]):
        row["kept_points"], row["kept_links"] = r["kept_points"], r["kept_links"]
        if "found" in r:
            row["found"] = r["found"]
    every = []
    for t in chained["tracks"]:
        first, length, start = int(t["first"]), int(t["length"]), int(t["frame"])
        if length == 1:
            rows[start]["lone"] += 1
            every.append([])
            continue
        drawn_links = draw_track(smooth(chained["points"]["position"][first:first + length], w))
        every.append(drawn_links)
        for i, (skipped, d, B, drawn) in enumerate(drawn_links):
            row = rows[start + i]
            if skipped:
                row["links_skipped"] += 1
                continue
            row["samples"] += len(B)
            row["repeats"] += int((~drawn).sum())
            kept = B[drawn]
            if deposit & POINTS:
                inside, flat = bins_inside(kept, point_map.shape)
                np.add.at(point_map.reshape(-1), flat[inside], np.uint32(1))
                row["points_deposited"] += int(inside.sum())
                row["points_outside"] += int((~inside).sum())
            if deposit & LINKS:
                inside, flat = bins_inside(kept, counts.shape)
                np.add.at(counts.reshape(-1), flat[inside], np.uint32(1))
                q = tracks_ref.fixed(d)
                for r in range(3):
                    np.add.at(sums[r].reshape(-1), flat[inside], q[r])
                row["links_deposited"] += int(inside.sum())
                row["links_outside"] += int((~inside).sum())
    return {"rows": rows, "links": every, "tracks": chained["tracks"], "points": chained["points"], "lengths": chained["lengths"]}


def draw_positions(coordinates, max_distance, min_length, w, **maps):
    """the call on the frames' map coordinates (a list of (n, 3) arrays, oldest first)"""
    return draw_chained(chains.chain_positions(coordinates, max_distance, min_length), w, **maps)


def draw_records(lists, placements, max_distance, min_length, w, use_offsets=True, **maps):
    """the call on the frames' find_peaks records: lists[n] = (index (k, 3), offset (k, 3))"""
    return draw_chained(chains.chain_records(lists, placements, max_distance, min_length, use_offsets), w, **maps)


def draw_frames(frames, thresholds, placements, max_distance, max_per_frame, min_length, w, use_offsets=True, first=None, count=None, **maps):
    """the call on real frames (Z, Y, X); the rows also carry found, find_peaks' number"""
    return draw_chained(chains.chain_frames(frames, thresholds, placements, max_distance, max_per_frame, min_length, use_offsets, first, count),
                        w, **maps)


def totals(rows):
    """the sums of the rows' counters over the frames"""
    return {c: sum(r[c] for r in rows) for c in COUNTERS}
