"""What chaining the pairs into tracks on the device costs (beamformer_hip_track_peaks_last_frames, csrc/frame_tracks.hip): device_ms of the
call -- the events around the mark pass and the scan, and around emit, place, nearest, link, the jump rounds, keep, the two scans and
finish, added -- and the host clock around the C entry, on the frames and at the thresholds of tools/pairs_rate.py:
  - three variants of block B's real plane, 24 x 1 x 40, at 0.1 of each frame's largest magnitude, reach 1.5 voxels;
  - the FORCES block on three moving grids of 16 x 16 x 32 and of 32 x 32 x 32, at threshold 0, reach 1.5 voxels;
  - BASELINE config 1's RF (ogl_beamforming_amd/configs.py) on a 256 x 1 x 256 plane under 8 speeds of sound, at 0.1 and at 0.02 of each
    frame's max_abs, reach 1.5 voxels, up to 65536 peaks a frame.
Each case runs at min_length 2 with both record lists, with both deposits as well, and with the deposits alone (both lists NULL);
--repeats calls after two warm-up calls; median, smallest and largest of each.  Measured against it, in the same run: the pair call
with records on the same frames (profiles/pairs_rate.json has the parent commit's numbers for it; --pairs-json copies them into the
result), and the host alternative -- that pair call plus a numpy chaining of the downloaded pairs into the same tracks.
Run from the repository root on a GPU box:
PYTHONPATH=. python tools/tracks_rate.py --json profiles/tracks_rate.json [--pairs-json profiles/pairs_rate.json] [--commit ID]"""
import argparse
import ctypes as C
import json
import statistics
import time

import numpy as np

from ogl_beamforming_amd import configs, lib, params as P
from tests import variants_cases as vc

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=15)
ap.add_argument("--json", default="")
ap.add_argument("--pairs-json", default="")
ap.add_argument("--commit", default="")
args = ap.parse_args()

CAP = P.HIP_MAX_PEAKS_PER_FRAME
MIN_LENGTH = 2
BOTH = P.HIP_TRACK_DEPOSIT_POINTS | P.HIP_TRACK_DEPOSIT_LINKS
L = lib.library()
L.beamformer_set_global_timeout(0xFFFFFFFF)
IDENTITY = np.ascontiguousarray(np.eye(3, 4).reshape(-1), np.float64)
IDENTITY_PTR = IDENTITY.ctypes.data_as(C.POINTER(C.c_double))


def summary(times, scale):
    return {"median_us": statistics.median(times) * scale, "min_us": min(times) * scale, "max_us": max(times) * scale, "runs": len(times)}


def plane_b():
    acq = vc.block("linear", iq=False, cw=False)
    lib.beamform_variants(acq.bp, acq.rf, vc.candidates(acq.bp), acq.filters)
    return 3, vc.POINTS


def forces(points):
    acq = vc.forces_block()
    views = [lib.view(points, tuple(v + k * 0.04e-3 for v in vc.LO3), tuple(v + k * 0.04e-3 for v in vc.HI3)) for k in range(3)]
    lib.beamform_views(acq.bp, acq.rf, views, acq.filters)
    return 3, points


def large_plane():
    acq = configs.config(1)
    m = list(acq.bp.das_voxel_transform)              # das_transform_2d_xz: x extent m[0] from m[12], depth extent m[6] from m[14]
    bp = type(acq.bp).from_buffer_copy(acq.bp)
    bp.das_voxel_transform[:] = [float(v) for v in configs.das_transform_3d((m[12], 0.0, m[14]), (m[12] + m[0], 0.0, m[14] + m[6]))]
    bp.output_points[:3] = [256, 1, 256]
    variants = [lib.variant_of(bp, speed_of_sound=1400.0 + 280.0 * (k + 0.5) / 8) for k in range(8)]
    lib.beamform_variants(bp, np.ascontiguousarray(acq.rf), variants, acq.filters)
    return 8, (256, 1, 256)


def chained_on_the_host(pairs, peaks, min_length):
    """the kept tracks' lengths from the downloaded pair records: the successor table of every frame pair, heads found by a mask, the
    chains followed for all heads at once, a frame a step"""
    K = len(peaks)
    newer = [np.full(n, -1, np.int64) for n in peaks]
    linked = [np.zeros(n, bool) for n in peaks]
    for n in range(K - 1):
        mine = pairs[pairs["frame"] == n]
        newer[n][mine["a"]] = mine["b"]
        linked[n + 1][mine["b"]] = True
    lengths = []
    for s in range(K):
        at = np.flatnonzero(~linked[s])
        length = np.ones(len(at), np.int64)
        alive = np.arange(len(at))
        for n in range(s, K - 1):
            step = newer[n][at[alive]]
            alive = alive[step >= 0]
            at[alive] = step[step >= 0]
            length[alive] += 1
            if not len(alive):
                break
        lengths.append(length)
    lengths = np.concatenate(lengths)
    return lengths[lengths >= min_length]


rows = []
for name, make, fractions in (("3 x 24x1x40 (block B)", plane_b, (0.1,)), ("3 x 16x16x32 (FORCES)", lambda: forces((16, 16, 32)), (0.0,)),
                              ("3 x 32x32x32 (FORCES)", lambda: forces((32, 32, 32)), (0.0,)), ("8 x 256x1x256 (config 1)", large_plane, (0.1, 0.02))):
    K, points = make()                                   # pushed once: the call does not touch the ring
    metrics, _ = lib.score_last_frames(K)
    out_rows, pair_rows = (P.HipTrackedFrame * K)(), (P.HipPeakPairs * (K - 1))()
    tracks = np.empty(K * CAP, np.dtype(P.HipPeakTrack))                  # (virtual memory: only what a call stores is touched)
    track_points = np.empty(K * CAP, np.dtype(P.HipTrackPoint))
    pairs = np.empty((K - 1) * CAP, np.dtype(P.HipPeakPair))
    tracks_ptr, points_ptr = tracks.ctypes.data_as(C.POINTER(P.HipPeakTrack)), track_points.ctypes.data_as(C.POINTER(P.HipTrackPoint))
    pairs_ptr = pairs.ctypes.data_as(C.POINTER(P.HipPeakPair))
    track_total, point_total, pair_total, ms = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_float(0)
    lib.track_map_reset(points)
    lib.localisation_map_reset(points)
    for fraction in fractions:
        levels = (C.c_float * K)(*[float(np.float32(fraction) * np.float32(metrics[k].max_abs)) for k in range(K)])
        row = {"case": name, "frames": K, "points": list(points), "threshold_fraction_of_max_abs": fraction, "max_distance": 1.5, "min_length": MIN_LENGTH}

        def track_call(deposit, with_records):
            assert L.beamformer_hip_track_peaks_last_frames(K, None, levels, K, IDENTITY_PTR, 1, 1, 1.5, CAP, MIN_LENGTH, deposit, out_rows,
                                                            tracks_ptr if with_records else None, points_ptr if with_records else None,
                                                            C.byref(track_total), C.byref(point_total), C.byref(ms)), lib.last_error()

        def pair_call():
            assert L.beamformer_hip_pair_peaks_last_frames(K, None, levels, K, IDENTITY_PTR, 1, 1, 1.5, CAP, 0, pair_rows, pairs_ptr, C.byref(pair_total),
                                                           C.byref(ms)), lib.last_error()

        def pair_call_and_host_chaining():
            pair_call()
            peaks = [int(pair_rows[0].peaks[0])] + [int(r.peaks[1]) for r in pair_rows]
            row["host_tracks_kept"] = int(len(chained_on_the_host(pairs[:pair_total.value], peaks, MIN_LENGTH)))

        for label, call in (("tracks", lambda: track_call(0, True)), ("tracks_and_deposits", lambda: track_call(BOTH, True)),
                            ("deposits_without_records", lambda: track_call(BOTH, False)), ("pair_call", pair_call),
                            ("pair_call_and_host_chaining", pair_call_and_host_chaining)):
            wall, device = [], []
            for n in range(args.repeats + 2):
                assert L.beamformer_hip_synchronize()
                t0 = time.perf_counter()
                call()
                if n >= 2:
                    wall.append(time.perf_counter() - t0)
                    device.append(float(ms.value))
            row[label] = {"wall": summary(wall, 1e6), "device": summary(device, 1e3)}
        track_call(0, True)
        row["peaks"] = [int(r.peaks) for r in out_rows]
        row["tracks_kept"], row["points_kept"] = int(track_total.value), int(point_total.value)
        row["heads"] = int(sum(int(r.heads) for r in out_rows))
        row["longest"] = int(tracks[:track_total.value]["length"].max()) if track_total.value else 0
        assert row["tracks_kept"] == row["host_tracks_kept"], "the host chaining counts other tracks"
        rows.append(row)
        print(json.dumps(row), flush=True)
lib.track_map_reset(None)
lib.localisation_map_reset(None)

result = {"commit": args.commit, "repeats": args.repeats,
          "timing": "host clock around each call (it ends in a synchronise) after two warm-up calls; device: the call's device_ms, events around its launches; "
                    "pair_call_and_host_chaining: the pair call with records and the numpy chaining of the downloaded records, its device time the pair call's",
          "rows": rows}
if args.pairs_json:
    with open(args.pairs_json) as f:
        before = json.load(f)
    result["pair_call_before"] = {"commit": before.get("commit", ""), "rows": [{"case": r["case"], "threshold_fraction_of_max_abs": r["threshold_fraction_of_max_abs"],
                                                                               "pairs": r["pairs"]} for r in before["rows"]]}
if args.json:
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1)
print("| frames | threshold | peaks a frame | tracks kept of heads | longest | tracks: device us (min .. max) | wall us | pair call: device us | wall us | pair call + host chaining: wall us |")
print("|---|---|---|---|---|---|---|---|---|---|")
for r in rows:
    def cell(s):
        return f"{s['median_us']:.0f} ({s['min_us']:.0f} .. {s['max_us']:.0f})"
    print(f"| {r['case']} | {r['threshold_fraction_of_max_abs']} | {min(r['peaks'])} .. {max(r['peaks'])} | {r['tracks_kept']} of {r['heads']} | {r['longest']} | "
          f"{cell(r['tracks']['device'])} | {cell(r['tracks']['wall'])} | {cell(r['pair_call']['device'])} | {cell(r['pair_call']['wall'])} | "
          f"{cell(r['pair_call_and_host_chaining']['wall'])} |")
