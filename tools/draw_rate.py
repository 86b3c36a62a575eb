"""What drawing the kept tracks into both maps on the device costs (beamformer_hip_draw_tracks_last_frames, csrc/frame_tracks.hip): device_ms
of the call -- the track call's launches, then smooth and draw -- and the host clock around the C entry, on the frames and at the
thresholds of tools/tracks_rate.py, under a placement of 8 x the identity onto maps 8 times finer than the frame along every axis of
more than one point, reach 12 map cells (1.5 voxels), min_length 2, both deposits; at smooth 0 and at smooth 2.
Measured against it, in the same run: the host route it replaces -- the track call with BOTH record lists downloaded and a numpy
drawing of them (the same definition, vectorised over all samples, np.add.at into host maps of the same size; its deposit totals are
asserted equal to the device's rows) --, and the track call with both lists alone.
--repeats calls after two warm-up calls; median, smallest and largest of each.
Run from the repository root on a GPU box:
PYTHONPATH=. python tools/draw_rate.py --json profiles/draw_rate.json [--commit ID]"""
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
ap.add_argument("--commit", default="")
args = ap.parse_args()

CAP = P.HIP_MAX_PEAKS_PER_FRAME
MIN_LENGTH, FINER, REACH = 2, 8, 12.0
BOTH = P.HIP_TRACK_DEPOSIT_POINTS | P.HIP_TRACK_DEPOSIT_LINKS
L = lib.library()
L.beamformer_set_global_timeout(0xFFFFFFFF)
PLACEMENT = np.ascontiguousarray((np.eye(3, 4) * FINER).reshape(-1), np.float64)
PLACEMENT_PTR = PLACEMENT.ctypes.data_as(C.POINTER(C.c_double))


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


def inside_of(B, shape):
    pz, py, px = shape
    inside = (B[:, 0] >= 0) & (B[:, 0] < px) & (B[:, 1] >= 0) & (B[:, 1] < py) & (B[:, 2] >= 0) & (B[:, 2] < pz)
    at = B[inside].astype(np.int64)
    return inside, (at[:, 2] * py + at[:, 1]) * px + at[:, 0]


def drawn_on_the_host(tracks, points, w, density, counts, sums):
    """the downloaded record lists drawn by the header's definition, every step over all points, links or samples at once; returns
    (samples, repeats, deposited into `density`, deposited into `counts`)"""
    n = len(points)
    if not n:
        return 0, 0, 0, 0
    position, slot = points["position"], np.arange(n)
    first, length = tracks["first"][points["track"]].astype(np.int64), tracks["length"][points["track"]].astype(np.int64)
    place = slot - first
    s = position
    if w:
        total, terms = np.zeros_like(position), np.zeros(n)
        for off in range(-w, w + 1):                   # ascending j: the definition's order of addition
            valid = (place + off >= 0) & (place + off < length)
            term = position[np.where(valid, slot + off, 0)]
            total = np.where(valid[:, None], np.where((terms == 0)[:, None], term, total + term), total)
            terms += valid
        s = total / terms[:, None]
    older = slot[place + 1 < length]
    a, d = s[older], s[older + 1] - s[older]
    e = np.abs(d).max(axis=1)
    keep = e <= P.HIP_MAX_LINK_SAMPLES
    older, a, d, e = older[keep], a[keep], d[keep], e[keep]
    S = np.maximum(1, np.ceil(e)).astype(np.int64)
    link = np.repeat(np.arange(len(S)), S)
    k = np.arange(int(S.sum())) - np.repeat(np.cumsum(S) - S, S)
    t = (k + 0.5) / S[link]
    B = np.floor((a[link] + d[link] * t[:, None]) + 0.5)
    at = older[link]
    follows = np.zeros(len(B), bool)
    follows[1:] = (at[1:] == at[:-1]) | ((at[1:] == at[:-1] + 1) & (place[at[1:]] > 0))
    repeat = follows.copy()
    repeat[1:] &= (B[1:] == B[:-1]).all(axis=1)
    B, link = B[~repeat], link[~repeat]
    inside, flat = inside_of(B, density.shape)
    np.add.at(density.reshape(-1), flat, np.uint32(1))
    in_points = int(inside.sum())
    inside, flat = inside_of(B, counts.shape)
    np.add.at(counts.reshape(-1), flat, np.uint32(1))
    q = np.floor(d * 1048576.0 + 0.5).astype(np.int64)[link[inside]]
    for r in range(3):
        np.add.at(sums[r].reshape(-1), flat, q[:, r])
    return len(repeat), int(repeat.sum()), in_points, int(inside.sum())


rows = []
for name, make, fractions in (("3 x 24x1x40 (block B)", plane_b, (0.1,)), ("3 x 16x16x32 (FORCES)", lambda: forces((16, 16, 32)), (0.0,)),
                              ("3 x 32x32x32 (FORCES)", lambda: forces((32, 32, 32)), (0.0,)), ("8 x 256x1x256 (config 1)", large_plane, (0.1, 0.02))):
    K, points = make()                                   # pushed once: the calls do not touch the ring
    metrics, _ = lib.score_last_frames(K)
    field = tuple(int(v) * (FINER if v > 1 else 1) for v in points)
    drawn_rows, tracked_rows = (P.HipDrawnFrame * K)(), (P.HipTrackedFrame * K)()
    tracks = np.empty(K * CAP, np.dtype(P.HipPeakTrack))                  # (virtual memory: only what a call stores is touched)
    track_points = np.empty(K * CAP, np.dtype(P.HipTrackPoint))
    tracks_ptr, points_ptr = tracks.ctypes.data_as(C.POINTER(P.HipPeakTrack)), track_points.ctypes.data_as(C.POINTER(P.HipTrackPoint))
    track_total, point_total, ms = C.c_uint32(0), C.c_uint32(0), C.c_float(0)
    lib.track_map_reset(field)
    lib.localisation_map_reset(field)
    host_density, host_counts = np.zeros(field[::-1], np.uint32), np.zeros(field[::-1], np.uint32)
    host_sums = np.zeros((3,) + field[::-1], np.int64)
    for fraction in fractions:
        levels = (C.c_float * K)(*[float(np.float32(fraction) * np.float32(metrics[k].max_abs)) for k in range(K)])
        row = {"case": name, "frames": K, "points": list(points), "map": list(field), "threshold_fraction_of_max_abs": fraction, "max_distance": REACH,
               "min_length": MIN_LENGTH}

        def draw_call(smooth):
            assert L.beamformer_hip_draw_tracks_last_frames(K, None, levels, K, PLACEMENT_PTR, 1, 1, REACH, CAP, MIN_LENGTH, smooth, BOTH, drawn_rows,
                                                            C.byref(ms)), lib.last_error()

        def track_call():
            assert L.beamformer_hip_track_peaks_last_frames(K, None, levels, K, PLACEMENT_PTR, 1, 1, REACH, CAP, MIN_LENGTH, 0, tracked_rows, tracks_ptr,
                                                            points_ptr, C.byref(track_total), C.byref(point_total), C.byref(ms)), lib.last_error()

        def track_call_and_host_drawing(smooth):
            track_call()
            row[f"host_smooth_{smooth}"] = drawn_on_the_host(tracks[:track_total.value], track_points[:point_total.value], smooth, host_density,
                                                             host_counts, host_sums)

        for label, call in (("draw_smooth_0", lambda: draw_call(0)), ("draw_smooth_2", lambda: draw_call(2)), ("track_call", track_call),
                            ("track_call_and_host_drawing_smooth_0", lambda: track_call_and_host_drawing(0)),
                            ("track_call_and_host_drawing_smooth_2", lambda: track_call_and_host_drawing(2))):
            wall, device = [], []
            for n in range(args.repeats + 2):
                assert L.beamformer_hip_synchronize()
                t0 = time.perf_counter()
                call()
                if n >= 2:
                    wall.append(time.perf_counter() - t0)
                    device.append(float(ms.value))
            row[label] = {"wall": summary(wall, 1e6), "device": summary(device, 1e3)}
        for smooth in (0, 2):
            draw_call(smooth)
            total = {name: int(sum(int(getattr(r, name)) for r in drawn_rows)) for name, _ in P.HipDrawnFrame._fields_[4:14]}
            row[f"rows_smooth_{smooth}"] = total
            assert tuple(row.pop(f"host_smooth_{smooth}")) == (total["samples"], total["repeats"], total["points_deposited"], total["links_deposited"]), \
                "the host drawing counts other samples"
        row["peaks"] = [int(r.peaks) for r in drawn_rows]
        rows.append(row)
        print(json.dumps(row), flush=True)
lib.track_map_reset(None)
lib.localisation_map_reset(None)

result = {"commit": args.commit, "repeats": args.repeats,
          "timing": "host clock around each call (it ends in a synchronise) after two warm-up calls; device: the call's device_ms, events around its launches; "
                    "track_call_and_host_drawing: the track call with both record lists and the numpy drawing of the downloaded records into host maps, "
                    "its device time the track call's",
          "rows": rows}
if args.json:
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1)
print("| frames | threshold | peaks a frame | kept links | samples (w 0) | draw w 0: device us (min .. max) | wall us | draw w 2: device us | wall us | "
      "track call: device us | wall us | track call + host drawing w 0: wall us | w 2: wall us |")
print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
for r in rows:
    def cell(s):
        return f"{s['median_us']:.0f} ({s['min_us']:.0f} .. {s['max_us']:.0f})"
    print(f"| {r['case']} | {r['threshold_fraction_of_max_abs']} | {min(r['peaks'])} .. {max(r['peaks'])} | {r['rows_smooth_0']['kept_links']} | "
          f"{r['rows_smooth_0']['samples']} | {cell(r['draw_smooth_0']['device'])} | {cell(r['draw_smooth_0']['wall'])} | {cell(r['draw_smooth_2']['device'])} | "
          f"{cell(r['draw_smooth_2']['wall'])} | {cell(r['track_call']['device'])} | {cell(r['track_call']['wall'])} | "
          f"{cell(r['track_call_and_host_drawing_smooth_0']['wall'])} | {cell(r['track_call_and_host_drawing_smooth_2']['wall'])} |")
