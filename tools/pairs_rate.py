"""What linking peaks on the device costs (beamformer_hip_pair_peaks_last_frames, csrc/frame_tracks.hip): device_ms of the call -- the
events around the mark pass and the scan, and around the emit pass, place, nearest, match, scan and emit, added -- and the host clock
around the C entry, at the shapes of tests/test_gpu_tracks.py and at one larger frame:
  - three variants of block B's real plane, 24 x 1 x 40, at 0.1 of each frame's largest magnitude, reach 1.5 voxels;
  - the FORCES block on three moving grids of 16 x 16 x 32 and of 32 x 32 x 32, at threshold 0, reach 1.5 voxels;
  - BASELINE config 1's RF (ogl_beamforming_amd/configs.py) on a 256 x 1 x 256 plane under 8 speeds of sound, at 0.1 and at 0.02 of each
    frame's max_abs, reach 1.5 voxels, up to 65536 peaks a frame.
Each case runs without deposit, with deposit into a track map of the frames' grid, and without records (pairs NULL); --repeats calls
after two warm-up calls; median, smallest and largest of each.  There is no route to compare with: before this call the peak lists were
downloaded and paired on the host.  The nearest kernel evaluates peaks[n] x peaks[n + 1] distances a direction a frame pair: the rows
carry that product.
Run from the repository root on a GPU box:
PYTHONPATH=. python tools/pairs_rate.py --json profiles/pairs_rate.json [--commit ID]"""
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
L = lib.library()
L.beamformer_set_global_timeout(0xFFFFFFFF)
IDENTITY = np.ascontiguousarray(np.eye(3, 4).reshape(-1), np.float64)


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


rows = []
for name, make, fractions in (("3 x 24x1x40 (block B)", plane_b, (0.1,)), ("3 x 16x16x32 (FORCES)", lambda: forces((16, 16, 32)), (0.0,)),
                              ("3 x 32x32x32 (FORCES)", lambda: forces((32, 32, 32)), (0.0,)), ("8 x 256x1x256 (config 1)", large_plane, (0.1, 0.02))):
    K, points = make()                                   # pushed once: the call does not touch the ring
    metrics, _ = lib.score_last_frames(K)
    out_rows = (P.HipPeakPairs * (K - 1))()
    records = np.empty((K - 1) * CAP, np.dtype(P.HipPeakPair))            # (virtual memory: only what a call stores is touched)
    records_ptr = records.ctypes.data_as(C.POINTER(P.HipPeakPair))
    total, ms = C.c_uint32(0), C.c_float(0)
    lib.track_map_reset(points)
    for fraction in fractions:
        levels = (C.c_float * K)(*[float(np.float32(fraction) * np.float32(metrics[k].max_abs)) for k in range(K)])
        row = {"case": name, "frames": K, "points": list(points), "threshold_fraction_of_max_abs": fraction, "max_distance": 1.5}
        for label, deposit, out in (("pairs", 0, records_ptr), ("pairs_and_deposit", 1, records_ptr), ("deposit_without_records", 1, None)):
            wall, device = [], []
            for n in range(args.repeats + 2):
                assert L.beamformer_hip_synchronize()
                t0 = time.perf_counter()
                assert L.beamformer_hip_pair_peaks_last_frames(K, None, levels, K, IDENTITY.ctypes.data_as(C.POINTER(C.c_double)), 1, 1, 1.5, CAP, deposit,
                                                               out_rows, out, C.byref(total), C.byref(ms)), lib.last_error()
                if n >= 2:
                    wall.append(time.perf_counter() - t0)
                    device.append(float(ms.value))
            row[label] = {"wall": summary(wall, 1e6), "device": summary(device, 1e3)}
        row["peaks"] = [int(out_rows[0].peaks[0])] + [int(r.peaks[1]) for r in out_rows]
        row["found"] = [int(out_rows[0].found[0])] + [int(r.found[1]) for r in out_rows]
        row["pairs_made"] = [int(r.pairs) for r in out_rows]
        row["distance_evaluations"] = int(sum(2 * int(r.peaks[0]) * int(r.peaks[1]) for r in out_rows))
        rows.append(row)
        print(json.dumps(row), flush=True)
lib.track_map_reset(None)

result = {"commit": args.commit, "repeats": args.repeats,
          "timing": "host clock around each call (it ends in a synchronise) after two warm-up calls; device: the call's device_ms, events around its launches",
          "rows": rows}
if args.json:
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1)
print("| frames | threshold | peaks a frame | pairs | distance evaluations | device us (min .. max) | wall us (min .. max) | with deposit: device us | wall us |")
print("|---|---|---|---|---|---|---|---|---|")
for r in rows:
    def cell(s):
        return f"{s['median_us']:.0f} ({s['min_us']:.0f} .. {s['max_us']:.0f})"
    print(f"| {r['case']} | {r['threshold_fraction_of_max_abs']} | {min(r['peaks'])} .. {max(r['peaks'])} | {sum(r['pairs_made'])} | {r['distance_evaluations']} | "
          f"{cell(r['pairs']['device'])} | {cell(r['pairs']['wall'])} | {cell(r['pairs_and_deposit']['device'])} | {cell(r['pairs_and_deposit']['wall'])} |")
