"""What the spatial filter on the device costs and buys (beamformer_hip_convolve_last_frames; csrc/spatial.hip): on the 512 x 1 x 1024
complex view plane and on a 256 x 256 x 256 complex volume, K = 1 and K = 64 frames -- one frame of BASELINE config 1's RF
(ogl_beamforming_amd/configs.py: 64 channels, one transmit) and K scaled copies of it by a mix 1 -> K --, in one process, in turn,
  (floor)   beamformer_hip_mix_last_frames K -> K with identity weights, asked for its device_ms: every frame read once and written
            once, the streaming floor of one pass;
  (x, y, z) the filter along one axis alone, 9 taps, Zero mode, asked for its device_ms: one pass each;
  (all)     9 taps on every live axis (2 on the plane, 3 in the volume), Zero mode, and the same in Normalised mode;
  (all33)   33 taps on every live axis, the plane only: where arithmetic starts to matter;
timed floor, x, ..., floor, x, ... for --repeats rounds after two warm-up rounds: median, smallest and largest of each device_ms.
Every step filters the K newest frames, which are the outputs of the step before it (Gaussian taps that sum to 1 and identity weights
keep the values in range; a pass's time does not depend on them); the ring holds three runs.
Once per shape: the route without the call -- beamformer_hip_copy_frame of the K frames and the float32 numpy separable filter
(tests/spatial_ref.py: convolve_float32) on the host, a host clock around both; its result cannot return to the ring at all (no
upload path for frames exists).  The volume's host route is timed at K = 1 only.  The device's frames are checked against the
reference's bound once per shape, at K = 1.
Rates: bytes = passes x K frames read and written once, over the median device_ms, beside the measured copy rate of the MI355X.
Run from the repository root on a GPU box: PYTHONPATH=. python tools/spatial_rate.py --json profiles/spatial_rate.json [--commit ID]"""
import argparse
import ctypes as C
import json
import os
import statistics
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--plane-counts", default="1,64")
ap.add_argument("--volume-counts", default="1,64")
ap.add_argument("--volume", type=int, default=256)
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--json", default="")
ap.add_argument("--commit", default="")
args = ap.parse_args()

counts_of = {"plane": [int(v) for v in args.plane_counts.split(",") if v], "volume": [int(v) for v in args.volume_counts.split(",") if v]}
POINTS = {"plane": (512, 1, 1024), "volume": (args.volume,) * 3}
largest = max([int(np.prod(POINTS[s])) * 8 * max(k) for s, k in counts_of.items() if k] + [1 << 28])
os.environ.setdefault("BEAMFORMER_HIP_FRAME_RING_BYTES", str(3 * largest + (1 << 28)))     # three runs of the largest case (before the library loads)

from ogl_beamforming_amd import configs, lib, params as P  # noqa: E402
from tests import spatial_ref as ref  # noqa: E402

COPY_RATE_MEASURED, HBM_PEAK_SPEC, F32_PEAK = 6.29e12, 8.0e12, 157.3e12
L = lib.library()
L.beamformer_set_global_timeout(0xFFFFFFFF)
acq = configs.config(1)
rf = np.ascontiguousarray(acq.rf)
for s, fp in enumerate(acq.filters):
    assert L.beamformer_create_filter(C.byref(fp), s, 0), lib.last_error()
m = list(acq.bp.das_voxel_transform)              # das_transform_2d_xz: x extent m[0] from m[12], depth extent m[6] from m[14]
x0, x1, z0, z1 = m[12], m[12] + m[0], m[14], m[14] + m[6]
BOXES = {"plane": ((x0, 0.0, z0), (x1, 0.0, z1)), "volume": ((x0, -2e-3, z0), (x1, 2e-3, z1))}
G9, G33 = ref.gaussian(9, 1.5), ref.gaussian(33, 5.0)


def summary(times):
    return {"median_us": statistics.median(times) * 1e3, "min_us": min(times) * 1e3, "max_us": max(times) * 1e3, "runs": len(times)}


rows = []
for shape, points in POINTS.items():
    lo, hi = BOXES[shape]
    bp = type(acq.bp).from_buffer_copy(acq.bp)
    bp.das_voxel_transform[:] = [float(v) for v in configs.das_transform_3d(lo, hi)]
    bp.output_points[:3] = list(points)
    voxels = int(np.prod(points))
    frame_bytes = (voxels * 8 + 63) // 64 * 64
    live = [a for a in range(3) if points[a] > 1]
    steps = {"xyz"[a]: ([G9 if b == a else None for b in range(3)], 0) for a in live}
    steps["all"] = ([G9 if a in live else None for a in range(3)], 0)
    steps["all_normalised"] = (steps["all"][0], 1)
    if shape == "plane":
        steps["all33"] = ([G33 if a in live else None for a in range(3)], 0)
    for K in counts_of[shape]:
        lib.beamform(bp, rf, acq.filters)
        if K > 1:
            lib.mix_last_frames(1, (1.0 + 0.5 * np.arange(K) / K).astype(np.complex64)[:, None])
        eye = np.eye(K, dtype=np.complex64)
        row = {"shape": shape, "points": list(points), "frames": K, "frame_bytes": frame_bytes}

        if K == 1:
            # the device's frame against the reference, and the route without the call, once
            info = P.HipFrameInfo()
            assert L.beamformer_hip_get_last_frame_info(C.byref(info))
            t0 = time.perf_counter()
            source = lib.copy_frame(int(info.frame_id)).copy()
            t1 = time.perf_counter()
            host = ref.convolve_float32(source, steps["all"][0])
            t2 = time.perf_counter()
            first, _ = lib.convolve_last_frames(1, steps["all"][0])
            device = lib.copy_frame(first)
            values, bound = ref.convolve(source, steps["all"][0])
            worst, inside = ref.share_of_bound(device, values, bound)
            assert inside, worst
            row["device_against_reference_share_of_bound"] = worst
            row["host_route_copy_frame_s"], row["host_route_numpy_float32_s"] = t1 - t0, t2 - t1
            row["host_route_frames"] = 1
            del host, values, bound, device, source
        elif shape == "plane":
            info = P.HipFrameInfo()
            assert L.beamformer_hip_get_last_frame_info(C.byref(info))
            newest = int(info.frame_id)
            t0 = time.perf_counter()
            frames = [lib.copy_frame(newest - K + 1 + k).copy() for k in range(K)]
            t1 = time.perf_counter()
            for f in frames:
                ref.convolve_float32(f, steps["all"][0])
            t2 = time.perf_counter()
            row["host_route_copy_frame_s"], row["host_route_numpy_float32_s"] = t1 - t0, t2 - t1
            row["host_route_frames"] = K
            del frames
        else:
            row["host_route"] = "not measured at this K (K = 1 is)"

        ms = {"floor": []}
        ms.update({name: [] for name in steps})
        for n in range(2 + args.repeats):
            _, t = lib.mix_last_frames(K, eye)
            ms["floor"].append(t)
            for name, (taps, mode) in steps.items():
                _, t = lib.convolve_last_frames(K, taps, mode)
                ms[name].append(t)
        for v in ms.values():
            del v[:2]
        floor = statistics.median(ms["floor"])
        row["floor_mix_identity_device_us"] = summary(ms["floor"])
        row["floor_bytes_per_second"] = 2 * K * frame_bytes / (floor * 1e-3)
        row["floor_share_of_copy_rate"] = row["floor_bytes_per_second"] / COPY_RATE_MEASURED
        for name, (taps, mode) in steps.items():
            passes = sum(h is not None for h in taps)
            t = statistics.median(ms[name])
            row[name] = {"passes": passes, "taps": [0 if h is None else len(h) for h in taps], "mode": mode, "device_us": summary(ms[name]),
                         "multiple_of_floor": t / floor, "multiple_of_floor_per_pass": t / floor / passes,
                         "bytes_per_second": passes * 2 * K * frame_bytes / (t * 1e-3),
                         "fma_per_second": sum(len(h) for h in taps if h is not None) * 2 * K * voxels / (t * 1e-3)}
        if "host_route_numpy_float32_s" in row:
            n = row["host_route_frames"]
            device_s = statistics.median(ms["all"]) * 1e-3 * n / K
            row["host_route_over_device_call"] = (row["host_route_copy_frame_s"] + row["host_route_numpy_float32_s"]) / device_s
        rows.append(row)
        print(json.dumps(row), flush=True)

result = {"commit": args.commit, "repeats": args.repeats,
          "timing": "device: events around the launches of each call (device_ms), rounds floor, x, (y,) z, all, all_normalised(, all33) in turn after two "
                    "warm-up rounds, every step on the K newest frames; host route: a host clock around copy_frame and around the numpy filter, once",
          "peaks": {"copy_rate_measured_float4": COPY_RATE_MEASURED, "hbm_specified": HBM_PEAK_SPEC, "f32_flop_per_second": F32_PEAK},
          "ring_bytes": int(os.environ["BEAMFORMER_HIP_FRAME_RING_BYTES"]),
          "rows": rows}
if args.json:
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1)
