"""What the slow-time autocorrelation on the device buys (beamformer_hip_autocorrelate_last_frames; csrc/autocorr.hip): the ensembles of
tools/ensemble_filter_rate.py -- K frames of variants pushes of BASELINE config 1's RF (64 channels, one transmit, complex frames) under
K speeds of sound, on a 256 x 1 x 256 plane and on a 64 x 64 x 64 volume, K = 8 and 64 -- are queued once, the projector that removes
their strongest slow-time component is made from their Gram matrix, and then, in turn, in one process,
  (a) before:    beamformer_hip_mix_last_frames K -> K, beamformer_get_last_frames of the K filtered frames, lags 0 and 1 of them in
                 numpy (complex64): the only route to a power Doppler image of a filtered ensemble without this call;
  (b) now:       beamformer_hip_autocorrelate_last_frames(K, W, K, 2) and beamformer_get_last_frames of the 2 lag frames;
  (c) mix:       the mix K -> K alone, asked for its device_ms;
  (d) kernel:    the autocorrelation alone, weights and 2 lags, asked for its device_ms;
  (e) identity:  the identity form (weights NULL) on the K newest frames, 2 lags, asked for its device_ms;
timed a, b, c, d, e, a, ... with a host clock around each (every one ends in a synchronise: a download, or a call asked for its time)
for --repeats rounds after two warm-up rounds: median, smallest and largest of each.  Every step queues frames of its own behind the
ensemble, so the ensemble is queued again before every step, outside the timed window: all five read the same K frames.  Once per
ensemble, before the rounds, (b)'s two frames are checked against (a)'s numpy result.
The kernel's rates: bytes = K frames read once and 2 written, flop = 8 K K voxels for the filtered samples and 8 K voxels a lag, over the
median device_ms, beside the measured copy rate and the f32 peak of the MI355X; "binds" names the larger of the two least times.
Run from the repository root on a GPU box: PYTHONPATH=. python tools/autocorr_rate.py --json profiles/autocorr_rate.json [--commit ID]"""
import argparse
import ctypes as C
import json
import statistics
import time

import numpy as np

from ogl_beamforming_amd import configs, lib, params as P

ap = argparse.ArgumentParser()
ap.add_argument("--plane-counts", default="8,64")
ap.add_argument("--volume-counts", default="8,64")
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--json", default="")
ap.add_argument("--commit", default="")
args = ap.parse_args()

COPY_RATE_MEASURED, HBM_PEAK_SPEC, F32_PEAK = 6.29e12, 8.0e12, 157.3e12
LAGS = 2
L = lib.library()
L.beamformer_set_global_timeout(0xFFFFFFFF)
acq = configs.config(1)
rf = np.ascontiguousarray(acq.rf)
for s, fp in enumerate(acq.filters):
    assert L.beamformer_create_filter(C.byref(fp), s, 0), lib.last_error()
m = list(acq.bp.das_voxel_transform)              # das_transform_2d_xz: x extent m[0] from m[12], depth extent m[6] from m[14]
x0, x1, z0, z1 = m[12], m[12] + m[0], m[14], m[14] + m[6]
SHAPES = {"256x1x256": ((256, 1, 256), (x0, 0.0, z0), (x1, 0.0, z1), args.plane_counts),
          "64x64x64": ((64, 64, 64), (x0, -2e-3, z0), (x1, 2e-3, z1), args.volume_counts)}


def summary(times, scale=1e6):
    return {"median_us": statistics.median(times) * scale, "min_us": min(times) * scale, "max_us": max(times) * scale, "runs": len(times)}


rows = []
for name, (points, lo, hi, counts) in SHAPES.items():
    bp = type(acq.bp).from_buffer_copy(acq.bp)
    bp.das_voxel_transform[:] = [float(v) for v in configs.das_transform_3d(lo, hi)]
    bp.output_points[:3] = list(points)
    voxels = int(np.prod(points))
    frame_bytes = (voxels * 8 + 63) // 64 * 64
    for K in (int(v) for v in counts.split(",") if v):
        speeds = [1400.0 + 280.0 * (k + 0.5) / K for k in range(K)]
        raw = np.zeros(K * frame_bytes // 4, np.float32)
        raw_lags = np.zeros(LAGS * frame_bytes // 4, np.float32)
        weights = np.zeros((K, K), np.complex64)
        weights_ptr = weights.ctypes.data_as(C.POINTER(C.c_float))
        ms, first = C.c_float(0), C.c_uint32(0)
        device_ms = {"mix": [], "kernel": [], "identity": []}

        def queue_ensemble():
            for at in range(0, K, P.HIP_MAX_VARIANTS):
                lib.beamform_variants(bp, rf, [lib.variant_of(bp, speed_of_sound=v) for v in speeds[at:at + P.HIP_MAX_VARIANTS]], acq.filters)

        def frames_of(buffer, count):
            return np.ascontiguousarray(buffer.reshape(count, frame_bytes // 4)[:, : 2 * voxels]).view(np.complex64)

        def leg_before():
            assert L.beamformer_hip_mix_last_frames(K, weights_ptr, K, 0, None, None), lib.last_error()
            assert L.beamformer_get_last_frames(raw.ctypes.data_as(C.c_void_p), raw.nbytes, K), lib.last_error()
            y = frames_of(raw, K)
            return np.stack([(y.real * y.real + y.imag * y.imag).sum(axis=0), (np.conj(y[:-1]) * y[1:]).sum(axis=0)])

        def leg_now():
            assert L.beamformer_hip_autocorrelate_last_frames(K, weights_ptr, K, LAGS, 0, None, None), lib.last_error()
            assert L.beamformer_get_last_frames(raw_lags.ctypes.data_as(C.c_void_p), raw_lags.nbytes, LAGS), lib.last_error()
            return frames_of(raw_lags, LAGS)

        def run_mix():
            assert L.beamformer_hip_mix_last_frames(K, weights_ptr, K, 0, C.byref(first), C.byref(ms)), lib.last_error()
            device_ms["mix"].append(float(ms.value))

        def run_kernel():
            assert L.beamformer_hip_autocorrelate_last_frames(K, weights_ptr, K, LAGS, 0, C.byref(first), C.byref(ms)), lib.last_error()
            device_ms["kernel"].append(float(ms.value))

        def run_identity():
            assert L.beamformer_hip_autocorrelate_last_frames(K, None, K, LAGS, 0, C.byref(first), C.byref(ms)), lib.last_error()
            device_ms["identity"].append(float(ms.value))

        # the projector of the ensemble, and (b) against (a) on the same K frames
        queue_ensemble()
        gram, _, _ = lib.gram_last_frames(K)
        projector, _ = lib.clutter_projector(gram, 1)
        weights[:] = projector
        now = leg_now().copy()
        queue_ensemble()
        before = leg_before()
        finite = np.isfinite(before)
        assert np.array_equal(np.isfinite(now), finite), "the device's lags are not finite where numpy's are"
        off = float(np.abs(now[finite] - before[finite]).max() / np.abs(before[0][finite[0]]).max())
        assert not now[0].imag[finite[0]].any() and off <= 1e-4, f"the device's lags are not numpy's: {off:.3e} of the largest power"

        steps = (("before", leg_before), ("now", leg_now), ("mix", run_mix), ("kernel", run_kernel), ("identity", run_identity))
        t = {label: [] for label, _ in steps}
        for n in range(2 + args.repeats):
            for label, run in steps:
                queue_ensemble()
                assert L.beamformer_hip_synchronize()
                t0 = time.perf_counter()
                run()
                if n >= 2:
                    t[label].append(time.perf_counter() - t0)
        for v in device_ms.values():
            del v[:2]
        kernel_s = statistics.median(device_ms["kernel"]) * 1e-3
        kernel_bytes, kernel_flop = (K + LAGS) * frame_bytes, (8 * K * K + 8 * LAGS * K) * voxels
        least_bytes_s, least_flop_s = kernel_bytes / COPY_RATE_MEASURED, kernel_flop / F32_PEAK
        row = {"shape": name, "points": list(points), "frames": K, "lags": LAGS, "frame_bytes": frame_bytes,
               "before_mix_download_numpy": summary(t["before"]), "now_autocorrelate_download": summary(t["now"]),
               "mix_call": summary(t["mix"]), "kernel_call": summary(t["kernel"]), "identity_call": summary(t["identity"]),
               "mix_device_us": summary(device_ms["mix"], 1e3), "kernel_device_us": summary(device_ms["kernel"], 1e3),
               "identity_device_us": summary(device_ms["identity"], 1e3),
               "device_lags_against_numpy": off,
               "kernel_bytes": kernel_bytes, "kernel_flop": kernel_flop, "kernel_source_reads": (K + 15) // 16,
               "kernel_bytes_per_second": kernel_bytes / kernel_s, "kernel_flop_per_second": kernel_flop / kernel_s,
               "kernel_share_of_copy_rate": kernel_bytes / kernel_s / COPY_RATE_MEASURED, "kernel_share_of_f32_peak": kernel_flop / kernel_s / F32_PEAK,
               "kernel_binds": "bytes" if least_bytes_s > least_flop_s else "flop", "kernel_least_time_us": max(least_bytes_s, least_flop_s) * 1e6}
        row["now_over_before"] = row["now_autocorrelate_download"]["median_us"] / row["before_mix_download_numpy"]["median_us"]
        row["kernel_over_mix_device"] = row["kernel_device_us"]["median_us"] / row["mix_device_us"]["median_us"]
        row["now_beats_before"] = bool(row["now_autocorrelate_download"]["median_us"] < row["before_mix_download_numpy"]["median_us"])
        row["spreads_apart"] = bool(row["now_autocorrelate_download"]["max_us"] < row["before_mix_download_numpy"]["min_us"])
        rows.append(row)
        print(json.dumps(row), flush=True)

result = {"commit": args.commit, "repeats": args.repeats,
          "timing": "host clock around each step (every one ends in a synchronise), rounds before, now, mix, kernel, identity in turn after two "
                    "warm-up rounds, the ensemble queued again before every step, outside its window; device: events around the one launch of each call",
          "peaks": {"copy_rate_measured_float4": COPY_RATE_MEASURED, "hbm_specified": HBM_PEAK_SPEC, "f32_flop_per_second": F32_PEAK},
          "now_beats_before_everywhere": all(r["now_beats_before"] for r in rows),
          "rows": rows}
print(json.dumps({k: v for k, v in result.items() if k != "rows"}))
if args.json:
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1)
