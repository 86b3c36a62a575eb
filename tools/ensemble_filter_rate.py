"""What filtering an ensemble on the device buys (beamformer_hip_gram_last_frames, beamformer_hip_clutter_projector,
beamformer_hip_mix_last_frames; csrc/ensemble.hip): K frames of variants pushes -- BASELINE config 1's RF (ogl_beamforming_amd/configs.py:
64 channels, one transmit, complex frames) under K speeds of sound, at most 64 a push -- on a 256 x 1 x 256 plane (K = 8, 64, 256) and
on a 64 x 64 x 64 volume (K = 8, 64) are queued once and then, in turn,
  (a) gram:      the Gram call end to end (host clock around the C entry, which ends in a synchronise) and its device_ms;
  (b) download:  beamformer_get_last_frames of the K newest frames alone -- the only way to filter before;
  (c) mix:       K -> K frames under the projector of (a)'s matrix, asked for its device_ms (so the call ends in a synchronise);
  (d) filter:    gram + projector (host, Jacobi) + mix (not asked for its time) + beamformer_hip_synchronize: the whole step;
timed a, b, c, d, a, ... for --repeats rounds after two warm-up rounds: median, smallest and largest of each, the projector's host time
apart.  (c) and (d) queue K new frames each: from the second round on the K newest frames are filtered frames, of the same size and
kind (the projector is idempotent: they stay bounded), and (b) downloads those.  Once per ensemble, before the rounds:
  (e) host:      the download, numpy's Gram matrix, numpy.linalg.eigh and the matrix product -- what a caller did before;
the device's matrix is checked against numpy's there.
The mix's rates: bytes = K frames read once and K written, flop = 8 K K voxels, over the median device_ms, beside the measured copy
rate and the f32 peak of the MI355X; "binds" names the larger of the two least times.  Source frames are read ceil(K / 16) times by the
kernel; what the reads after the first cost is the distance between the byte rate and the copy rate.
The claim the feature makes, recorded as "claim_holds": at K = 64 on the plane (d) takes less time than (b).  Run from the repository
root on a GPU box: PYTHONPATH=. python tools/ensemble_filter_rate.py --json profiles/ensemble_filter_rate.json [--commit ID]"""
import argparse
import ctypes as C
import json
import statistics
import time

import numpy as np

from ogl_beamforming_amd import configs, lib, params as P

ap = argparse.ArgumentParser()
ap.add_argument("--plane-counts", default="8,64,256")
ap.add_argument("--volume-counts", default="8,64")
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--json", default="")
ap.add_argument("--commit", default="")
args = ap.parse_args()

COPY_RATE_MEASURED, HBM_PEAK_SPEC, F32_PEAK = 6.29e12, 8.0e12, 157.3e12
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


def summary(times):
    return {"median_us": statistics.median(times) * 1e6, "min_us": min(times) * 1e6, "max_us": max(times) * 1e6, "runs": len(times)}


rows = []
for name, (points, lo, hi, counts) in SHAPES.items():
    bp = type(acq.bp).from_buffer_copy(acq.bp)
    bp.das_voxel_transform[:] = [float(v) for v in configs.das_transform_3d(lo, hi)]
    bp.output_points[:3] = list(points)
    voxels = int(np.prod(points))
    frame_bytes = (voxels * 8 + 63) // 64 * 64
    for K in (int(v) for v in counts.split(",") if v):
        speeds = [1400.0 + 280.0 * (k + 0.5) / K for k in range(K)]
        for at in range(0, K, P.HIP_MAX_VARIANTS):
            lib.beamform_variants(bp, rf, [lib.variant_of(bp, speed_of_sound=v) for v in speeds[at:at + P.HIP_MAX_VARIANTS]], acq.filters)
        raw = np.zeros(K * frame_bytes // 4, np.float32)
        gram = np.zeros((K, K), np.complex128)
        gram_ptr = gram.ctypes.data_as(C.POINTER(C.c_double))
        weights, values = np.zeros((K, K), np.complex64), np.zeros(K, np.float64)
        weights_ptr, values_ptr = weights.ctypes.data_as(C.POINTER(C.c_float)), values.ctypes.data_as(C.POINTER(C.c_double))
        info, ms, first = P.HipEnsembleInfo(), C.c_float(0), C.c_uint32(0)
        gram_ms, mix_ms, projector_s = [], [], []

        def run_gram():
            assert L.beamformer_hip_gram_last_frames(K, None, gram_ptr, C.byref(info), C.byref(ms)), lib.last_error()
            gram_ms.append(float(ms.value))

        def run_projector():
            t0 = time.perf_counter()
            assert L.beamformer_hip_clutter_projector(gram_ptr, K, 1, 0, weights_ptr, values_ptr), lib.last_error()
            projector_s.append(time.perf_counter() - t0)

        def download():
            assert L.beamformer_get_last_frames(raw.ctypes.data_as(C.c_void_p), raw.nbytes, K), lib.last_error()

        def run_mix():
            assert L.beamformer_hip_mix_last_frames(K, weights_ptr, K, 0, C.byref(first), C.byref(ms)), lib.last_error()
            mix_ms.append(float(ms.value))

        def run_filter():
            assert L.beamformer_hip_gram_last_frames(K, None, gram_ptr, None, None), lib.last_error()
            run_projector()
            assert L.beamformer_hip_mix_last_frames(K, weights_ptr, K, 0, None, None), lib.last_error()
            assert L.beamformer_hip_synchronize()

        # (e), once, and the device's matrix against numpy's on the same frames
        t0 = time.perf_counter()
        download()
        frames = np.ascontiguousarray(raw.reshape(K, frame_bytes // 4)[:, : 2 * voxels]).view(np.complex64)
        good = np.isfinite(frames.real).all(axis=0) & np.isfinite(frames.imag).all(axis=0)
        f = frames[:, good].astype(np.complex128)
        host_gram = f.conj() @ f.T
        lam, vec = np.linalg.eigh(host_gram)
        kept = vec[:, : K - 1]                                                  # ascending: all but the strongest
        host_out = ((kept @ kept.conj().T).astype(np.complex64) @ frames)
        host_s = time.perf_counter() - t0
        run_gram()
        assert int(info.voxels) == int(good.sum()) and int(info.voxels) + int(info.non_finite) == voxels
        assert np.abs(gram - host_gram).max() <= 1e-9 * np.abs(host_gram).max(), "the device's Gram matrix is not numpy's"
        del f, host_out

        run_projector(); run_mix(); run_filter(); download()
        run_gram(); run_mix(); run_filter(); download()
        gram_ms.clear(); mix_ms.clear(); projector_s.clear()
        t = {"gram": [], "download": [], "mix": [], "filter": []}
        for n in range(args.repeats):
            for label, run in (("gram", run_gram), ("download", download), ("mix", run_mix), ("filter", run_filter)):
                assert L.beamformer_hip_synchronize()
                t0 = time.perf_counter()
                run()
                t[label].append(time.perf_counter() - t0)
        mix_s = statistics.median(mix_ms) * 1e-3
        mix_bytes, mix_flop = 2 * K * frame_bytes, 8 * K * K * voxels
        least_bytes_s, least_flop_s = mix_bytes / COPY_RATE_MEASURED, mix_flop / F32_PEAK
        row = {"shape": name, "points": list(points), "frames": K, "frame_bytes": frame_bytes, "voxels_finite_in_all": int(info.voxels),
               "gram": summary(t["gram"]), "download": summary(t["download"]), "mix": summary(t["mix"]), "filter": summary(t["filter"]),
               "projector_host": summary(projector_s), "host_download_eigh_matmul_once_us": host_s * 1e6,
               "gram_device_us": {"median_us": statistics.median(gram_ms) * 1e3, "min_us": min(gram_ms) * 1e3, "max_us": max(gram_ms) * 1e3},
               "mix_device_us": {"median_us": statistics.median(mix_ms) * 1e3, "min_us": min(mix_ms) * 1e3, "max_us": max(mix_ms) * 1e3},
               "mix_bytes": mix_bytes, "mix_flop": mix_flop, "mix_source_reads": (K + 15) // 16,
               "mix_bytes_per_second": mix_bytes / mix_s, "mix_flop_per_second": mix_flop / mix_s,
               "mix_share_of_copy_rate": mix_bytes / mix_s / COPY_RATE_MEASURED, "mix_share_of_f32_peak": mix_flop / mix_s / F32_PEAK,
               "mix_binds": "bytes" if least_bytes_s > least_flop_s else "flop",
               "mix_least_time_us": max(least_bytes_s, least_flop_s) * 1e6}
        for label in ("gram", "mix", "filter"):
            row[label + "_over_download"] = row[label]["median_us"] / row["download"]["median_us"]
        row["filter_spreads_apart"] = bool(row["filter"]["max_us"] < row["download"]["min_us"])
        rows.append(row)
        print(json.dumps(row), flush=True)

claimed = [r for r in rows if r["shape"] == "256x1x256" and r["frames"] == 64]
claim = claimed[0] if claimed else None
result = {"commit": args.commit, "repeats": args.repeats,
          "timing": "host clock around each step (every one ends in a synchronise), rounds gram, download, mix, filter in turn after two warm-up rounds; "
                    "device: events around the Gram call's three launches, around the mix's one",
          "peaks": {"copy_rate_measured_float4": COPY_RATE_MEASURED, "hbm_specified": HBM_PEAK_SPEC, "f32_flop_per_second": F32_PEAK},
          "claim": "at 64 frames of 256 x 1 x 256, gram + projector + mix takes less time than downloading the 64 frames",
          "claim_holds": None if claim is None else bool(claim["filter"]["median_us"] < claim["download"]["median_us"]),
          "rows": rows}
print(json.dumps({k: v for k, v in result.items() if k != "rows"}))
if args.json:
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1)
