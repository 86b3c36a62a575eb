"""What scoring frames on the device buys (beamformer_hip_score_last_frames, csrc/frame_metrics.hip): the K frames of a variants push --
BASELINE config 1's RF (ogl_beamforming_amd/configs.py: 64 channels, one transmit, complex frames) under K speeds of sound, on a
256 x 1 x 256 plane and on a 64 x 64 x 64 volume, K = 1, 8, 64 -- are pushed once and then
  (a) scored: score_last_frames(K) end to end (host clock around the call, which ends in a synchronise), and its device_ms (two events
      around the two launches);
  (b) downloaded: beamformer_get_last_frames of the same K frames alone -- the cheapest thing a caller who wants these numbers had before;
  (c) downloaded and scored on the host with the numpy reference (tests/frame_metrics_ref.py).
The three are timed in turn (a, b, c, a, b, c, ...), --repeats rounds after two warm-up rounds ((c), the slow one, takes part in the
first --host-repeats of them); median, smallest and largest of each.
bytes_per_second: the K frames' bytes, read once, over the median device_ms, beside the HBM peak of the MI355X (8.0 TB/s specified,
6.29 TB/s measured with a float4 copy) -- frames of these sizes were just written and mostly still sit in the 256 MiB Infinity Cache, so
the figure says how far the reduction is from any memory bound, not which memory it read.
The claim the feature makes, recorded as "claim_holds": at K = 8 on the plane, (a) takes less time than (b).  Run from the repository
root on a GPU box:
PYTHONPATH=. python tools/frame_metrics_rate.py --json profiles/frame_metrics_rate.json [--commit ID]"""
import argparse
import ctypes as C
import json
import statistics
import time

import numpy as np

from ogl_beamforming_amd import configs, lib, params as P
from tests import frame_metrics_ref as ref

ap = argparse.ArgumentParser()
ap.add_argument("--counts", default="1,8,64")
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--host-repeats", type=int, default=3, help="rounds in which (c), the slow one, takes part")
ap.add_argument("--json", default="")
ap.add_argument("--commit", default="")
args = ap.parse_args()

HBM_PEAK_SPEC, HBM_PEAK_MEASURED = 8.0e12, 6.29e12
L = lib.library()
L.beamformer_set_global_timeout(0xFFFFFFFF)
acq = configs.config(1)
rf = np.ascontiguousarray(acq.rf)
ptr, size = rf.ctypes.data_as(C.c_void_p), rf.nbytes
for s, fp in enumerate(acq.filters):
    assert L.beamformer_create_filter(C.byref(fp), s, 0), lib.last_error()
m = list(acq.bp.das_voxel_transform)              # das_transform_2d_xz: x extent m[0] from m[12], depth extent m[6] from m[14]
x0, x1, z0, z1 = m[12], m[12] + m[0], m[14], m[14] + m[6]
SHAPES = {"256x1x256": ((256, 1, 256), (x0, 0.0, z0), (x1, 0.0, z1)), "64x64x64": ((64, 64, 64), (x0, -2e-3, z0), (x1, 2e-3, z1))}


def summary(times):
    return {"median_us": statistics.median(times) * 1e6, "min_us": min(times) * 1e6, "max_us": max(times) * 1e6, "runs": len(times)}


rows = []
for name, (points, lo, hi) in SHAPES.items():
    bp = type(acq.bp).from_buffer_copy(acq.bp)
    bp.das_voxel_transform[:] = [float(v) for v in configs.das_transform_3d(lo, hi)]
    bp.output_points[:3] = list(points)
    voxels = int(np.prod(points))
    frame_bytes = (voxels * 8 + 63) // 64 * 64
    for K in (int(v) for v in args.counts.split(",")):
        variants = [lib.variant_of(bp, speed_of_sound=1400.0 + 280.0 * (k + 0.5) / K) for k in range(K)]
        frames = lib.beamform_variants(bp, rf, variants, acq.filters)          # pushed once: scoring and downloading leave the ring alone
        assert frames.dtype == np.complex64 and frames.shape == (K, points[2], points[1], points[0])
        raw = np.zeros(K * frame_bytes // 4, np.float32)
        device_ms = []

        def score():
            found, ms = lib.score_last_frames(K)
            device_ms.append(ms)
            return found

        def download():
            assert L.beamformer_get_last_frames(raw.ctypes.data_as(C.c_void_p), raw.nbytes, K), lib.last_error()

        def download_and_score():
            download()
            each = raw.reshape(K, frame_bytes // 4)[:, : 2 * voxels]
            return [ref.metrics(np.ascontiguousarray(each[k]).view(np.complex64).reshape(points[2], points[1], points[0])) for k in range(K)]

        found, expected = score(), download_and_score()
        for k in range(K):                        # the rows are the frames': a rate of wrong numbers is no rate
            assert found[k].voxels == expected[k]["voxels"] and abs(found[k].sum_abs2 - expected[k]["sum_abs2"]) <= 2e-6 * expected[k]["sum_abs2"], k
        score(); download()
        device_ms.clear()
        t = {"score": [], "download": [], "download_and_numpy": []}
        for n in range(args.repeats):
            for label, run in (("score", score), ("download", download), ("download_and_numpy", download_and_score)):
                if label == "download_and_numpy" and n >= args.host_repeats:
                    continue
                assert L.beamformer_hip_synchronize()
                t0 = time.perf_counter()
                run()
                t[label].append(time.perf_counter() - t0)
        row = {"shape": name, "points": list(points), "frames": K, "frame_bytes": frame_bytes,
               "score": summary(t["score"]), "download": summary(t["download"]), "download_and_numpy": summary(t["download_and_numpy"]),
               "score_device_us": {"median_us": statistics.median(device_ms) * 1e3, "min_us": min(device_ms) * 1e3, "max_us": max(device_ms) * 1e3}}
        row["score_over_download"] = row["score"]["median_us"] / row["download"]["median_us"]
        row["score_over_download_and_numpy"] = row["score"]["median_us"] / row["download_and_numpy"]["median_us"]
        row["bytes_per_second"] = K * frame_bytes / (statistics.median(device_ms) * 1e-3)
        row["share_of_hbm_peak_spec"] = row["bytes_per_second"] / HBM_PEAK_SPEC
        row["share_of_hbm_peak_measured"] = row["bytes_per_second"] / HBM_PEAK_MEASURED
        rows.append(row)
        print(json.dumps(row), flush=True)

claimed = [r for r in rows if r["shape"] == "256x1x256" and r["frames"] == 8]
claim = claimed[0] if claimed else None
result = {"commit": args.commit, "repeats": args.repeats, "host_repeats": args.host_repeats,
          "timing": "host clock around each call (every one ends in a synchronise), rounds a, b, c in turn after two warm-up rounds; device: two events around the two launches",
          "hbm_peak_bytes_per_second": {"specified": HBM_PEAK_SPEC, "measured_float4_copy": HBM_PEAK_MEASURED},
          "claim": "at 8 frames of 256 x 1 x 256, scoring on the device takes less time than downloading the frames",
          "claim_holds": None if claim is None else bool(claim["score"]["median_us"] < claim["download"]["median_us"]), "rows": rows}
print(json.dumps({k: v for k, v in result.items() if k != "rows"}))
if args.json:
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1)
