"""What selecting quantiles on the device costs (beamformer_hip_quantiles_last_frames, csrc/frame_quantiles.hip): the K frames of a
variants push -- BASELINE config 1's RF (ogl_beamforming_amd/configs.py: 64 channels, one transmit, complex frames) under K speeds of
sound, on a 256 x 1 x 256 plane and on a 64 x 64 x 64 volume, K = 1, 8, 64 -- are pushed once and then
  (a) ranked: quantiles_last_frames(K, fractions) end to end (host clock around the call, which ends in a synchronise), and its device_ms
      (two events around the memset and the six launches), without and with the histograms;
  (b) scored: score_last_frames(K), the reduce call that reads the same frames ONCE, as a yardstick for one read;
  (c) downloaded: beamformer_get_last_frames of the same K frames alone -- what a caller who wants a quantile had to do first;
  (d) downloaded and ranked on the host with the numpy reference (tests/frame_quantiles_ref.py).
The four are timed in turn, --repeats rounds after two warm-up rounds ((d), the slow one, takes part in the first --host-repeats of
them); median, smallest and largest of each.
read_bytes_per_second: 3 x the K frames' bytes -- the three count passes each read every voxel -- over the median device_ms, beside the
rate of a float4 copy on the MI355X (6.29 TB/s measured) -- frames of these sizes were just written and mostly still sit in the 256 MiB
Infinity Cache, so the figure says how far the selection is from any memory bound, not which memory it read.
Run from the repository root on a GPU box:
PYTHONPATH=. python tools/frame_quantiles_rate.py --json profiles/frame_quantiles_rate.json [--commit ID]"""
import argparse
import ctypes as C
import json
import statistics
import time

import numpy as np

from ogl_beamforming_amd import configs, lib
from tests import frame_quantiles_ref as ref

ap = argparse.ArgumentParser()
ap.add_argument("--counts", default="1,8,64")
ap.add_argument("--fractions", default="0.05,0.5,0.99,0.999")
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--host-repeats", type=int, default=2, help="rounds in which (d), the slow one, takes part")
ap.add_argument("--json", default="")
ap.add_argument("--commit", default="")
args = ap.parse_args()

COPY_RATE_MEASURED = 6.29e12
FRACTIONS = [float(v) for v in args.fractions.split(",")]
L = lib.library()
L.beamformer_set_global_timeout(0xFFFFFFFF)
acq = configs.config(1)
rf = np.ascontiguousarray(acq.rf)
for s, fp in enumerate(acq.filters):
    assert L.beamformer_create_filter(C.byref(fp), s, 0), lib.last_error()
m = list(acq.bp.das_voxel_transform)              # das_transform_2d_xz: x extent m[0] from m[12], depth extent m[6] from m[14]
x0, x1, z0, z1 = m[12], m[12] + m[0], m[14], m[14] + m[6]
SHAPES = {"256x1x256": ((256, 1, 256), (x0, 0.0, z0), (x1, 0.0, z1)), "64x64x64": ((64, 64, 64), (x0, -2e-3, z0), (x1, 2e-3, z1))}


def summary(times, scale=1e6):
    return {"median_us": statistics.median(times) * scale, "min_us": min(times) * scale, "max_us": max(times) * scale, "runs": len(times)}


rows = []
for name, (points, lo, hi) in SHAPES.items():
    bp = type(acq.bp).from_buffer_copy(acq.bp)
    bp.das_voxel_transform[:] = [float(v) for v in configs.das_transform_3d(lo, hi)]
    bp.output_points[:3] = list(points)
    voxels = int(np.prod(points))
    frame_bytes = (voxels * 8 + 63) // 64 * 64
    for K in (int(v) for v in args.counts.split(",")):
        variants = [lib.variant_of(bp, speed_of_sound=1400.0 + 280.0 * (k + 0.5) / K) for k in range(K)]
        frames = lib.beamform_variants(bp, rf, variants, acq.filters)          # pushed once: every call below leaves the ring alone
        assert frames.dtype == np.complex64 and frames.shape == (K, points[2], points[1], points[0])
        raw = np.zeros(K * frame_bytes // 4, np.float32)
        device_ms = {"rank": [], "rank_with_histograms": [], "score": []}

        def rank():
            found = lib.quantiles_last_frames(K, FRACTIONS)
            device_ms["rank"].append(found[3])
            return found

        def rank_with_histograms():
            device_ms["rank_with_histograms"].append(lib.quantiles_last_frames(K, FRACTIONS, histograms=True)[3])

        def score():
            device_ms["score"].append(lib.score_last_frames(K)[1])

        def download():
            assert L.beamformer_get_last_frames(raw.ctypes.data_as(C.c_void_p), raw.nbytes, K), lib.last_error()

        def download_and_rank():
            download()
            each = raw.reshape(K, frame_bytes // 4)[:, : 2 * voxels]
            return [ref.quantiles(np.ascontiguousarray(each[k]).view(np.complex64).reshape(points[2], points[1], points[0]), FRACTIONS) for k in range(K)]

        (found_rows, found, _, _), expected = rank(), download_and_rank()
        for k in range(K):                        # the records are the frames': a rate of wrong numbers is no rate
            assert int(found_rows[k].voxels) == expected[k]["voxels"]
            for j, q in enumerate(expected[k]["rows"]):
                got = found[k * len(FRACTIONS) + j]
                assert (int(got.rank), int(got.below), int(got.equal)) == (q["rank"], q["below"], q["equal"]) and got.value == q["value"], (k, j)
        rank_with_histograms(); score(); download()
        for times in device_ms.values():
            times.clear()
        runs = (("rank", rank), ("rank_with_histograms", rank_with_histograms), ("score", score), ("download", download), ("download_and_numpy", download_and_rank))
        t = {label: [] for label, _ in runs}
        for n in range(args.repeats):
            for label, run in runs:
                if label == "download_and_numpy" and n >= args.host_repeats:
                    continue
                assert L.beamformer_hip_synchronize()
                t0 = time.perf_counter()
                run()
                t[label].append(time.perf_counter() - t0)
        row = {"shape": name, "points": list(points), "frames": K, "frame_bytes": frame_bytes, "fractions": FRACTIONS}
        row.update({label: summary(times) for label, times in t.items()})
        row.update({label + "_device_us": summary(times, 1e3) for label, times in device_ms.items()})
        row["rank_over_download"] = row["rank"]["median_us"] / row["download"]["median_us"]
        row["rank_device_over_score_device"] = row["rank_device_us"]["median_us"] / row["score_device_us"]["median_us"]
        row["read_bytes_per_second"] = 3 * K * frame_bytes / (row["rank_device_us"]["median_us"] * 1e-6)
        row["share_of_copy_rate_measured"] = row["read_bytes_per_second"] / COPY_RATE_MEASURED
        rows.append(row)
        print(json.dumps(row), flush=True)

result = {"commit": args.commit, "repeats": args.repeats, "host_repeats": args.host_repeats,
          "timing": "host clock around each call (every one ends in a synchronise), rounds in turn after two warm-up rounds; device: two events around the call's launches",
          "copy_rate_measured_float4": COPY_RATE_MEASURED, "rows": rows}
if args.json:
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1)
