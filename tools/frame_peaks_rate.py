"""What finding peaks on the device buys (beamformer_hip_find_peaks_last_frames, csrc/frame_peaks.hip): the K frames of a variants push
-- BASELINE config 1's RF (ogl_beamforming_amd/configs.py: 64 channels, one transmit, complex frames) under K speeds of sound, on a
256 x 1 x 256 plane and on a 64 x 64 x 64 volume, K = 1, 8, 64 -- are pushed once and then, at thresholds of 0.5 and 0.1 of each frame's
own max_abs and at threshold 0 (the worst case: every wave walks its neighbourhood, and a frame of speckle has a peak every dozen voxels),
  (a) searched: the call end to end (host clock around the C entry, which ends in a synchronise; the caller's buffers allocated once),
      and its device_ms (events around the mark and scan launches and around the emit launch, added);
  (b) downloaded: beamformer_get_last_frames of the same K frames alone -- what a caller who wants the peaks had before;
  (c) downloaded and searched on the host with the numpy reference (tests/frame_peaks_ref.py).
The three are timed in turn (a, b, c, a, b, c, ...), --repeats rounds after two warm-up rounds ((c), the slow one, takes part in the
first --host-repeats of them); median, smallest and largest of each.
bytes_per_second: the K frames' bytes, read once, over the median device_ms, beside the HBM peak of the MI355X -- frames of these sizes
were just written and mostly still sit in the Infinity Cache, so the figure says how far the search is from any memory bound, not which
memory it read.
The claim the feature makes, recorded as "claim_holds": at K = 8 on the plane and threshold 0.5, (a) takes less time than (b) with the
spreads apart -- the slowest (a) below the fastest (b).  Run from the repository root on a GPU box:
PYTHONPATH=. python tools/frame_peaks_rate.py --json profiles/frame_peaks_rate.json [--commit ID]"""
import argparse
import ctypes as C
import json
import statistics
import time

import numpy as np

from ogl_beamforming_amd import configs, lib, params as P
from tests import frame_peaks_ref as ref

ap = argparse.ArgumentParser()
ap.add_argument("--counts", default="1,8,64")
ap.add_argument("--fractions", default="0.5,0.1,0")
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--host-repeats", type=int, default=3, help="rounds in which (c), the slow one, takes part")
ap.add_argument("--json", default="")
ap.add_argument("--commit", default="")
args = ap.parse_args()

HBM_PEAK_SPEC, HBM_PEAK_MEASURED = 8.0e12, 6.29e12
CAP = P.HIP_MAX_PEAKS_PER_FRAME
L = lib.library()
L.beamformer_set_global_timeout(0xFFFFFFFF)
acq = configs.config(1)
rf = np.ascontiguousarray(acq.rf)
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
        frames = lib.beamform_variants(bp, rf, variants, acq.filters)          # pushed once: searching and downloading leave the ring alone
        assert frames.dtype == np.complex64 and frames.shape == (K, points[2], points[1], points[0])
        metrics, _ = lib.score_last_frames(K)
        raw = np.zeros(K * frame_bytes // 4, np.float32)
        found_rows = (P.HipFramePeaks * K)()
        records = np.empty(K * CAP, np.dtype(P.HipFramePeak))                 # (virtual memory: only what a call stores is touched)
        records_ptr = records.ctypes.data_as(C.POINTER(P.HipFramePeak))
        total, ms = C.c_uint32(0), C.c_float(0)
        for fraction in (float(v) for v in args.fractions.split(",")):
            thresholds = [float(np.float32(fraction) * np.float32(metrics[k].max_abs)) for k in range(K)]
            levels = (C.c_float * K)(*thresholds)
            device_ms = []

            def search():
                assert L.beamformer_hip_find_peaks_last_frames(K, None, levels, K, CAP, found_rows, records_ptr, C.byref(total), C.byref(ms)), lib.last_error()
                device_ms.append(float(ms.value))

            def download():
                assert L.beamformer_get_last_frames(raw.ctypes.data_as(C.c_void_p), raw.nbytes, K), lib.last_error()

            def download_and_search():
                download()
                each = raw.reshape(K, frame_bytes // 4)[:, : 2 * voxels]
                return [ref.peaks(np.ascontiguousarray(each[k]).view(np.complex64).reshape(points[2], points[1], points[0]), thresholds[k], cap=CAP)
                        for k in range(K)]

            search()
            expected = download_and_search()
            for k in range(K):                    # the lists are the frames': a rate of wrong lists is no rate
                mine = records[int(found_rows[k].first):int(found_rows[k].first) + int(found_rows[k].stored)]
                assert int(found_rows[k].found) == expected[k]["found"] and int(found_rows[k].above_threshold) == expected[k]["above_threshold"], k
                assert np.array_equal(mine["index"], expected[k]["index"]), k
            search(); download()
            device_ms.clear()
            t = {"search": [], "download": [], "download_and_numpy": []}
            for n in range(args.repeats):
                for label, run in (("search", search), ("download", download), ("download_and_numpy", download_and_search)):
                    if label == "download_and_numpy" and n >= args.host_repeats:
                        continue
                    assert L.beamformer_hip_synchronize()
                    t0 = time.perf_counter()
                    run()
                    t[label].append(time.perf_counter() - t0)
            row = {"shape": name, "points": list(points), "frames": K, "frame_bytes": frame_bytes, "threshold_fraction_of_max_abs": fraction,
                   "peaks_found": int(sum(int(r.found) for r in found_rows)), "peaks_stored": int(total.value),
                   "above_threshold": int(sum(int(r.above_threshold) for r in found_rows)),
                   "search": summary(t["search"]), "download": summary(t["download"]), "download_and_numpy": summary(t["download_and_numpy"]),
                   "search_device_us": {"median_us": statistics.median(device_ms) * 1e3, "min_us": min(device_ms) * 1e3, "max_us": max(device_ms) * 1e3}}
            row["search_over_download"] = row["search"]["median_us"] / row["download"]["median_us"]
            row["search_over_download_and_numpy"] = row["search"]["median_us"] / row["download_and_numpy"]["median_us"]
            row["spreads_apart"] = bool(row["search"]["max_us"] < row["download"]["min_us"])
            row["bytes_per_second"] = K * frame_bytes / (statistics.median(device_ms) * 1e-3)
            row["share_of_hbm_peak_spec"] = row["bytes_per_second"] / HBM_PEAK_SPEC
            row["share_of_hbm_peak_measured"] = row["bytes_per_second"] / HBM_PEAK_MEASURED
            rows.append(row)
            print(json.dumps(row), flush=True)

claimed = [r for r in rows if r["shape"] == "256x1x256" and r["frames"] == 8 and r["threshold_fraction_of_max_abs"] == 0.5]
claim = claimed[0] if claimed else None
result = {"commit": args.commit, "repeats": args.repeats, "host_repeats": args.host_repeats,
          "timing": "host clock around each call (every one ends in a synchronise), rounds a, b, c in turn after two warm-up rounds; device: events around mark + scan and around emit, added",
          "hbm_peak_bytes_per_second": {"specified": HBM_PEAK_SPEC, "measured_float4_copy": HBM_PEAK_MEASURED},
          "claim": "at 8 frames of 256 x 1 x 256 and a threshold of 0.5 of each frame's max_abs, finding the peaks on the device takes less time than "
                   "downloading the frames, the slowest search below the fastest download",
          "claim_holds": None if claim is None else bool(claim["search"]["median_us"] < claim["download"]["median_us"] and claim["spreads_apart"]),
          "rows": rows}
print(json.dumps({k: v for k, v in result.items() if k != "rows"}))
if args.json:
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1)
