"""What accumulating the localisation map on the device buys (beamformer_hip_accumulate_peaks_last_frames, csrc/frame_peaks.hip).  BASELINE
config 1's RF (ogl_beamforming_amd/configs.py: 64 channels, one transmit, complex frames) gives the frames: K = 8 and 64 frames of a
256 x 1 x 256 plane (a variants push under K speeds of sound) and 1024 patch frames of 17 x 1 x 17 (one views push, the patches on a
32 x 32 lattice over the plane), pushed once.  The map is 1021 x 1 x 1021 over the plane: four times finer an axis.  At thresholds of
0.5 and 0.1 of each frame's own max_abs,
  (a) accumulated: the call end to end (host clock around the C entry, which ends in its one synchronise; the rows allocated once), and
      its device_ms (events around its four launches);
  (b) the route it replaces: beamformer_hip_find_peaks_last_frames with its records downloaded (cap 65536, buffers allocated once), then
      the records binned on the host with the numpy reference (tests/localisation_ref.py: vectorised, one pass a frame) -- timed as the
      call alone and as call plus binning.
(a) and (b) are timed in turn, --repeats rounds after two warm-up rounds; median, smallest and largest of each.  Before anything is
timed the device's map is compared with (b)'s, byte for byte: a rate of wrong maps is no rate.  The map is reset before every timed
(a) outside the clock (the reset is a memset a caller pays once a map, not once a call).
Run from the repository root on a GPU box:
PYTHONPATH=. python tools/localisation_rate.py --json profiles/localisation_rate.json --markdown profiles/localisation_rate.md [--commit ID]"""
import argparse
import ctypes as C
import json
import statistics
import time

import numpy as np

from ogl_beamforming_amd import configs, lib, params as P
from tests import localisation_ref as ref

ap = argparse.ArgumentParser()
ap.add_argument("--fractions", default="0.5,0.1")
ap.add_argument("--repeats", type=int, default=15)
ap.add_argument("--json", default="")
ap.add_argument("--markdown", default="")
ap.add_argument("--commit", default="")
args = ap.parse_args()

CAP = P.HIP_MAX_PEAKS_PER_FRAME
L = lib.library()
L.beamformer_set_global_timeout(0xFFFFFFFF)
acq = configs.config(1)
rf = np.ascontiguousarray(acq.rf)
for s, fp in enumerate(acq.filters):
    assert L.beamformer_create_filter(C.byref(fp), s, 0), lib.last_error()
m = list(acq.bp.das_voxel_transform)              # das_transform_2d_xz: x extent m[0] from m[12], depth extent m[6] from m[14]
x0, x1, z0, z1 = m[12], m[12] + m[0], m[14], m[14] + m[6]
PLANE = (256, 1, 256)
MAP = (1021, 1, 1021)
grid = lib.view(MAP, (x0, 0.0, z0), (x1, 1e-3, z1))            # a y extent: the map's transform has to be regular
bp = type(acq.bp).from_buffer_copy(acq.bp)
bp.das_voxel_transform[:] = [float(v) for v in configs.das_transform_3d((x0, 0.0, z0), (x1, 0.0, z1))]
bp.output_points[:3] = list(PLANE)


def summary(times):
    return {"median_us": statistics.median(times) * 1e6, "min_us": min(times) * 1e6, "max_us": max(times) * 1e6, "runs": len(times)}


def plane_frames(K):
    variants = [lib.variant_of(bp, speed_of_sound=1400.0 + 280.0 * (k + 0.5) / K) for k in range(K)]
    frames = lib.beamform_variants(bp, rf, variants, acq.filters)
    assert frames.shape == (K, PLANE[2], PLANE[1], PLANE[0])
    A = lib.map_placement(list(bp.das_voxel_transform), PLANE, list(grid.das_voxel_transform), MAP)
    return K, np.tile(A.reshape(-1), K).reshape(K, 12), int(frames[0].nbytes)


def patch_frames():
    """1024 patches of 17 x 1 x 17 voxels spanning 4 voxels of the plane's pitch, centred on a 32 x 32 lattice"""
    px, pz = (x1 - x0) / 255.0, (z1 - z0) / 255.0
    views = []
    for j in range(32):
        for i in range(32):
            cx, cz = x0 + (4.0 + 8.0 * i) * px, z0 + (4.0 + 8.0 * j) * pz
            views.append(lib.view((17, 1, 17), (cx - 2 * px, 0.0, cz - 2 * pz), (cx + 2 * px, 0.0, cz + 2 * pz)))
    frames = lib.beamform_views(bp, rf, views, acq.filters)
    assert len(frames) == 1024 and frames[0].shape == (17, 1, 17)
    A = np.stack([lib.map_placement(list(v.das_voxel_transform), (17, 1, 17), list(grid.das_voxel_transform), MAP).reshape(-1) for v in views])
    return 1024, A, int(frames[0].nbytes)


rows = []
for name, make in (("8 x 256x1x256", lambda: plane_frames(8)), ("64 x 256x1x256", lambda: plane_frames(64)), ("1024 x 17x1x17", patch_frames)):
    K, placements, frame_bytes = make()                  # pushed once: neither route touches the ring
    placements = np.ascontiguousarray(placements, np.float64)
    placements_ptr = placements.ctypes.data_as(C.POINTER(C.c_double))
    metrics, _ = lib.score_last_frames(K)
    deposits = (P.HipMapDeposits * K)()
    found_rows = (P.HipFramePeaks * K)()
    records = np.empty(K * CAP, np.dtype(P.HipFramePeak))                 # (virtual memory: only what a call stores is touched)
    records_ptr = records.ctypes.data_as(C.POINTER(P.HipFramePeak))
    total, ms = C.c_uint32(0), C.c_float(0)
    for fraction in (float(v) for v in args.fractions.split(",")):
        levels = (C.c_float * K)(*[float(np.float32(fraction) * np.float32(metrics[k].max_abs)) for k in range(K)])
        device_ms = {"accumulate": [], "find_peaks": []}

        def accumulate():
            assert L.beamformer_hip_accumulate_peaks_last_frames(K, None, levels, K, placements_ptr, K, 1, deposits, C.byref(ms)), lib.last_error()
            device_ms["accumulate"].append(float(ms.value))

        def find_peaks():
            assert L.beamformer_hip_find_peaks_last_frames(K, None, levels, K, CAP, found_rows, records_ptr, C.byref(total), C.byref(ms)), lib.last_error()
            device_ms["find_peaks"].append(float(ms.value))

        host_map = np.zeros((MAP[2], MAP[1], MAP[0]), np.uint32)       # the host route keeps its map too: allocated once, added to

        def find_peaks_and_bin():
            find_peaks()
            for k in range(K):
                mine = records[int(found_rows[k].first):int(found_rows[k].first) + int(found_rows[k].stored)]
                ref.deposit_records(host_map, mine["index"], mine["offset"], placements[k])

        lib.localisation_map_reset(MAP)
        accumulate()
        find_peaks_and_bin()
        counts, info = lib.localisation_map_copy()
        assert counts.tobytes() == host_map.tobytes() and all(r.stored == r.found for r in found_rows)
        accumulate(); find_peaks_and_bin()
        for times in device_ms.values():
            times.clear()
        t = {"accumulate": [], "find_peaks": [], "find_peaks_and_bin": []}
        for n in range(args.repeats):
            for label, run in (("accumulate", accumulate), ("find_peaks", find_peaks), ("find_peaks_and_bin", find_peaks_and_bin)):
                if label == "accumulate":
                    lib.localisation_map_reset(MAP)
                if label == "find_peaks_and_bin":
                    device_ms["find_peaks"], kept = [], device_ms["find_peaks"]      # (its device time is the call's: counted once)
                assert L.beamformer_hip_synchronize()
                t0 = time.perf_counter()
                run()
                t[label].append(time.perf_counter() - t0)
                if label == "find_peaks_and_bin":
                    device_ms["find_peaks"] = kept
        row = {"case": name, "frames": K, "frame_bytes": frame_bytes, "map_points": list(MAP), "threshold_fraction_of_max_abs": fraction,
               "peaks_found": int(sum(int(r.found) for r in deposits)), "deposited": int(sum(int(r.deposited) for r in deposits)),
               "outside": int(sum(int(r.outside) for r in deposits)), "record_bytes_downloaded": int(total.value) * 32,
               "accumulate": summary(t["accumulate"]), "find_peaks": summary(t["find_peaks"]), "find_peaks_and_bin": summary(t["find_peaks_and_bin"])}
        for label, times in device_ms.items():
            row[label + "_device_us"] = {"median_us": statistics.median(times) * 1e3, "min_us": min(times) * 1e3, "max_us": max(times) * 1e3}
        row["accumulate_over_find_peaks"] = row["accumulate"]["median_us"] / row["find_peaks"]["median_us"]
        row["accumulate_over_find_peaks_and_bin"] = row["accumulate"]["median_us"] / row["find_peaks_and_bin"]["median_us"]
        row["spreads_apart_from_find_peaks"] = bool(row["accumulate"]["max_us"] < row["find_peaks"]["min_us"] or row["find_peaks"]["max_us"] < row["accumulate"]["min_us"])
        row["spreads_apart_from_find_peaks_and_bin"] = bool(row["accumulate"]["max_us"] < row["find_peaks_and_bin"]["min_us"])
        rows.append(row)
        print(json.dumps(row), flush=True)
lib.localisation_map_reset(None)

result = {"commit": args.commit, "repeats": args.repeats,
          "timing": "host clock around each call (every one ends in a synchronise), a, b, b + binning in turn after two warm-up rounds; the map reset "
                    "outside the clock; device: events around the launches of each call",
          "rows": rows}
if args.json:
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1)
table = ["| frames | threshold | peaks | accumulate: wall us (min .. max) | device us | find_peaks + download: wall us (min .. max) | device us | + host binning: wall us (min .. max) |",
         "|---|---|---|---|---|---|---|---|"]
for r in rows:
    def cell(s):
        return f"{s['median_us']:.0f} ({s['min_us']:.0f} .. {s['max_us']:.0f})"
    table.append(f"| {r['case']} | {r['threshold_fraction_of_max_abs']} | {r['peaks_found']} | {cell(r['accumulate'])} | {r['accumulate_device_us']['median_us']:.0f} | "
                 f"{cell(r['find_peaks'])} | {r['find_peaks_device_us']['median_us']:.0f} | {cell(r['find_peaks_and_bin'])} |")
print("\n".join(table))
if args.markdown:
    with open(args.markdown, "w") as f:
        f.write("\n".join(table) + "\n")
