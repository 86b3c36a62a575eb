"""What the shift correlation on the device costs (beamformer_hip_correlate_last_frames; csrc/correlate.hip), beside the project's own
yardstick for double arithmetic fed from LDS, the Gram matrix (beamformer_hip_gram_last_frames; csrc/ensemble.hip): K = 64 frames, the
whole frame as the box, in one process, in turn,
  plane    256 x 1 x 256 complex, the windows (1, 0, 1), (4, 0, 4) and (16, 0, 16): T = 9, 81 and 1089 shifts;
  volume   64 x 64 x 64 complex, the window (2, 2, 2): T = 125;
  gram     the Gram matrix of the same K frames over the same box,
each asked for its device_ms, timed gram, window, window, ... for --repeats rounds after two warm-up rounds: median, smallest and largest.
The frames are one frame of BASELINE config 1's RF (ogl_beamforming_amd/configs.py) and K scaled copies of it by a mix 1 -> K; the time
of either call does not depend on the values.
The figure of merit is complex products per second: K T V for the correlation (every frame, the reference's own included, at every shift
over the V voxels of the box; the few terms a shift loses at the frame's edge are counted as done) against K (K + 1) / 2 V for the Gram
matrix (its upper triangle).  A correlation product carries five sums (re, im, two energies, the count), a Gram product two.
Run from the repository root on a GPU box: PYTHONPATH=. python tools/motion_rate.py --json profiles/motion_rate.json [--commit ID]"""
import argparse
import ctypes as C
import json
import os
import statistics

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--json", default="")
ap.add_argument("--commit", default="")
args = ap.parse_args()

K = args.frames
CASES = {"plane": ((256, 1, 256), [(1, 0, 1), (4, 0, 4), (16, 0, 16)]), "volume": ((64, 64, 64), [(2, 2, 2)])}
largest = max(int(np.prod(points)) * 8 * K for points, _ in CASES.values())
os.environ.setdefault("BEAMFORMER_HIP_FRAME_RING_BYTES", str(3 * largest + (1 << 28)))     # (before the library loads)

from ogl_beamforming_amd import configs, lib, params as P  # noqa: E402

L = lib.library()
L.beamformer_set_global_timeout(0xFFFFFFFF)
acq = configs.config(1)
rf = np.ascontiguousarray(acq.rf)
for s, fp in enumerate(acq.filters):
    assert L.beamformer_create_filter(C.byref(fp), s, 0), lib.last_error()
m = list(acq.bp.das_voxel_transform)              # das_transform_2d_xz: x extent m[0] from m[12], depth extent m[6] from m[14]
x0, x1, z0, z1 = m[12], m[12] + m[0], m[14], m[14] + m[6]
BOXES = {"plane": ((x0, 0.0, z0), (x1, 0.0, z1)), "volume": ((x0, -2e-3, z0), (x1, 2e-3, z1))}


def summary(times):
    return {"median_us": statistics.median(times) * 1e3, "min_us": min(times) * 1e3, "max_us": max(times) * 1e3, "runs": len(times)}


rows = []
for shape, (points, windows) in CASES.items():
    lo, hi = BOXES[shape]
    bp = type(acq.bp).from_buffer_copy(acq.bp)
    bp.das_voxel_transform[:] = [float(v) for v in configs.das_transform_3d(lo, hi)]
    bp.output_points[:3] = list(points)
    voxels = int(np.prod(points))
    lib.beamform(bp, rf, acq.filters)
    if K > 1:
        lib.mix_last_frames(1, (1.0 + 0.5 * np.arange(K) / K).astype(np.complex64)[:, None])
    ms = {"gram": []}
    ms.update({w: [] for w in windows})
    for n in range(2 + args.repeats):
        _, info, t = lib.gram_last_frames(K)
        assert int(info.voxels) == voxels and int(info.non_finite) == 0
        ms["gram"].append(t)
        for w in windows:
            table, info, t = lib.correlate_last_frames(K, K // 2, w)
            ms[w].append(t)
            if n == 0:
                # the reference's own entry at no shift has everything as a term; every frame is a positive multiple of the reference
                T = int(info.shifts)
                centre = tuple(w[::-1])
                assert int(table["terms"][(0, K // 2) + centre]) == voxels and (table["re"][0][(slice(None),) + centre] > 0).all()
                found = lib.displacements_from_correlation(table, w)
                print(f"  {shape} window {w}: shifts {np.unique(found['shift'].reshape(-1, 3), axis=0).tolist()}, coefficients "
                      f"{float(found['coefficient'].min())!r} to {float(found['coefficient'].max())!r}", flush=True)
                # (the volume is the image of a linear array: it does not vary along y, so every sy ties with 0 there)
                assert not found["shift"][..., (0, 2)].any() and np.allclose(found["coefficient"], 1.0, atol=1e-6)
    for v in ms.values():
        del v[:2]
    gram = statistics.median(ms["gram"])
    gram_rate = K * (K + 1) / 2 * voxels / (gram * 1e-3)
    row = {"shape": shape, "points": list(points), "frames": K, "voxels": voxels,
           "gram": {"device_us": summary(ms["gram"]), "complex_products": K * (K + 1) // 2 * voxels, "complex_products_per_second": gram_rate}}
    for w in windows:
        T = int(np.prod([2 * s + 1 for s in w]))
        t = statistics.median(ms[w])
        rate = K * T * voxels / (t * 1e-3)
        row["window_%d_%d_%d" % w] = {"max_shift": list(w), "shifts": T, "device_us": summary(ms[w]), "complex_products": K * T * voxels,
                                      "complex_products_per_second": rate, "share_of_gram_rate": rate / gram_rate}
    rows.append(row)
    print(json.dumps(row), flush=True)

result = {"commit": args.commit, "repeats": args.repeats,
          "timing": "events around the launches of each call (device_ms), rounds gram, window, window, ... in turn after two warm-up rounds",
          "ring_bytes": int(os.environ["BEAMFORMER_HIP_FRAME_RING_BYTES"]),
          "rows": rows}
if args.json:
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1)
