"""What the warp on the device costs (beamformer_hip_warp_last_frames; csrc/warp.hip): on the 512 x 1 x 1024 complex view plane and on
a 256 x 256 x 256 complex volume, K = 1 and K = 64 frames -- one frame of BASELINE config 1's RF (ogl_beamforming_amd/configs.py: 64
channels, one transmit) and K scaled copies of it by a mix 1 -> K --, in one process, in turn,
  (floor)    beamformer_hip_mix_last_frames K -> K with identity weights, asked for its device_ms: every frame read once and
             written once, the streaming floor DESIGN 3.7e uses;
  (convolve) one pass of beamformer_hip_convolve_last_frames, 9 taps along x;
  (rigid)    a sub-voxel shift per frame, Linear and Cubic;
  (lattice)  a field of +- 2 voxels on 9 x 1 x 9 nodes (plane) / 5 x 5 x 5 nodes (volume) that span the frame, Linear and Cubic;
  (direct)   the same four calls with every tile down the direct path (das path flag WarpDirect);
  (wild)     the automatic fallback: a field on 16 x 1 x 32 / 8 x 8 x 8 nodes, within +- 1 voxel over the low half of x and alternating
             between +- 128 voxels from node to node over the high half, Linear and Cubic, no flag: the tiles of the high half find
             their source boxes over the LDS budget and take the direct path by themselves, the others are staged, in one launch;
             the share of direct tiles is worked out from the field (tests/warp_ref.py: tile_boxes) and recorded;
Clamp edge everywhere (a step warps the outputs of the step before it: the values stay in range), timed floor, convolve, rigid, ...
for --repeats rounds after two warm-up rounds: median, smallest and largest of each device_ms.  The ring holds three runs.
The device's frames are checked against the reference's bound once, on the plane at K = 1 (the numpy reference gathers tap by tap:
the volume's 2^24 voxels under 64 taps are left to the suite's small grids).
Rates: bytes = K frames read and written once, over the median device_ms, beside the measured copy rate of the MI355X; taps per
second = K x voxels x taps of the support.
Run from the repository root on a GPU box: PYTHONPATH=. python tools/warp_rate.py --json profiles/warp_rate.json [--commit ID]"""
import argparse
import ctypes as C
import json
import os
import statistics

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
from tests import spatial_ref, warp_ref as ref  # noqa: E402

COPY_RATE_MEASURED, HBM_PEAK_SPEC, F32_PEAK = 6.29e12, 8.0e12, 157.3e12
LINEAR, CUBIC, CLAMP = int(P.HipWarpInterpolation.Linear), int(P.HipWarpInterpolation.Cubic), int(P.HipWarpEdge.Clamp)
L = lib.library()
L.beamformer_set_global_timeout(0xFFFFFFFF)
acq = configs.config(1)
rf = np.ascontiguousarray(acq.rf)
for s, fp in enumerate(acq.filters):
    assert L.beamformer_create_filter(C.byref(fp), s, 0), lib.last_error()
m = list(acq.bp.das_voxel_transform)              # das_transform_2d_xz: x extent m[0] from m[12], depth extent m[6] from m[14]
x0, x1, z0, z1 = m[12], m[12] + m[0], m[14], m[14] + m[6]
BOXES = {"plane": ((x0, 0.0, z0), (x1, 0.0, z1)), "volume": ((x0, -2e-3, z0), (x1, 2e-3, z1))}
G9 = spatial_ref.gaussian(9, 1.5)


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
    nodes = (9, 1, 9) if shape == "plane" else (5, 5, 5)
    lattice = dict(nodes=nodes, node_first=(0, 0, 0), node_step=tuple(max(1.0, (points[a] - 1) / max(1, nodes[a] - 1)) for a in range(3)))
    rng = np.random.default_rng(9990)
    for K in counts_of[shape]:
        lib.beamform(bp, rf, acq.filters)
        if K > 1:
            lib.mix_last_frames(1, (1.0 + 0.5 * np.arange(K) / K).astype(np.complex64)[:, None])
        eye = np.eye(K, dtype=np.complex64)
        row = {"shape": shape, "points": list(points), "frames": K, "frame_bytes": frame_bytes, "nodes": list(nodes)}
        shifts = (rng.integers(-7, 8, (K, 3)) / 8.0).astype(np.float32)
        field = rng.uniform(-2.0, 2.0, (K, nodes[2], nodes[1], nodes[0], 3)).astype(np.float32)
        wild_nodes = (16, 1, 32) if shape == "plane" else (8, 8, 8)
        wild_lattice = dict(nodes=wild_nodes, node_first=(0, 0, 0), node_step=tuple(max(1.0, (points[a] - 1) / max(1, wild_nodes[a] - 1)) for a in range(3)))
        iz, iy, ix = np.meshgrid(np.arange(wild_nodes[2]), np.arange(wild_nodes[1]), np.arange(wild_nodes[0]), indexing="ij")
        wild = np.where((ix + iy + iz) % 2 == 0, 128.0, -128.0)[None, ..., None] + rng.uniform(-2.0, 2.0, (K, wild_nodes[2], wild_nodes[1], wild_nodes[0], 3))
        wild[:, :, :, :wild_nodes[0] // 2, :] = rng.uniform(-1.0, 1.0, (K, wild_nodes[2], wild_nodes[1], wild_nodes[0] // 2, 3))
        wild = wild.astype(np.float32)
        steps = {}
        for path, flag in (("", 0), ("_direct", P.HIP_DAS_PATH_WARP_DIRECT)):
            for name, interpolation in (("linear", LINEAR), ("cubic", CUBIC)):
                steps["rigid_" + name + path] = (dict(displacements=shifts, interpolation=interpolation, edge=CLAMP), flag)
                steps["lattice_" + name + path] = (dict(displacements=field, interpolation=interpolation, edge=CLAMP, **lattice), flag)

        for name, interpolation in (("linear", LINEAR), ("cubic", CUBIC)):
            steps["wild_" + name] = (dict(displacements=wild, interpolation=interpolation, edge=CLAMP, **wild_lattice), 0)
            if K == 1:                             # (frame 0 of the field; the pattern is the same at every K)
                boxes = ref.tile_boxes((points[2], points[1], points[0]), wild[0], interpolation=interpolation, **wild_lattice)
                row["wild_" + name + "_direct_tile_share"] = float((boxes > ref.BOX_VOXELS).mean())
                row["wild_" + name + "_tiles_within_a_fifth_of_the_budget"] = int(((boxes > 0.8 * ref.BOX_VOXELS) & (boxes < 1.2 * ref.BOX_VOXELS)).sum())

        if K == 1 and shape == "plane":
            info = P.HipFrameInfo()
            assert L.beamformer_hip_get_last_frame_info(C.byref(info))
            source = lib.copy_frame(int(info.frame_id)).copy()
            worst = {}
            for name in ("lattice_linear", "lattice_cubic", "lattice_cubic_direct", "wild_cubic"):
                k, flag = steps[name]
                L.beamformer_hip_set_das_path(flag)
                first, _ = lib.warp_last_frames(1, **k)
                L.beamformer_hip_set_das_path(0)
                device = lib.copy_frame(first)
                values, bound = ref.warp(source, k["displacements"][0], k["nodes"], k["node_first"], k["node_step"], interpolation=k["interpolation"], edge=ref.CLAMP)
                worst[name], inside = ref.share_of_bound(device, values, bound)
                assert inside, (name, worst)
                lib.mix_last_frames(2, np.array([[1, 0]], np.complex64))          # the source is the newest frame again
            row["device_against_reference_share_of_bound"] = worst
            del source, values, bound, device

        ms = {"floor": [], "convolve_x": []}
        ms.update({name: [] for name in steps})
        for n in range(2 + args.repeats):
            _, t = lib.mix_last_frames(K, eye)
            ms["floor"].append(t)
            _, t = lib.convolve_last_frames(K, [G9, None, None])
            ms["convolve_x"].append(t)
            for name, (k, flag) in steps.items():
                L.beamformer_hip_set_das_path(flag)
                _, t = lib.warp_last_frames(K, **k)
                L.beamformer_hip_set_das_path(0)
                ms[name].append(t)
        for v in ms.values():
            del v[:2]
        floor = statistics.median(ms["floor"])
        row["floor_mix_identity_device_us"] = summary(ms["floor"])
        row["floor_bytes_per_second"] = 2 * K * frame_bytes / (floor * 1e-3)
        row["floor_share_of_copy_rate"] = row["floor_bytes_per_second"] / COPY_RATE_MEASURED
        row["convolve_x_9_taps_device_us"] = summary(ms["convolve_x"])
        row["convolve_x_multiple_of_floor"] = statistics.median(ms["convolve_x"]) / floor
        for name, (k, flag) in steps.items():
            t = statistics.median(ms[name])
            taps = (4 if k["interpolation"] == CUBIC else 2) ** len(live)
            row[name] = {"taps": taps, "direct": bool(flag), "device_us": summary(ms[name]), "multiple_of_floor": t / floor,
                         "multiple_of_convolve_pass": t / statistics.median(ms["convolve_x"]),
                         "bytes_per_second": 2 * K * frame_bytes / (t * 1e-3), "share_of_copy_rate": 2 * K * frame_bytes / (t * 1e-3) / COPY_RATE_MEASURED,
                         "taps_per_second": taps * K * voxels / (t * 1e-3)}
        for name in [n for n in steps if not n.endswith("_direct") and not n.startswith("wild_")]:
            row[name]["staged_over_direct"] = statistics.median(ms[name]) / statistics.median(ms[name + "_direct"])
        rows.append(row)
        print(json.dumps(row), flush=True)

result = {"commit": args.commit, "repeats": args.repeats,
          "timing": "device: events around the launch of each call (device_ms), rounds floor, convolve_x, the ten warps in turn after two warm-up "
                    "rounds, every step on the K newest frames",
          "peaks": {"copy_rate_measured_float4": COPY_RATE_MEASURED, "hbm_specified": HBM_PEAK_SPEC, "f32_flop_per_second": F32_PEAK},
          "ring_bytes": int(os.environ["BEAMFORMER_HIP_FRAME_RING_BYTES"]),
          "rows": rows}
if args.json:
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1)
