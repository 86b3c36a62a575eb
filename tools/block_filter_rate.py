"""What the block-wise clutter filter costs on the device (beamformer_hip_gram_boxes_last_frames, beamformer_hip_mix_field_last_frames;
csrc/ensemble_blocks.hip), each beside the only way the library had before: a 512 x 1 x 512 complex ring, K = M = 64, a 15 x 1 x 15
lattice (first node at 32, step 32) and boxes of half 32 -- 225 boxes of 65 x 1 x 65 voxels (64 where the frame clips the last node's),
neighbours half overlapping.
  gram   gram_boxes of the 225 boxes in ONE call, against the same 225 boxes through beamformer_hip_gram_last_frames, a call and a
         synchronise a box; both by the host clock (each ends in a synchronise) and by the sum of their device times;
  mix    mix_field, against C x the device time of beamformer_hip_mix_last_frames for the same K and M on the same frames, C = 4 corners
         on a plane: the arithmetic the definition implies.  The plain kernel is the yardstick; its own run-to-run spread is recorded.
         Both shapes of the kernel are timed (hook BLEND_SHAPE): 0, the corner nodes outermost, and 1, each source loaded once for all
         corners; their outputs are compared byte for byte once.  Two more lattices take the field mix apart, each in both shapes:
         ONE NODE -- one cell, the whole frame, one corner: the plain mix's work in the blend kernels, full rows -- and ONE CELL OF 4
         CORNERS -- 2 x 1 x 2 nodes at 0 and 512, so the whole frame is one cell that blends along x and z: four corners without the
         short rows of small cells.
Rounds of gram_boxes, the 225 single calls, the plain mix, the field mix, in turn, --repeats of them after two warm-up rounds: median,
smallest and largest.  The frames are one frame of BASELINE config 1's RF on that grid and K scaled copies of it by a mix 1 -> K; every
node's weight table is a seeded unitary matrix, so the mixes keep the frames' energy round after round; no call's time depends on the
values.  On the first round the matrices of the one call are compared byte for byte with the single calls'.
Run from the repository root on a GPU box: PYTHONPATH=. python tools/block_filter_rate.py --json profiles/block_filter_rate.json [--commit ID]"""
import argparse
import ctypes as C
import json
import os
import statistics
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--json", default="")
ap.add_argument("--commit", default="")
args = ap.parse_args()

K = M = args.frames
POINTS, NODES, FIRST, STEP, HALF = (512, 1, 512), (15, 1, 15), (32, 0, 32), (32, 1, 32), (32, 0, 32)
frame_bytes = int(np.prod(POINTS)) * 8
os.environ.setdefault("BEAMFORMER_HIP_FRAME_RING_BYTES", str(8 * K * frame_bytes))      # (before the library loads)

from ogl_beamforming_amd import configs, lib, params as P  # noqa: E402

L = lib.library()
L.beamformer_set_global_timeout(0xFFFFFFFF)
acq = configs.config(1)
rf = np.ascontiguousarray(acq.rf)
for s, fp in enumerate(acq.filters):
    assert L.beamformer_create_filter(C.byref(fp), s, 0), lib.last_error()
m = list(acq.bp.das_voxel_transform)              # das_transform_2d_xz: x extent m[0] from m[12], depth extent m[6] from m[14]
bp = type(acq.bp).from_buffer_copy(acq.bp)
bp.das_voxel_transform[:] = [float(v) for v in configs.das_transform_3d((m[12], 0.0, m[14]), (m[12] + m[0], 0.0, m[14] + m[6]))]
bp.output_points[:3] = list(POINTS)
lib.beamform(bp, rf, acq.filters)
lib.mix_last_frames(1, (1.0 + 0.5 * np.arange(K) / K).astype(np.complex64)[:, None])

rng = np.random.default_rng(9100)
nodes = NODES[0] * NODES[1] * NODES[2]
W = np.stack([np.linalg.qr(rng.standard_normal((K, K)) + 1j * rng.standard_normal((K, K)))[0] for _ in range(nodes)]).astype(np.complex64)
W = W.reshape(NODES[2], NODES[1], NODES[0], M, K)
boxes = lib.lattice_boxes(POINTS, NODES, FIRST, STEP, HALF)
# (65 x 1 x 65 voxels but for the last node of an axis, at 480: its box is clipped at 512 and 64 wide)
assert len(boxes) == 225 and tuple(boxes[0].count) == (65, 1, 65) and tuple(boxes[-1].count) == (64, 1, 64)

# the cells of the field mix (csrc/frame_ops.cpp cuts the same): segments an axis, and how many corner nodes a voxel has on average
segments = []
for a in range(3):
    if NODES[a] == 1:
        segments.append([(POINTS[a], 1)])
        continue
    at = [min(POINTS[a], FIRST[a] + j * STEP[a]) for j in range(NODES[a])]
    axis = [(at[0], 1)] + [(at[j + 1] - at[j], 2) for j in range(NODES[a] - 1)] + [(POINTS[a] - at[-1], 1)]
    segments.append([s for s in axis if s[0] > 0])
cells = [(sx[0] * sy[0] * sz[0], sx[1] * sy[1] * sz[1]) for sz in segments[2] for sy in segments[1] for sx in segments[0]]
voxels = int(np.prod(POINTS))
mean_corners = sum(v * c for v, c in cells) / voxels


def summary(times):
    return {"median_us": statistics.median(times) * 1e3, "min_us": min(times) * 1e3, "max_us": max(times) * 1e3, "runs": len(times)}


SHAPES = ((0, "corners_outermost"), (1, "sources_once"))
LATTICES = {"mix_field": (W, FIRST, STEP), "one_node": (W[7:8, :, 7:8], (0, 0, 0), (1, 1, 1)),
            "one_cell_4_corners": (W[:2, :, :2], (0, 0, 0), (POINTS[0], 1, POINTS[2]))}
names = ("gram_boxes_wall", "gram_boxes_device", "gram_singles_wall", "gram_singles_device", "mix_plain_device") + \
    tuple(f"{lattice}_{shape}_device" for lattice in LATTICES for _, shape in SHAPES)
ms = {name: [] for name in names}
for n in range(2 + args.repeats):
    L.beamformer_hip_synchronize()
    t0 = time.perf_counter()
    G, infos, device = lib.gram_boxes_last_frames(K, boxes)
    ms["gram_boxes_wall"].append((time.perf_counter() - t0) * 1e3)
    ms["gram_boxes_device"].append(device)
    t0 = time.perf_counter()
    singles = [lib.gram_last_frames(K, b) for b in boxes]
    ms["gram_singles_wall"].append((time.perf_counter() - t0) * 1e3)
    ms["gram_singles_device"].append(sum(s[2] for s in singles))
    if n == 0:
        assert all(G[b].tobytes() == singles[b][0].tobytes() and bytes(infos[b]) == bytes(singles[b][1]) for b in range(len(boxes)))
        assert all(int(i.voxels) == int(np.prod(list(b.count))) and int(i.non_finite) == 0 for i, b in zip(infos, boxes))
        print("  the 225 matrices of the one call are the single calls', byte for byte", flush=True)
    ms["mix_plain_device"].append(lib.mix_last_frames(K, W[7, 0, 7])[1])
    # (each mix moves "the K newest": the three time the same work on different values; the shapes are compared on one ensemble below)
    for lattice, (weights, first, step) in LATTICES.items():
        for shape, name in SHAPES:
            lib.set_hook("BLEND_SHAPE", shape)
            ms[f"{lattice}_{name}_device"].append(lib.mix_field_last_frames(K, weights, first, step)[1])
    lib.set_hook("BLEND_SHAPE", None)
for v in ms.values():
    del v[:2]
L.beamformer_hip_synchronize()
newest = lib.get_last_frames(bp, 1)
assert np.isfinite(newest.view(np.float32)).all()
# the two shapes on one ensemble: a mix back to 8 frames, filtered under each shape
outputs = []
for shape in (0, 1):
    lib.beamform(bp, rf, acq.filters)
    lib.mix_last_frames(1, (1.0 + 0.5 * np.arange(8) / 8).astype(np.complex64)[:, None])
    lib.set_hook("BLEND_SHAPE", shape)
    lib.mix_field_last_frames(8, W[:, :, :, :8, :8], FIRST, STEP)
    outputs.append(lib.get_last_frames(bp, 8).copy())
lib.set_hook("BLEND_SHAPE", None)
assert outputs[0].tobytes() == outputs[1].tobytes() and np.isfinite(outputs[0].view(np.float32)).all()
print("  the two shapes of the field mix give the same bytes", flush=True)

med = {name: statistics.median(v) for name, v in ms.items()}
plain = ms["mix_plain_device"]
result = {"commit": args.commit, "repeats": args.repeats, "frames": K, "outputs": M, "points": list(POINTS), "nodes": list(NODES),
          "node_first": list(FIRST), "node_step": list(STEP), "half": list(HALF), "boxes": len(boxes), "box_points": [65, 1, 65], "box_voxels_in_all": int(sum(int(np.prod(list(b.count))) for b in boxes)),
          "cells": len(cells), "mean_corner_nodes_a_voxel": mean_corners,
          "timing": "rounds of gram_boxes, the single calls, the plain mix, the field mix, in turn after two warm-up rounds; wall: host clock "
                    "around calls that end in a synchronise; device: events around the launches of each call (device_ms)",
          "ring_bytes": int(os.environ["BEAMFORMER_HIP_FRAME_RING_BYTES"]),
          "times": {name: summary(v) for name, v in ms.items()},
          "gram": {"wall_ratio_boxes_over_singles": med["gram_boxes_wall"] / med["gram_singles_wall"],
                   "device_ratio_boxes_over_singles": med["gram_boxes_device"] / med["gram_singles_device"]},
          "mix": {"corners": 4, "plain_spread": (max(plain) - min(plain)) / med["mix_plain_device"],
                  "shapes": {shape: {"field_over_4_plain": med[f"mix_field_{shape}_device"] / (4 * med["mix_plain_device"]),
                                     "field_over_mean_corners_plain": med[f"mix_field_{shape}_device"] / (mean_corners * med["mix_plain_device"]),
                                     "one_node_over_plain": med[f"one_node_{shape}_device"] / med["mix_plain_device"],
                                     "one_cell_4_corners_over_4_plain": med[f"one_cell_4_corners_{shape}_device"] / (4 * med["mix_plain_device"])}
                             for _, shape in SHAPES}}}
print(json.dumps(result), flush=True)
if args.json:
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1)
