"""What the push entry points produce, without a single time in it: for a fixed list of small cases (tests/cases.py) pushed as single
frames, as device-resident frames and as bursts, the SHA-256 of every exported frame with its id, and beside them the bookkeeping a
client can read back -- das_path, das_row_end_planes and the stage kinds of beamformer_hip_get_last_frame_timings, a burst's route and
stage kinds from beamformer_hip_get_last_burst_info, das_pairs where pair counting is on, the graphs instantiated where frame graphs
are.  The kernels are deterministic and the RF is seeded, so two builds of the library that enqueue the same work print the same
object: run it on both (OGL_BEAMFORMER_LIB selects the library, tools/build_variant.sh builds the other one) and compare.
Run from the repository root on a GPU box:  PYTHONPATH=. python tools/push_digest.py --json profiles/push_digest.json"""
import argparse
import ctypes as C
import hashlib
import json

import numpy as np
import torch

from ogl_beamforming_amd import lib, params as P
from tests import cases
from tests.test_gpu_burst import noise_frames, row_end_case

ap = argparse.ArgumentParser()
ap.add_argument("--json", default="")
args = ap.parse_args()

torch.cuda.set_device(0)
L = lib.library()
L.beamformer_set_global_timeout(0xFFFFFFFF)
OVERLAP_BYTES = 8 << 20           # csrc/executor.cpp kOverlapBytes: host uploads from this size on go over the copy engine


def fresh(acq, devices=(0,)):
    """a library that has seen nothing: ids start at 0, no plan, no timing sample"""
    L.beamformer_hip_shutdown()
    assert L.beamformer_hip_set_devices((C.c_int32 * len(devices))(*devices), len(devices)), lib.last_error()
    for slot, fp in enumerate(acq.filters):
        assert L.beamformer_create_filter(C.byref(fp), slot, 0), lib.last_error()
    assert L.beamformer_push_simple_parameters(C.byref(acq.bp)), lib.last_error()


def newest(acq, count, pairs=False):
    """the `count` newest frames and the newest frame's row of the timing table"""
    info, t = P.HipFrameInfo(), P.HipFrameTimings()
    frames = lib.get_last_frames(acq.bp, count)
    assert L.beamformer_hip_get_last_frame_info(C.byref(info)), lib.last_error()
    assert L.beamformer_hip_get_last_frame_timings(C.byref(t)), lib.last_error()
    out = {"frames": [{"id": int(info.frame_id) - (count - 1 - k), "sha256": hashlib.sha256(frames[k].tobytes()).hexdigest()} for k in range(count)],
           "das_path": int(t.das_path), "das_row_end_planes": int(t.das_row_end_planes),
           "stage_kinds": [int(t.stage_kind[i]) for i in range(int(t.stage_count))],
           "staged_and_tile_counters": [int(t.staged_window_violations), int(t.tile_staged_chunks), int(t.tile_gather_chunks)]}
    if pairs:
        out["das_pairs"] = int(t.das_pairs)
    return out


def single(acq, rf, on_device=False, pairs=False):
    rf = np.ascontiguousarray(rf)
    if on_device:
        dev = torch.from_numpy(rf.view(np.uint8).reshape(-1)).cuda()
        torch.cuda.synchronize()
        assert L.beamformer_hip_push_device_data_with_compute(C.c_void_p(dev.data_ptr()), rf.nbytes, 0, 0), lib.last_error()
        assert L.beamformer_hip_synchronize()
    else:
        assert L.beamformer_push_data_with_compute(rf.ctypes.data_as(C.c_void_p), rf.nbytes, 0, 0), lib.last_error()
    return newest(acq, 1, pairs)


def burst(acq, rf, on_device=False, pairs=False):
    n, size = rf.shape[0], rf[0].nbytes
    if on_device:
        dev = torch.from_numpy(rf.view(np.uint8).reshape(-1)).cuda()
        torch.cuda.synchronize()
        assert L.beamformer_hip_push_device_data_burst_with_compute(C.c_void_p(dev.data_ptr()), size, n, 0, 0), lib.last_error()
        assert L.beamformer_hip_synchronize()
    else:
        assert L.beamformer_hip_push_data_burst_with_compute(rf.ctypes.data_as(C.c_void_p), size, n, 0, 0), lib.last_error()
    out = newest(acq, n, pairs)
    info = lib.last_burst_info()
    assert out["frames"][0]["id"] == int(info.first_frame_id) and int(info.frame_count) == n
    out["burst"] = {"burst_kernel": int(info.route.burst_kernel), "single_path": int(info.route.single_path),
                    "frames_per_thread": int(info.route.frames_per_thread), "das_launches": int(info.route.das_launches),
                    "stage_launches": int(info.route.stage_launches), "reason": info.route.reason.decode(),
                    "stage_kinds": [int(info.stage_kind[i]) for i in range(int(info.stage_count))]}
    return out


def single_and_burst5(acq, seed, pairs=False):
    fresh(acq)
    rf = noise_frames(acq, 5, seed)
    return {"single": single(acq, rf[0], pairs=pairs), "burst5": burst(acq, rf, pairs=pairs)}


def graph_counts():
    replayed, built = C.c_uint64(), C.c_uint64()
    L.beamformer_hip_frame_graph_counts(C.byref(replayed), C.byref(built))
    return replayed.value, built.value


result = {}

# the general kernel, zero-copy upload: every way in
acq = cases.make("config1_small")
fresh(acq)
rf = noise_frames(acq, 9, 100)
result["config1_small"] = {"single": single(acq, rf[0]), "single_device": single(acq, rf[1], on_device=True),
                           "burst2": burst(acq, rf[:2]), "burst5": burst(acq, rf[:5]), "burst9": burst(acq, rf),
                           "burst5_device": burst(acq, rf[:5], on_device=True)}
# the ingest kernel with work to do (A1S2, a shuffled and padded mapping); the per-frame route of a burst with the staged counters and
# the hercules tables
for k, name in enumerate(["rca_a1s2", "rca_shuffled_padded", "rca_staged_auto", "forces", "hercules_wide_cw"]):
    result[name] = single_and_burst5(cases.make(name), 200 + k)
# several parts per frame
acq = row_end_case(P.InterpolationMode.Linear)
result[acq.name] = single_and_burst5(acq, 300)

# frame graphs: the plan's first frame runs uncaptured, the second instantiates the graph, the third updates it in place
acq = cases.make("config4_small")
fresh(acq)
rf = noise_frames(acq, 3, 400)
replayed0, built0 = graph_counts()
L.beamformer_hip_enable_frame_graphs(1)
try:
    pushes = [single(acq, rf[k]) for k in range(3)]
finally:
    L.beamformer_hip_enable_frame_graphs(0)
replayed, built = graph_counts()
result["config4_small_frame_graphs"] = {"pushes": pushes, "graph_frames": replayed - replayed0, "graph_instantiations": built - built0}

# two device contexts on one ordinal: every frame is two z-slabs, stitched by the export
fresh(acq, devices=(0, 0))
result["config4_small_two_contexts"] = {"pushes": [single(acq, rf[k]) for k in range(2)]}
L.beamformer_hip_shutdown()
assert L.beamformer_hip_set_devices((C.c_int32 * 1)(0), 1)

# pair counting
L.beamformer_hip_enable_pair_counting(1)
try:
    result["config1_small_pair_counting"] = single_and_burst5(cases.make("config1_small"), 500, pairs=True)
finally:
    L.beamformer_hip_enable_pair_counting(0)

# the copy-engine upload: rows padded until one frame is kOverlapBytes of host memory
acq = cases.make("rca_shuffled_padded")
assert acq.bp.data_kind == int(P.DataKind.Int16) and acq.rf.dtype == np.int16
rows = int(acq.bp.raw_data_dimensions[1])
row = -(-OVERLAP_BYTES // (rows * acq.rf.itemsize))
acq.bp.raw_data_dimensions[0] = row
padded = np.zeros((rows, row), acq.rf.dtype)
padded[:, : acq.rf.shape[1]] = noise_frames(acq, 1, 600)[0]
assert padded.nbytes >= OVERLAP_BYTES > padded.nbytes - rows * acq.rf.itemsize
fresh(acq)
result["rca_shuffled_padded_8MiB"] = {"single": single(acq, padded), "rf_bytes": padded.nbytes}

text = json.dumps(result, indent=1, sort_keys=True)
print(text)
if args.json:
    with open(args.json, "w") as f:
        f.write(text + "\n")
