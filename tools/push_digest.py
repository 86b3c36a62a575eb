"""What the push entry points produce, without a single time in it: for a fixed list of small cases (tests/cases.py) pushed as single
frames, as device-resident frames, as bursts and as views pushes, the SHA-256 of every exported frame with its id, and beside them the
bookkeeping a client can read back -- das_path, das_row_end_planes and the stage kinds of beamformer_hip_get_last_frame_timings, a
burst's route and stage kinds from beamformer_hip_get_last_burst_info, a views push's from beamformer_hip_get_last_views_info, das_pairs
where pair counting is on (of the newest frame's row: the C ABI reads no other row's), which of the two info calls is served after each
push of a mixed sequence, what a views push that fails leaves behind, the graphs instantiated where frame graphs are; and for the row-column DAS family every named case under every das path mode and staged-kernel hook of its parity tests.  The kernels are deterministic and the RF is seeded, so two builds of the library that enqueue the same work print the same
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
from tests.test_gpu_views import kernel_views, per_view_views, prepared
from tests.test_views_host import mixed_views

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

# ---- views pushes: one RF frame on K grids ----
PREFER, NO_KERNEL, FAIL_DAS = P.HIP_DAS_PATH_PREFER_VIEWS_KERNEL, P.HIP_DAS_PATH_NO_VIEWS_KERNEL, P.HIP_DAS_PATH_FAIL_VIEWS_DAS


def sha(frame):
    return hashlib.sha256(np.ascontiguousarray(frame).tobytes()).hexdigest()


def row(pairs=False):
    """the newest frame's row of the timing table"""
    t = P.HipFrameTimings()
    assert L.beamformer_hip_get_last_frame_timings(C.byref(t)), lib.last_error()
    out = {"das_path": int(t.das_path), "das_row_end_planes": int(t.das_row_end_planes), "das_voxels": int(t.das_voxels),
           "stage_kinds": [int(t.stage_kind[i]) for i in range(int(t.stage_count))],
           "staged_and_tile_counters": [int(t.staged_window_violations), int(t.tile_staged_chunks), int(t.tile_gather_chunks)]}
    if pairs:
        out["das_pairs"] = int(t.das_pairs)
    return out


def views_push(rf, views, on_device=False, pairs=False):
    """one views push: per view its id, digest and the path of its own decision; the push's route and stage kinds; the last view's row"""
    rf = np.ascontiguousarray(rf)
    array = (P.HipView * len(views))(*views)
    if on_device:
        dev = torch.from_numpy(rf.view(np.uint8).reshape(-1)).cuda()
        torch.cuda.synchronize()
        assert L.beamformer_hip_push_device_data_views_with_compute(C.c_void_p(dev.data_ptr()), rf.nbytes, array, len(views), 0), lib.last_error()
        assert L.beamformer_hip_synchronize()
    else:
        assert L.beamformer_hip_push_data_views_with_compute(rf.ctypes.data_as(C.c_void_p), rf.nbytes, array, len(views), 0), lib.last_error()
    frames = lib.get_last_views(views)
    info = lib.last_views_info()
    assert int(info.view_count) == len(views)
    return {"views": [{"id": int(info.first_frame_id) + k, "sha256": sha(frames[k]), "das_path": int(info.route.path[k])} for k in range(len(views))],
            "route": {"kernel_views": int(info.route.kernel_views), "das_launches": int(info.route.das_launches), "reason": info.route.reason.decode(),
                      "stage_kinds": [int(info.stage_kind[i]) for i in range(int(info.stage_count))]},
            "last_row": row(pairs)}


def served():
    """which of the two info calls the newest push serves, and the error of the one it refuses"""
    out = {}
    for name, fn, struct in (("burst_info", L.beamformer_hip_get_last_burst_info, P.HipBurstInfo), ("views_info", L.beamformer_hip_get_last_views_info, P.HipViewsInfo)):
        info = struct()
        out[name] = "served" if fn(C.byref(info)) else lib.last_error()[0].name
    return out


try:
    # the views kernel's view set under the automatic path, preferred and switched off, from host and from device-resident RF
    acq = cases.make("config1_small")
    rf = noise_frames(acq, 6, 700)
    views = kernel_views(acq)
    result["views_config1_small"] = {}
    for name, mode in (("auto", 0), ("prefer_kernel", PREFER), ("no_kernel", NO_KERNEL)):
        fresh(acq)
        L.beamformer_hip_set_das_path(mode)
        result["views_config1_small"][name] = {"host": views_push(rf[0], views), "device": views_push(rf[1], views, on_device=True)}

    # views the kernel takes and views it does not, in one push
    mixed = cases.make("rca_flash_none_tx")
    fresh(mixed)
    L.beamformer_hip_set_das_path(PREFER)
    result["views_mixed"] = views_push(noise_frames(mixed, 1, 710)[0], mixed_views(mixed))
    L.beamformer_hip_set_das_path(0)

    # every view its own single-frame launch(es): the staged counters and the hercules tables per view
    for k, name in enumerate(["rca_staged_auto", "hercules_wide_cw"]):
        other = cases.make(name)
        fresh(other)
        result["views_" + name] = views_push(noise_frames(other, 1, 720 + k)[0], per_view_views(other))

    # several parts per view: the plane, the rows around the depth at which the RF rows end, the strip past them
    ends, ends_rf, ends_views, _ = prepared("row_ends_linear")
    fresh(ends)
    L.beamformer_hip_set_das_path(PREFER)
    result["views_row_ends_linear"] = {"prefer_kernel": views_push(ends_rf, ends_views)}
    L.beamformer_hip_set_das_path(NO_KERNEL)
    result["views_row_ends_linear"]["no_kernel"] = views_push(ends_rf, ends_views)

    # pair counting runs per view: view k's count is the newest row's after a push that ends with view k
    fresh(acq)
    L.beamformer_hip_enable_pair_counting(1)
    counted = {}
    for name, mode in (("prefer_kernel", PREFER), ("no_kernel", NO_KERNEL)):
        L.beamformer_hip_set_das_path(mode)
        counted[name] = {"whole": views_push(rf[0], views, pairs=True),
                         "das_pairs_of_view": [views_push(rf[0], views[: k + 1], pairs=True)["last_row"]["das_pairs"] for k in range(len(views))]}
    result["views_config1_small_pair_counting"] = counted

    # more frames than timing slots on the per-frame route, pair counting on: counters and pair-count copies for the newest 32 only
    fresh(acq)
    L.beamformer_hip_set_das_path(P.HIP_DAS_PATH_NO_BURST_KERNEL)
    result["config1_small_pair_counting_burst40"] = burst(acq, noise_frames(acq, 40, 730), pairs=True)
    L.beamformer_hip_enable_pair_counting(0)

    # a views push that fails at its DAS stage (flag 0x2000), in both routes: failure, a tombstone under every id, the next single push
    three = views[:3]
    array = (P.HipView * 3)(*three)
    result["views_failed"] = {}
    for name, mode in (("prefer_kernel", PREFER), ("no_kernel", NO_KERNEL)):
        fresh(acq)
        L.beamformer_hip_set_das_path(mode)
        before = single(acq, rf[2])
        L.beamformer_hip_set_das_path(mode | FAIL_DAS)
        pushed = bool(L.beamformer_hip_push_data_views_with_compute(rf[3].ctypes.data_as(C.c_void_p), rf[3].nbytes, array, 3, 0))
        entry = {"before": before, "push": "served" if pushed else lib.last_error()[0].name, "info": served(), "last_frames": {}}
        sentinel = np.full(1 << 16, -7.0, np.float32)
        for count in (1, 2, 3):
            ok = bool(L.beamformer_get_last_frames(sentinel.ctypes.data_as(C.c_void_p), sentinel.nbytes, count))
            entry["last_frames"][str(count)] = {"served": ok, "error": lib.last_error()[0].name, "buffer_untouched": bool((sentinel == -7.0).all())}
        entry["frame_info_served"] = bool(L.beamformer_hip_get_last_frame_info(C.byref(P.HipFrameInfo())))
        entry["frame_timings_served"] = bool(L.beamformer_hip_get_last_frame_timings(C.byref(P.HipFrameTimings())))
        L.beamformer_hip_set_das_path(mode)
        entry["single_after"] = single(acq, rf[4])
        entry["views_after"] = views_push(rf[5], three)
        result["views_failed"][name] = entry

    # single -> views -> burst -> views -> single: which info call each push leaves served
    fresh(acq)
    L.beamformer_hip_set_das_path(0)
    sequence = []
    for step in ("single", "views", "burst", "views", "single"):
        if step == "single":
            entry = single(acq, rf[0])
        elif step == "views":
            entry = views_push(rf[1], three)
        else:
            entry = burst(acq, rf[:5])
        sequence.append({"push": step, "result": entry, "info": served()})
    result["single_views_burst_views_single"] = sequence
finally:
    L.beamformer_hip_enable_pair_counting(0)
    L.beamformer_hip_set_das_path(0)


# ---- the row-column DAS family (das_staged*.hip, das_separable.hip): every named case the gather or a staged kernel takes, under
# the das path modes and staged-kernel hooks of tests/test_gpu_parity.py -- the frame's digest and the path that produced it
from tests.test_gpu_parity import SEPARABLE, STAGED                      # noqa: E402

STAGED_SHAPES = ["5,4,5", "4,5,5", "6,4,5", "5,5,5", "4,6,5", "5,4,6", "4,5,6", "6,4,6", "5,5,6", "4,6,6"]
FAMILY_MODES = [("path0", 0, ()), ("path2", 2, ()), ("path3", 3, ()), ("path3_checked", 3, (("STAGED_CHECKED", "1"),)),
                ("path3_nouniform", 3, (("STAGED_NOUNIFORM", "1"),))] + \
               [("path3_shape_" + shape, 3, (("STAGED_SHAPE", shape),)) for shape in STAGED_SHAPES]
family = {}
L.beamformer_hip_shutdown()
assert L.beamformer_hip_set_devices((C.c_int32 * 1)(0), 1)
try:
    for name in sorted(STAGED | SEPARABLE):
        acq = cases.make(name)
        family[name] = {}
        for label, mode, hooks in FAMILY_MODES:
            for hook, value in hooks:
                lib.set_hook(hook, value)
            L.beamformer_hip_set_das_path(mode)
            try:
                frame = lib.beamform(acq.bp, acq.rf, acq.filters)
                t = P.HipFrameTimings()
                assert L.beamformer_hip_get_last_frame_timings(C.byref(t)), lib.last_error()
                family[name][label] = {"sha256": sha(frame), "das_path": int(t.das_path), "das_row_end_planes": int(t.das_row_end_planes),
                                       "staged_window_violations": int(t.staged_window_violations)}
            finally:
                for hook, _ in hooks:
                    lib.set_hook(hook, None)
finally:
    L.beamformer_hip_set_das_path(0)
result["rca_family"] = family

text = json.dumps(result, indent=1, sort_keys=True)
print(text)
if args.json:
    with open(args.json, "w") as f:
        f.write(text + "\n")
