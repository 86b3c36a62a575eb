"""What the push entry points produce, without a single time in it: for a fixed list of small cases (tests/cases.py) pushed as single
frames, as device-resident frames, as bursts, as views pushes and -- on every route each has -- as READI sweeps, READI images, burst
views pushes and variants pushes, the SHA-256 of every exported frame with its id, and beside them the
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
from tests.das_push import kernel_views, mixed_views, noise_frames, per_view_views, prepared, row_end_case

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


# ---- the other multi-frame pushes: a READI sweep, a READI image, a burst views push, a variants push -- each on every route it has,
# from host and from device-resident RF, with pair counting on and under the SCRATCH_POISON hook
from tests import readi_image_cases as R                                  # noqa: E402
from tests import variants_cases as vc                                    # noqa: E402
from tests.das_push import GROUPS5, four_views, groups_for, sweep_case    # noqa: E402

NO_BURST = P.HIP_DAS_PATH_NO_BURST_KERNEL


def compact(value):
    """the same record with every leaf collection on one line: a dict or list of plain values becomes one string (k=v pairs by key, or
    the values in order), bottom-up -- a frame is "id=... sha256=...", a route one line; a list of records stays a list.  The sections
    below record some hundred pushes: written out a value a line they would be most of the file."""
    plain = lambda x: x is None or isinstance(x, (str, int, float, bool))
    if isinstance(value, dict):
        inner = {k: compact(v) for k, v in value.items()}
        return " ".join(f"{k}={inner[k]}" for k in sorted(inner)) if all(plain(v) for v in inner.values()) else inner
    if isinstance(value, list):
        return " ".join(str(v) for v in value) if all(plain(v) for v in value) else [compact(v) for v in value]
    return value


def route_of(route, names, counted=()):
    """the named fields of an info call's route; `counted`: (array field, entries) pairs"""
    out = {name: int(getattr(route, name)) for name in names}
    out.update({name: [int(v) for v in getattr(route, name)[:n]] for name, n in counted})
    out["reason"] = route.reason.decode()
    return out


def pushed(frames, first_id, info, route, pairs):
    """what every push records: its frames' ids and digests, its route and stage kinds as its info call reports them, the newest row"""
    return {"frames": [{"id": int(first_id) + k, "sha256": sha(f)} for k, f in enumerate(frames)], "route": route,
            "stage_kinds": [int(info.stage_kind[i]) for i in range(int(info.stage_count))], "last_row": row(pairs)}


def on_device(rf):
    """(the tensor that keeps the copy alive, its pointer)"""
    dev = torch.from_numpy(np.ascontiguousarray(rf).view(np.uint8).reshape(-1)).cuda()
    torch.cuda.synchronize()
    return dev, dev.data_ptr()


def sweep_push(acq, rf, groups, device=False, pairs=False):
    dev, pointer = on_device(rf) if device else (None, None)
    frames = lib.beamform_readi_sweep(acq.bp, rf, groups, acq.filters, on_device_pointer=pointer)
    info = lib.last_burst_info()
    assert int(info.frame_count) == len(rf)
    return pushed(frames, info.first_frame_id, info, route_of(info.route, ["burst_kernel", "single_path", "frames_per_thread", "das_launches", "stage_launches", "min_frames"]), pairs)


def image_push(acq, rf, groups, device=False, pairs=False):
    dev, pointer = on_device(rf) if device else (None, None)
    frame = lib.beamform_readi_image(acq.bp, rf, groups, acq.filters, on_device_pointer=pointer)
    info = lib.last_readi_image_info()
    assert int(info.rf_frame_count) == len(rf)
    return pushed([frame], info.frame_id, info, route_of(info.route, ["transmit_count", "das_path", "das_launches", "stage_launches", "decode_launches"]), pairs)


def burst_views_push(acq, rf, views, device=False, pairs=False):
    dev, pointer = on_device(rf) if device else (None, None)
    frames = lib.beamform_burst_views(acq.bp, rf, views, acq.filters, on_device_pointer=pointer)
    info = lib.last_burst_views_info()
    assert (int(info.frame_count), int(info.view_count)) == (len(rf), len(views))
    route = route_of(info.route, ["rung", "kernel_views", "frame_kernel_views", "das_launches", "stage_launches", "frames_per_thread", "min_frames"], [("path", len(views))])
    return pushed([f for view in frames for f in view], info.first_frame_id, info, route, pairs)


def variants_push(acq, rf, variants, device=False, pairs=False):
    dev, pointer = on_device(rf) if device else (None, None)
    frames = lib.beamform_variants(acq.bp, rf, variants, acq.filters, on_device_pointer=pointer)
    info = lib.last_variants_info()
    K = len(variants)
    assert int(info.variant_count) == K
    route = route_of(info.route, ["kernel_variants", "fused_launches", "das_launches", "kernel_tiles", "min_tiles", "min_variants"], [("taken", K), ("path", K)])
    return pushed(list(frames), info.first_frame_id, info, route, pairs)


def every_way(acq, mode, push):
    """push(device=, pairs=) on a fresh library under das path `mode`: from host, from device-resident RF, with pair counting on and
    under SCRATCH_POISON"""
    fresh(acq)
    L.beamformer_hip_set_das_path(mode)
    out = {"host": push(), "device": push(device=True)}
    L.beamformer_hip_enable_pair_counting(1)
    try:
        out["pair_counting"] = push(pairs=True)
    finally:
        L.beamformer_hip_enable_pair_counting(0)
    lib.set_hook("SCRATCH_POISON", "1")
    try:
        out["scratch_poison"] = push()
    finally:
        lib.set_hook("SCRATCH_POISON", None)
        L.beamformer_hip_set_das_path(0)
    return out


def served_all():
    """which of the five info calls the newest push serves, and the error of those it refuses"""
    out = {}
    for name, fn, struct in (("burst_info", L.beamformer_hip_get_last_burst_info, P.HipBurstInfo), ("views_info", L.beamformer_hip_get_last_views_info, P.HipViewsInfo),
                             ("readi_image_info", L.beamformer_hip_get_last_readi_image_info, P.HipReadiImageInfo),
                             ("burst_views_info", L.beamformer_hip_get_last_burst_views_info, P.HipBurstViewsInfo),
                             ("variants_info", L.beamformer_hip_get_last_variants_info, P.HipVariantsInfo)):
        info = struct()
        out[name] = "served" if fn(C.byref(info)) else lib.last_error()[0].name
    return out


try:
    # a READI sweep: on its kernel (5 frames and more), on the per-frame route (flag 0x400), and of one frame
    sweep_acq = sweep_case("g4a4", P.InterpolationMode.Linear, True, False)
    sweep_rf = noise_frames(sweep_acq, 5, 800)
    groups5 = groups_for(sweep_acq, GROUPS5)
    result["readi_sweep"] = {"kernel": every_way(sweep_acq, 0, lambda **how: sweep_push(sweep_acq, sweep_rf, groups5, **how)),
                             "per_frame": every_way(sweep_acq, NO_BURST, lambda **how: sweep_push(sweep_acq, sweep_rf, groups5, **how)),
                             "one_frame": every_way(sweep_acq, 0, lambda **how: sweep_push(sweep_acq, sweep_rf[:1], groups5[:1], **how))}

    # a READI image: every group once (a permutation), and one RF frame
    image_acq = R.image_case("g4a4", P.InterpolationMode.Linear, "iq")
    image_rf = noise_frames(image_acq, 4, 810)
    permutation = R.PERMUTATIONS["g4a4"]
    result["readi_image"] = {"four_frames": every_way(image_acq, 0, lambda **how: image_push(image_acq, image_rf, permutation, **how)),
                             "one_frame": every_way(image_acq, 0, lambda **how: image_push(image_acq, image_rf[:1], permutation[:1], **how))}

    # a burst views push: the ladder's three rungs (automatic at 5 RF frames, 0x400, 0x800) and one RF frame
    bv_acq = cases.make("config1_small")
    bv_rf = noise_frames(bv_acq, 5, 820)
    bv_views = four_views(bv_acq)
    result["burst_views"] = {name: every_way(bv_acq, mode, lambda **how: burst_views_push(bv_acq, bv_rf, bv_views, **how))
                             for name, mode in (("rung1", 0), ("rung2_0x400", NO_BURST), ("rung3_0x800", NO_KERNEL))}
    result["burst_views"]["one_frame"] = every_way(bv_acq, 0, lambda **how: burst_views_push(bv_acq, bv_rf[:1], bv_views, **how))

    # a variants push: every variant fused (flag 0x8000, and eight candidates on the automatic route), none fused (flag 0x4000, and
    # three candidates below both thresholds), and a block whose variants run different single-frame kernels, each its own launch(es).
    # (No block of the test suites gives a route with some variants fused and others not: beamformer_hip_describe_variants, scanned.)
    v_acq = vc.block("linear", True, True)
    three_variants = vc.candidates(v_acq.bp)
    eight_variants = three_variants + [lib.variant_of(v_acq.bp, speed_of_sound=1400.0 + 40.0 * k) for k in range(5)]
    result["variants"] = {name: every_way(v_acq, mode, lambda **how: variants_push(v_acq, v_acq.rf, chosen, **how))
                          for name, mode, chosen in (("prefer_kernel", vc.PREFER, three_variants), ("no_kernel", vc.NO_KERNEL, three_variants),
                                                     ("automatic_eight", 0, eight_variants), ("automatic_three", 0, three_variants))}
    staged_acq = cases.make("rca_staged_auto")
    staged_variants = vc.candidates(staged_acq.bp) + [lib.variant_of(staged_acq.bp, speed_of_sound=3000.0)]
    result["variants"]["own_kernels"] = every_way(staged_acq, 0, lambda **how: variants_push(staged_acq, staged_acq.rf, staged_variants, **how))

    # a variants push that fails at its DAS stage (flag 0x2000), in both routes: failure, a tombstone under every id, the next pushes
    array = (P.HipDasVariant * 3)(*three_variants)
    v_rf = np.ascontiguousarray(v_acq.rf)
    result["variants_failed"] = {}
    for name, mode in (("prefer_kernel", vc.PREFER), ("no_kernel", vc.NO_KERNEL)):
        fresh(v_acq)
        L.beamformer_hip_set_das_path(mode)
        before = single(v_acq, v_rf)
        L.beamformer_hip_set_das_path(mode | FAIL_DAS)
        ok = bool(L.beamformer_hip_push_data_variants_with_compute(v_rf.ctypes.data_as(C.c_void_p), v_rf.nbytes, array, 3, 0, 0))
        entry = {"before": before, "push": "served" if ok else lib.last_error()[0].name, "info": served_all(), "last_frames": {}}
        sentinel = np.full(1 << 16, -7.0, np.float32)
        for count in (1, 2, 3):
            ok = bool(L.beamformer_get_last_frames(sentinel.ctypes.data_as(C.c_void_p), sentinel.nbytes, count))
            entry["last_frames"][str(count)] = {"served": ok, "error": lib.last_error()[0].name, "buffer_untouched": bool((sentinel == -7.0).all())}
        entry["frame_info_served"] = bool(L.beamformer_hip_get_last_frame_info(C.byref(P.HipFrameInfo())))
        entry["frame_timings_served"] = bool(L.beamformer_hip_get_last_frame_timings(C.byref(P.HipFrameTimings())))
        L.beamformer_hip_set_das_path(mode)
        entry["single_after"] = single(v_acq, v_rf)
        entry["variants_after"] = variants_push(v_acq, v_rf, three_variants)
        result["variants_failed"][name] = entry

    # one sequence over all push kinds: which of the five info calls each push leaves served
    L.beamformer_hip_set_das_path(0)
    steps = [("single", lambda: (fresh(bv_acq), single(bv_acq, bv_rf[0]))[1]), ("views", lambda: views_push(bv_rf[1], bv_views[:3])),
             ("burst", lambda: burst(bv_acq, bv_rf)), ("burst_views", lambda: burst_views_push(bv_acq, bv_rf, bv_views)),
             ("variants", lambda: variants_push(v_acq, v_acq.rf, eight_variants)), ("readi_sweep", lambda: sweep_push(sweep_acq, sweep_rf, groups5)),
             ("readi_image", lambda: image_push(image_acq, image_rf, permutation)), ("single", lambda: single(image_acq, image_rf[0])),
             ("variants", lambda: variants_push(v_acq, v_acq.rf, three_variants)), ("views", lambda: (fresh(bv_acq), views_push(bv_rf[1], bv_views[:3]))[1])]
    result["all_push_kinds"] = [{"push": name, "result": step(), "info": served_all()} for name, step in steps]
finally:
    L.beamformer_hip_enable_pair_counting(0)
    lib.set_hook("SCRATCH_POISON", None)
    L.beamformer_hip_set_das_path(0)
for section in ("readi_sweep", "readi_image", "burst_views", "variants", "variants_failed", "all_push_kinds"):
    result[section] = compact(result[section])


# ---- the row-column DAS family (das_staged*.hip, das_separable.hip): every named case the gather or a staged kernel takes, under
# the das path modes and staged-kernel hooks of tests/test_gpu_parity.py -- the frame's digest and the path that produced it
from tests.das_kernel_cases import SEPARABLE, STAGED                    # noqa: E402

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
