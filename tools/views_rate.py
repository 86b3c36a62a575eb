"""What a views push buys (beamformer_hip_push_data_views_with_compute): wall time per push, fence to fence with the upload, of ONE RF
frame beamformed on K grids (a) by one views push through the views kernel (csrc/das_views.hip; das path flag 0x1000, so that it
runs however few the tiles), (b) by one views push down the per-view route (flag 0x800: every view its single-frame launch on the
shared DAS input), (c) as a user of the parent commit does it: K x (push the parameter block with the view's grid + a single push of
the RF).  The three are timed in turn, --repeats rounds after two warm-up rounds; the figures are medians, and (b)'s run-to-run spread
(largest - smallest of its timed runs) is kept beside them.  Also the host microseconds the push spends in decide_views
(BeamformerHipViewsInfo::decide_us).  Acquisition: BASELINE config 1 at full size (64 channels, one plane wave); views: K patches of
16 x 1 x 16 and of 32 x 1 x 32 voxels inside its image, and the two planes of an X-plane of its own grid size.

csrc/das_select.h's kViewsMinTiles is the smallest tile count of this table at which (a) is not slower than (b) by more than three
times (b)'s spread ("min_tiles_from_this_table").  Run from the repository root on a GPU box:
PYTHONPATH=. python tools/views_rate.py --json profiles/views_rate.json [--commit ID]"""
import argparse
import ctypes as C
import json
import statistics
import time

import numpy as np

from ogl_beamforming_amd import configs, lib, params as P

ap = argparse.ArgumentParser()
ap.add_argument("--views", default="1,2,4,16,64,256")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--json", default="")
ap.add_argument("--commit", default="")
args = ap.parse_args()

L = lib.library()
L.beamformer_set_global_timeout(0xFFFFFFFF)
acq = configs.config(1)
for s, fp in enumerate(acq.filters):
    assert L.beamformer_create_filter(C.byref(fp), s, 0)
rf = np.ascontiguousarray(np.clip(np.rint(np.random.default_rng(3).normal(0, 1000.0, acq.rf.shape)), -32000, 32000).astype(acq.rf.dtype))
ptr, size = rf.ctypes.data_as(C.c_void_p), rf.nbytes

m = list(acq.bp.das_voxel_transform)              # das_transform_2d_xz: x extent m[0] from m[12], depth extent m[6] from m[14]
x0, x1, z0, z1 = m[12], m[12] + m[0], m[14], m[14] + m[6]
own = [int(n) for n in acq.bp.output_points[:3]]
pitch_x, pitch_z = (x1 - x0) / (own[0] - 1), (z1 - z0) / (own[1] - 1)


def patch_views(k, n):
    """k patches of n x 1 x n voxels at a quarter of the image's voxel pitch (the fine grid of a refinement), spread over the image"""
    rng = np.random.default_rng(100 + k + n)
    out = []
    for _ in range(k):
        cx, cz = rng.uniform(x0 * 0.8, x1 * 0.8), rng.uniform(z0 + 0.1 * (z1 - z0), z1 - 0.1 * (z1 - z0))
        hx, hz = 0.25 * pitch_x * (n - 1) / 2, 0.25 * pitch_z * (n - 1) / 2
        out.append(lib.view((n, 1, n), (cx - hx, 0, cz - hz), (cx + hx, 0, cz + hz)))
    return out


def xplane_views():
    """the XZ and the YZ plane through the array's axis, each of the case's own grid size (the reference's 3DXPlane view)"""
    return [lib.view(own, (x0, x0, z0), (x1, x1, z1), plane="xz", tag=0),        # BeamformerViewPlaneTag_XZ, _YZ
            lib.view(own, (x0, x0, z0), (x1, x1, z1), plane="yz", tag=1)]


def sets():
    for n in (16, 32):
        for k in (int(v) for v in args.views.split(",")):
            yield f"{k} patches of {n} x 1 x {n}", patch_views(k, n)
    yield "X-plane: 2 planes of the case's grid", xplane_views()


def block_with(view):
    bp = type(acq.bp).from_buffer_copy(acq.bp)
    bp.das_voxel_transform[:] = list(view.das_voxel_transform)
    bp.output_points[:3] = list(view.output_points)
    return bp


rows = []
for label, views in sets():
    K = len(views)
    array = (P.HipView * K)(*views)
    blocks = [block_with(v) for v in views]
    assert L.beamformer_push_simple_parameters(C.byref(acq.bp)), lib.last_error()
    infos = {"views_kernel": [], "per_view": []}

    def views_push(mode, key):
        def run():
            L.beamformer_hip_set_das_path(mode)
            assert L.beamformer_hip_push_data_views_with_compute(ptr, size, array, K, 0), lib.last_error()
            assert L.beamformer_hip_synchronize()
            infos[key].append(lib.last_views_info())
        return run

    def today():
        L.beamformer_hip_set_das_path(0)
        for bp in blocks:
            assert L.beamformer_push_parameters(C.cast(C.byref(bp), C.POINTER(P.Parameters))), lib.last_error()
            assert L.beamformer_push_data_with_compute(ptr, size, 0, 0), lib.last_error()
        assert L.beamformer_hip_synchronize()
        assert L.beamformer_push_parameters(C.cast(C.byref(acq.bp), C.POINTER(P.Parameters)))

    runs = {"views_kernel": views_push(P.HIP_DAS_PATH_PREFER_VIEWS_KERNEL, "views_kernel"),
            "per_view": views_push(P.HIP_DAS_PATH_NO_VIEWS_KERNEL, "per_view"), "today": today}
    times = {k: [] for k in runs}
    for round_ in range(args.repeats + 2):
        for key, run in runs.items():                      # alternating: the three in turn, round after round
            assert L.beamformer_hip_synchronize()
            t0 = time.perf_counter()
            run()
            if round_ >= 2:
                times[key].append(time.perf_counter() - t0)
    L.beamformer_hip_set_das_path(0)
    last = infos["views_kernel"][-1]
    row = {"views": label, "view_count": K, "tiles": int(sum(-(-int(np.prod(list(v.output_points))) // 256) for v in views)),
           "kernel_views": int(last.route.kernel_views), "das_launches_views_kernel": int(last.route.das_launches),
           "das_launches_per_view": int(infos["per_view"][-1].route.das_launches)}
    for key in runs:
        row[key + "_us"] = statistics.median(times[key]) * 1e6
    row["per_view_spread_us"] = (max(times["per_view"]) - min(times["per_view"])) * 1e6
    row["decide_views_us"] = statistics.median(float(i.decide_us) for i in infos["views_kernel"][2:])
    row["views_kernel_over_per_view"] = row["views_kernel_us"] / row["per_view_us"]
    row["views_kernel_over_today"] = row["views_kernel_us"] / row["today_us"]
    row["not_slower_than_per_view"] = bool(row["views_kernel_us"] <= row["per_view_us"] + 3 * row["per_view_spread_us"])
    rows.append(row)
    print(json.dumps(row), flush=True)

# the smallest tile count from which on every row of the table passes
passing = None
for row in sorted(rows, key=lambda r: r["tiles"], reverse=True):
    if not row["not_slower_than_per_view"]:
        break
    passing = row["tiles"]
result = {"commit": args.commit, "repeats": args.repeats, "acquisition": acq.name,
          "timing": "wall clock per push, fence to fence, upload included, median; the three routes timed in turn",
          "min_tiles_from_this_table": passing, "rows": rows}
if args.json:
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1)
print(json.dumps({"min_tiles_from_this_table": passing}))
