"""What a burst views push buys (beamformer_hip_push_data_burst_views_with_compute): wall time per QUEUED frame, fence to fence with
the upload, of N RF frames on K grids
  (a) as one push on the automatic path (the fused kernel, csrc/das_burst_views.hip, from kBurstViewsMinFrames RF frames on),
  (b) as one push on rung 2 (das path flag 0x400: the views kernel once per RF frame),
  (c) as one push on rung 3 (flag 0x800: every frame its single-frame launch),
  (d) as what the library offered before: K x (parameter push with that view's grid + burst push of the same RF) -- the baseline,
each the median of --repeats runs after two warm-up runs, with the spread (largest minus smallest) of those runs, and the DAS stage's
device time per frame of (a) and (b) from beamformer_hip_get_last_burst_views_info.  Config 1's RF (64 channels, one plane wave) on
K = 2 and 3 planes of 256 x 1 x 256 and on K = 16 patches of 16 x 1 x 16.  min_frames_from_this_table -- the smallest measured N from
which on (a) is not slower than (b) by more than three times (b)'s spread, in every workload -- is what csrc/das_select.h's
kBurstViewsMinFrames is set from.  (a) below the constant in force runs rung 2: such rows say so (a_rung), the fused kernel is not
measured there, and the table cannot put the threshold below that constant.  Run from the repository root on a GPU box:
PYTHONPATH=. python tools/burst_views_rate.py --json profiles/burst_views_rate.json [--commit ID]"""
import argparse
import ctypes as C
import json
import statistics
import subprocess
import time

import numpy as np

from ogl_beamforming_amd import configs, lib, params as P

ap = argparse.ArgumentParser()
ap.add_argument("--frames", default="2,4,5,6,8,16,64,256")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--json", default="")
ap.add_argument("--commit", default="")
args = ap.parse_args()

L = lib.library()
L.beamformer_set_global_timeout(0xFFFFFFFF)
DAS = int(P.ShaderKind.DAS)


def clocks():
    """what rocm-smi reports about the clocks right now (a query only), or the reason it could not be asked"""
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--showperflevel", "--json"], capture_output=True, text=True, timeout=20)
        d = json.loads(r.stdout)
        card = next(iter(d.values())) if d else {}
        return {k: str(v) for k, v in card.items() if any(w in k.lower() for w in ("sclk", "mclk", "performance"))}
    except Exception as e:
        return {"error": str(e)[:200]}


def timed(run, repeats, after=None):
    """(median, spread) of the wall time of `run` in seconds; `after` (called after every timed run) may collect device-side figures"""
    run(); run()
    times = []
    for _ in range(repeats):
        assert L.beamformer_hip_synchronize()
        t0 = time.perf_counter()
        run()
        times.append(time.perf_counter() - t0)
        if after:
            after()
    return statistics.median(times), max(times) - min(times)


def das_ms(info):
    kinds = [int(info.stage_kind[k]) for k in range(int(info.stage_count))]
    return float(info.stage_ms[kinds.index(DAS)])


acq = configs.config(1)
S = int(acq.bp.sample_count)
path = S / 25e6 * configs.SPEED_OF_SOUND
z0, z1 = 0.12 * path, 0.40 * path


def planes(k):
    """k planes of 256 x 1 x 256 (x by depth) over the image: at elevation y = 0, +2 mm, -2 mm"""
    return [lib.view((256, 1, 256), (-9.6e-3, y, z0), (9.6e-3, y, z1)) for y in (0.0, 2e-3, -2e-3)[:k]]


def patches(k):
    """k patches of 16 x 1 x 16, 1 mm wide, spread over the image"""
    out = []
    for i in range(k):
        x = -8e-3 + 1e-3 * i
        z = z0 + (z1 - z0 - 1e-3) * (i * 7 % k) / k
        out.append(lib.view((16, 1, 16), (x, 0, z), (x + 1e-3, 0, z + 1e-3)))
    return out


def on_grid(view):
    bp = type(acq.bp).from_buffer_copy(acq.bp)
    bp.das_voxel_transform[:] = list(view.das_voxel_transform)
    bp.output_points[:3] = [int(n) for n in view.output_points]
    return bp


def set_block(bp):
    for s, fp in enumerate(acq.filters):
        assert L.beamformer_create_filter(C.byref(fp), s, 0)
    assert L.beamformer_push_simple_parameters(C.byref(bp)), lib.last_error()


rows = []
idle = clocks()
set_block(acq.bp)
L.beamformer_hip_set_das_path(0)
warm = np.zeros((16,) + acq.rf.shape, acq.rf.dtype)
t0 = time.perf_counter()
while time.perf_counter() - t0 < 1.0:          # bursts of 16 for a second: the clocks leave their idle state before anything is timed
    assert L.beamformer_hip_push_data_burst_with_compute(warm.ctypes.data_as(C.c_void_p), warm[0].nbytes, 16, 0, 0), lib.last_error()
assert L.beamformer_hip_synchronize()
before = clocks()
rng = np.random.default_rng(3)
frame_counts = [int(v) for v in args.frames.split(",")]
min_frames_in_force = None

for workload, views in (("2 planes 256x1x256", planes(2)), ("3 planes 256x1x256", planes(3)), ("16 patches 16x1x16", patches(16))):
    K = len(views)
    array = (P.HipView * K)(*views)
    blocks = [on_grid(v) for v in views]
    for n in frame_counts:
        rf = np.clip(np.rint(rng.normal(0, 1000.0, (n,) + acq.rf.shape)), -32000, 32000).astype(acq.rf.dtype)
        ptr, size = rf.ctypes.data_as(C.c_void_p), rf[0].nbytes
        row = {"workload": workload, "views": K, "rf_frames": n, "frames": n * K, "frame_bytes_rf": size}

        def push():
            assert L.beamformer_hip_push_data_burst_views_with_compute(ptr, size, n, array, K, 0), lib.last_error()
            assert L.beamformer_hip_synchronize()

        def baseline():
            for bp in blocks:
                assert L.beamformer_push_simple_parameters(C.byref(bp)), lib.last_error()
                assert L.beamformer_hip_push_data_burst_with_compute(ptr, size, n, 0, 0), lib.last_error()
            assert L.beamformer_hip_synchronize()

        set_block(acq.bp)
        for label, mode in (("a", 0), ("b", P.HIP_DAS_PATH_NO_BURST_KERNEL), ("c", P.HIP_DAS_PATH_NO_VIEWS_KERNEL)):
            L.beamformer_hip_set_das_path(mode)
            infos = []
            median, spread = timed(push, args.repeats, lambda: infos.append(lib.last_burst_views_info()))
            row[label + "_us_per_frame"] = median / (n * K) * 1e6
            row[label + "_spread_us_per_frame"] = spread / (n * K) * 1e6
            row[label + "_rung"] = int(infos[-1].route.rung)
            row[label + "_das_launches"] = int(infos[-1].route.das_launches)
            min_frames_in_force = int(infos[-1].route.min_frames)
            if label != "c":
                row[label + "_das_us_per_frame"] = statistics.median(das_ms(i) for i in infos) * 1e3 / (n * K)
                row[label + "_device_us_per_frame"] = statistics.median(float(i.push_ms) for i in infos) * 1e3 / (n * K)
        L.beamformer_hip_set_das_path(0)
        median, spread = timed(baseline, args.repeats)
        row["d_us_per_frame"] = median / (n * K) * 1e6
        row["d_spread_us_per_frame"] = spread / (n * K) * 1e6
        set_block(acq.bp)
        row["a_over_b"] = row["a_us_per_frame"] / row["b_us_per_frame"]
        row["a_over_d"] = row["a_us_per_frame"] / row["d_us_per_frame"]
        row["a_not_slower_than_b"] = bool(row["a_rung"] == 1 and row["a_us_per_frame"] <= row["b_us_per_frame"] + 3.0 * row["b_spread_us_per_frame"])
        row["a_faster_than_d"] = bool(row["a_us_per_frame"] < row["d_us_per_frame"])
        rows.append(row)
        print(json.dumps(row), flush=True)


def threshold(of_rows):
    """the smallest measured N from which on every row's (a) ran the fused kernel and was not slower than (b) by more than 3 spreads"""
    best = None
    for n in sorted(frame_counts, reverse=True):
        if all(r["a_not_slower_than_b"] for r in of_rows if r["rf_frames"] == n):
            best = n
        else:
            break
    return best


result = {"commit": args.commit, "repeats": args.repeats, "timing": "wall clock per queued frame, fence to fence, upload included, median and spread (max - min)",
          "min_frames_in_force": min_frames_in_force,
          "min_frames_from_this_table": threshold(rows),
          "min_frames_by_workload": {w: threshold([r for r in rows if r["workload"] == w]) for w in dict.fromkeys(r["workload"] for r in rows)},
          "note": "rows below min_frames_in_force ran (a) on rung 2 (a_rung): the fused kernel was not measured there, so the table cannot put the threshold below the constant in force",
          "a_not_faster_than_d": [[r["workload"], r["rf_frames"]] for r in rows if not r["a_faster_than_d"]],
          "clocks_idle": idle, "clocks_before": before, "clocks_after": clocks(), "rows": rows}
if args.json:
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1)
print(json.dumps({k: v for k, v in result.items() if k != "rows"}))
