"""What a READI sweep buys (beamformer_hip_push_data_readi_sweep_with_compute): wall time per frame, fence to fence with the upload, of
the N group acquisitions of a READI sequence pushed (a) as one sweep through the sweep kernel (csrc/das_burst.hip:
das_readi_burst_kernel), (b) as one sweep forced down the per-frame DAS route (das path flag 0x400), (c) by N x (parameter push with
the frame's readi_group + beamformer_push_data_with_compute) -- what a caller had before the sweep, and the baseline the feature is
reported against.  The three are timed in turn, the median of --repeats runs after two warm-up runs each; (b)'s run-to-run spread is
the largest minus the smallest of its runs.  Beside them the device-side DAS time per frame of (a) and (b)
(beamformer_hip_get_last_burst_info, median of the same runs).

Acquisitions: the `readi` test case's geometry (tests/cases.py) scaled to a 256 x 1 x 256 plane and 64 channels, G = 4, 8, 16 groups
of 64 / G transmit events; N = G, 2G, 4G and 64 frames (and --extra-frames, around the threshold in force: below it (a) runs (b)'s
route and there is nothing to judge), group k % G for frame k.

csrc/das_select.h's kReadiSweepMinFrames is read off this table: the smallest N from which (a) is not slower than (b) by more than three
times (b)'s spread in every configuration measured at that N and above ("min_frames_from_this_table").  Run from the repository root
on a GPU box:
PYTHONPATH=. python tools/readi_rate.py --json profiles/readi_rate.json [--commit ID]"""
import argparse
import ctypes as C
import json
import statistics
import subprocess
import time

import numpy as np

from ogl_beamforming_amd import configs, lib, params as P

ap = argparse.ArgumentParser()
ap.add_argument("--groups", default="4,8,16")
ap.add_argument("--extra-frames", default="5,6", help="frame counts measured beside G, 2G, 4G and 64: around the threshold in force")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--json", default="")
ap.add_argument("--commit", default="")
args = ap.parse_args()

L = lib.library()
L.beamformer_set_global_timeout(0xFFFFFFFF)
DAS = int(P.ShaderKind.DAS)
NO_KERNEL = 0x400            # BeamformerHipDasPath_NoBurstKernel


def clocks():
    """what rocm-smi reports about the clocks right now (a query only), or the reason it could not be asked"""
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--showperflevel", "--json"], capture_output=True, text=True, timeout=20)
        d = json.loads(r.stdout)
        card = next(iter(d.values())) if d else {}
        return {k: str(v) for k, v in card.items() if any(w in k.lower() for w in ("sclk", "mclk", "performance"))}
    except Exception as e:
        return {"error": str(e)[:200]}


def readi_plane(G):
    """the `readi` case (16 channels, 4 x 4 transmit elements, 512 samples, 16 x 1 x 16 over +-1 mm x 5 .. 9 mm) at 64 channels,
    G x 64 / G transmit elements and 256 x 1 x 256 voxels over the lateral extent of the wider array"""
    return configs.forces(f"readi_plane_g{G}", 64, 64 // G, 512, (256, 1, 256), (-4e-3, 0, 5e-3), (4e-3, 0, 9e-3), seed=33, decode=0,
                          readi_groups=G, readi_group=0)


def runs_seconds(run, repeats, after=None):
    """wall times of `repeats` runs after two warm-up runs; `after` (called after every timed run) may collect device-side figures"""
    run(); run()
    times = []
    for _ in range(repeats):
        assert L.beamformer_hip_synchronize()
        t0 = time.perf_counter()
        run()
        times.append(time.perf_counter() - t0)
        if after:
            after()
    return times


def das_ms(info):
    kinds = [int(info.stage_kind[k]) for k in range(int(info.stage_count))]
    return float(info.stage_ms[kinds.index(DAS)])


def warm_up(acq, seconds=1.0):
    """sweeps of 16 for a second: the clocks leave their idle state before anything is timed"""
    rf = np.zeros((16,) + acq.rf.shape, acq.rf.dtype)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        assert L.beamformer_hip_push_data_readi_sweep_with_compute(rf.ctypes.data_as(C.c_void_p), rf[0].nbytes, 16, None, 0, 0), lib.last_error()
    assert L.beamformer_hip_synchronize()


rows = []
extra = [int(v) for v in args.extra_frames.split(",") if v]
idle = clocks()
before = None
for G in (int(v) for v in args.groups.split(",")):
    acq = readi_plane(G)
    assert L.beamformer_push_simple_parameters(C.byref(acq.bp)), lib.last_error()
    L.beamformer_hip_set_das_path(0)
    single_path = lib.describe_das(acq.bp, acq.filters)[0]
    warm_up(acq)
    if before is None:
        before = clocks()
    rng = np.random.default_rng(3)
    blocks = []
    for g in range(G):                       # (c)'s parameter pushes: the block with each group
        bp = type(acq.bp).from_buffer_copy(acq.bp)
        bp.readi_group = g
        blocks.append(bp)
    for n in sorted({G, 2 * G, 4 * G, 64} | set(extra)):
        rf = np.clip(np.rint(rng.normal(0, 1000.0, (n,) + acq.rf.shape)), -32000, 32000).astype(acq.rf.dtype)
        ptr, size = rf.ctypes.data_as(C.c_void_p), rf[0].nbytes
        frames = [rf[k].ctypes.data_as(C.c_void_p) for k in range(n)]
        ids = [k % G for k in range(n)]
        array = (C.c_uint32 * n)(*ids)
        row = {"acquisition": acq.name, "groups": G, "transmit_events": 64 // G, "frames": n, "single_path": single_path, "frame_bytes_rf": size}

        def sweep():
            assert L.beamformer_hip_push_data_readi_sweep_with_compute(ptr, size, n, array, 0, 0), lib.last_error()
            assert L.beamformer_hip_synchronize()

        def pushes():
            for k in range(n):
                assert L.beamformer_push_simple_parameters(C.byref(blocks[ids[k]])), lib.last_error()
                assert L.beamformer_push_data_with_compute(frames[k], size, 0, 0), lib.last_error()
            assert L.beamformer_hip_synchronize()

        assert L.beamformer_push_simple_parameters(C.byref(blocks[0])), lib.last_error()
        for label, mode in (("sweep_kernel", 0), ("sweep_per_frame", NO_KERNEL)):
            L.beamformer_hip_set_das_path(mode)
            infos = []
            times = runs_seconds(sweep, args.repeats, lambda: infos.append(lib.last_burst_info()))
            row[label + "_us_per_frame"] = statistics.median(times) / n * 1e6
            row[label + "_spread_us_per_frame"] = (max(times) - min(times)) / n * 1e6
            row[label + "_ran_sweep_kernel"] = int(infos[-1].route.burst_kernel)
            row[label + "_das_us_per_frame"] = statistics.median(das_ms(i) for i in infos) * 1e3 / n
            row[label + "_device_us_per_frame"] = statistics.median(float(i.burst_ms) for i in infos) * 1e3 / n
        L.beamformer_hip_set_das_path(0)
        row["pushes_us_per_frame"] = statistics.median(runs_seconds(pushes, args.repeats)) / n * 1e6
        assert L.beamformer_push_simple_parameters(C.byref(blocks[0])), lib.last_error()
        row["kernel_over_per_frame"] = row["sweep_kernel_us_per_frame"] / row["sweep_per_frame_us_per_frame"]
        row["kernel_over_pushes"] = row["sweep_kernel_us_per_frame"] / row["pushes_us_per_frame"]
        row["per_frame_over_pushes"] = row["sweep_per_frame_us_per_frame"] / row["pushes_us_per_frame"]
        row["not_slower_than_per_frame"] = bool(row["sweep_kernel_us_per_frame"] <= row["sweep_per_frame_us_per_frame"] + 3 * row["sweep_per_frame_spread_us_per_frame"])
        rows.append(row)
        print(json.dumps(row), flush=True)

# the smallest measured N from which the kernel is not slower in every row at that N and above (none: null)
counts = sorted({r["frames"] for r in rows})
chosen = None
for n in reversed(counts):
    at_n = [r for r in rows if r["frames"] == n]
    if not all(r["sweep_kernel_ran_sweep_kernel"] and r["not_slower_than_per_frame"] for r in at_n):
        break                                # slower here, or below the threshold in force: the kernel did not run, nothing to judge
    chosen = n
result = {"commit": args.commit, "repeats": args.repeats, "timing": "wall clock, fence to fence, upload included, median; spread: largest minus smallest run",
          "threshold_rule": "smallest N from which (a) <= (b) + 3 x (b)'s spread, in every configuration measured at that N and above",
          "sweep_kernel_forced_from": int(lib.describe_readi_sweep(readi_plane(4).bp, 64).min_frames),
          "min_frames_from_this_table": chosen, "clocks_idle": idle, "clocks_before": before, "clocks_after": clocks(), "rows": rows}
print(json.dumps({k: v for k, v in result.items() if k != "rows"}))
if args.json:
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1)
