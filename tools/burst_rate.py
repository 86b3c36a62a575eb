"""What a burst buys (beamformer_hip_push_data_burst_with_compute): wall time per frame, fence to fence with the upload, of N frames
pushed (a) by N calls of beamformer_push_data_with_compute, (b) as one burst through the burst kernel (csrc/das_burst.hip),
(c) as one burst forced down the per-frame DAS route (das path flag 0x400) -- the median of --repeats runs after two warm-up runs
each -- and the device-side DAS time per frame of (b) and (c) from beamformer_hip_get_last_burst_info (median of the same runs), beside the single path's DAS
time per frame from beamformer_hip_get_last_frame_timings.  Acquisitions: BASELINE config 1 at full size (64 channels, one plane
wave, 256 x 256) and a two-transmit plane-wave RCA plane of the same size.  csrc/das_select.h's kBurstMinFrames is set from this
table.  Run from the repository root on a GPU box:
PYTHONPATH=. python tools/burst_rate.py --json profiles/burst_rate.json [--commit ID]"""
import argparse
import ctypes as C
import json
import statistics
import subprocess
import time

import numpy as np

from ogl_beamforming_amd import configs, lib, params as P

ap = argparse.ArgumentParser()
ap.add_argument("--frames", default="1,2,4,8,16,64,256")
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


def two_transmit_plane():
    """config 1's array, sample count, grid and depth range with two steered plane waves (the general kernel: fewer than three)"""
    S = 2048
    path = S / 25e6 * configs.SPEED_OF_SOUND
    return configs.rca("rca_2tx_plane", 64, 2, S, (256, 256, 1), (-9.6e-3, 0, 0.12 * path), (9.6e-3, 0, 0.40 * path), seed=21,
                       orientation=0x22, f_number=1.0, angles=np.array([-5.0, 5.0]))


def median_seconds(run, repeats, after=None):
    """median wall time of `run`; `after` (called after every timed run) may collect device-side figures of it"""
    run(); run()
    times = []
    for _ in range(repeats):
        assert L.beamformer_hip_synchronize()
        t0 = time.perf_counter()
        run()
        times.append(time.perf_counter() - t0)
        if after:
            after()
    return statistics.median(times)


def das_ms(timings_like):
    kinds = [int(timings_like.stage_kind[k]) for k in range(int(timings_like.stage_count))]
    return float(timings_like.stage_ms[kinds.index(DAS)])


rows = []
idle = clocks()


def warm_up(acq, seconds=1.0):
    """bursts of 16 for a second: the clocks leave their idle state before anything is timed"""
    rf = np.zeros((16,) + acq.rf.shape, acq.rf.dtype)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        assert L.beamformer_hip_push_data_burst_with_compute(rf.ctypes.data_as(C.c_void_p), rf[0].nbytes, 16, 0, 0), lib.last_error()
    assert L.beamformer_hip_synchronize()


before = None
for acq in (configs.config(1), two_transmit_plane()):
    for s, fp in enumerate(acq.filters):
        assert L.beamformer_create_filter(C.byref(fp), s, 0)
    assert L.beamformer_push_simple_parameters(C.byref(acq.bp)), lib.last_error()
    L.beamformer_hip_set_das_path(0)
    single_path = lib.describe_das(acq.bp, acq.filters)[0]
    warm_up(acq)
    if before is None:
        before = clocks()
    rng = np.random.default_rng(3)
    for n in (int(v) for v in args.frames.split(",")):
        rf = np.clip(np.rint(rng.normal(0, 1000.0, (n,) + acq.rf.shape)), -32000, 32000).astype(acq.rf.dtype)
        ptr, size = rf.ctypes.data_as(C.c_void_p), rf[0].nbytes
        frames = [rf[k].ctypes.data_as(C.c_void_p) for k in range(n)]
        row = {"acquisition": acq.name, "frames": n, "single_path": single_path, "frame_bytes_rf": size}

        def singles():
            for p in frames:
                assert L.beamformer_push_data_with_compute(p, size, 0, 0), lib.last_error()
            assert L.beamformer_hip_synchronize()

        def burst():
            assert L.beamformer_hip_push_data_burst_with_compute(ptr, size, n, 0, 0), lib.last_error()
            assert L.beamformer_hip_synchronize()

        row["singles_us_per_frame"] = median_seconds(singles, args.repeats) / n * 1e6
        # (the single path samples its stage events one small frame in eight: an unsampled frame reports the newest sampled one's)
        t = P.HipFrameTimings()
        assert L.beamformer_hip_get_last_frame_timings(C.byref(t))
        row["single_das_us"] = das_ms(t) * 1e3
        for label, mode in (("burst_kernel", 0), ("burst_per_frame_das", P.HIP_DAS_PATH_NO_BURST_KERNEL)):
            L.beamformer_hip_set_das_path(mode)
            infos = []
            row[label + "_us_per_frame"] = median_seconds(burst, args.repeats, (lambda: infos.append(lib.last_burst_info())) if n >= 2 else None) / n * 1e6
            if n >= 2:
                row[label + "_ran_burst_kernel"] = int(infos[-1].route.burst_kernel)
                row[label + "_das_us_per_frame"] = statistics.median(das_ms(i) for i in infos) * 1e3 / n
                row[label + "_device_us_per_frame"] = statistics.median(float(i.burst_ms) for i in infos) * 1e3 / n
        L.beamformer_hip_set_das_path(0)
        row["burst_kernel_over_singles"] = row["burst_kernel_us_per_frame"] / row["singles_us_per_frame"]
        row["burst_per_frame_das_over_singles"] = row["burst_per_frame_das_us_per_frame"] / row["singles_us_per_frame"]
        rows.append(row)
        print(json.dumps(row), flush=True)
result = {"commit": args.commit, "repeats": args.repeats, "timing": "wall clock, fence to fence, upload included, median",
          "clocks_idle": idle, "clocks_before": before, "clocks_after": clocks(), "rows": rows}
if args.json:
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1)
