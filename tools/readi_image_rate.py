"""What the READI image push buys (beamformer_hip_push_data_readi_image_with_compute): the compounded image of the N = G group
acquisitions of a READI sequence obtained (a) by ONE image push -- the decode across acquisitions (csrc/readi_decode.hip), then one
FORCES DAS pass over G x A transmits -- and (b) by what the library offered before it: the sweep push of the same RF
(beamformer_hip_push_data_readi_sweep_with_compute, N READI DAS passes) followed by beamformer_hip_sum_last_frames(N).  Both end with
the result in host memory: (a) reads its frame back with beamformer_get_last_frames, (b)'s sum call returns the average.

The two sides ALTERNATE, run by run, after two warm-up runs each; wall clock, fence to fence, upload and read-back included; the
median of --repeats runs a side, the spread the largest minus the smallest run.  Beside them the device-side times of the same runs
(hipEvent pairs: beamformer_hip_get_last_readi_image_info / _burst_info): the DAS stage of each side, (a)'s decode stage, and each
push's first event to last.  The results are compared at the size timed: max|N x average - image| over max|image|.

Geometry: the harness-class FORCES plane (configs.harness("forces"): 256 channels x 128 transmit elements x 4096 Int16 samples,
{Demodulate, DAS}, cubic, F# 0.5, 512 x 1024 voxels) reduced to a READI block: G groups of 128 / G transmit events, decode off.
--scale shrinks every count (a rehearsal; a toy size measures overheads).  Run from the repository root on a GPU box:
PYTHONPATH=. python tools/readi_image_rate.py --json profiles/readi_image_rate.json [--commit ID]"""
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
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--json", default="")
ap.add_argument("--commit", default="")
args = ap.parse_args()
assert args.repeats >= 5, "at least five runs a side"

L = lib.library()
L.beamformer_set_global_timeout(0xFFFFFFFF)
DAS, DECODE = int(P.ShaderKind.DAS), int(P.ShaderKind.Decode)


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
    """the harness's FORCES plane with its transmit elements dealt into G READI groups"""
    h = configs.harness("forces", args.scale)
    bp = h.bp
    Cn, T, Sn = int(bp.channel_count), int(bp.acquisition_count), int(bp.sample_count)
    assert T % G == 0
    points = tuple(int(v) for v in bp.output_points[:3])
    scale = Sn / 4096.0
    lo, hi = tuple(v * scale for v in (-60e-3, -60e-3, 10e-3)), tuple(v * scale for v in (60e-3, 60e-3, 165e-3))
    acq = configs.forces(f"harness_readi_g{G}", Cn, T // G, Sn, points, lo, hi, seed=73, interp=P.InterpolationMode.Cubic, f_number=0.5,
                         pitch=float(bp.xdc_element_pitch[0]), fs=float(bp.sampling_frequency), fd=float(bp.demodulation_frequency),
                         stages=(P.ShaderKind.Demodulate, P.ShaderKind.DAS), decode=0, readi_groups=G, readi_group=0)
    # (the pitch went through the harness block's float32 field: the transforms agree to rounding)
    assert np.allclose(list(acq.bp.das_voxel_transform), list(bp.das_voxel_transform), rtol=1e-6, atol=0)
    assert np.allclose(list(acq.bp.xdc_transform), list(bp.xdc_transform), rtol=1e-6, atol=0)
    return acq


def stage_ms(info, kind):
    kinds = [int(info.stage_kind[k]) for k in range(int(info.stage_count))]
    return float(info.stage_ms[kinds.index(kind)])


rows = []
idle = clocks()
before = None
for G in (int(v) for v in args.groups.split(",")):
    acq = readi_plane(G)
    n = G
    for slot, fp in enumerate(acq.filters):
        assert L.beamformer_create_filter(C.byref(fp), slot, 0), lib.last_error()
    assert L.beamformer_push_simple_parameters(C.byref(acq.bp)), lib.last_error()
    L.beamformer_hip_set_das_path(0)
    rng = np.random.default_rng(5)
    rf = np.clip(np.rint(rng.normal(0, 1000.0, (n,) + acq.rf.shape)), -32000, 32000).astype(acq.rf.dtype)
    ptr, size = rf.ctypes.data_as(C.c_void_p), rf[0].nbytes
    array = (C.c_uint32 * n)(*[k % G for k in range(n)])
    shape = lib.frame_shape(acq.bp)
    voxels = int(np.prod(shape))
    frame_bytes = (voxels * 8 + 63) // 64 * 64
    image_out, sum_out = np.zeros(frame_bytes // 8, np.complex64), np.zeros(frame_bytes // 8, np.complex64)
    described = lib.describe_readi_image(acq.bp, n, None, acq.filters)
    sweep_route = lib.describe_readi_sweep(acq.bp, n, None, acq.filters)
    row = {"acquisition": acq.name, "groups": G, "transmit_events": int(acq.bp.acquisition_count), "frames": n, "channels": int(acq.bp.channel_count),
           "samples": int(acq.bp.sample_count), "voxels": voxels, "rf_bytes_per_frame": size, "image_das_path": int(described.das_path),
           "image_transmits": int(described.transmit_count), "sweep_kernel": int(sweep_route.burst_kernel), "sweep_single_path": int(sweep_route.single_path)}

    def image():
        assert L.beamformer_hip_push_data_readi_image_with_compute(ptr, size, n, array, 0, 0), lib.last_error()
        assert L.beamformer_get_last_frames(image_out.ctypes.data_as(C.c_void_p), image_out.nbytes, 1), lib.last_error()

    def sweep_and_sum():
        assert L.beamformer_hip_push_data_readi_sweep_with_compute(ptr, size, n, array, 0, 0), lib.last_error()
        assert L.beamformer_hip_sum_last_frames(n, sum_out.ctypes.data_as(C.c_void_p), sum_out.nbytes), lib.last_error()

    for _ in range(2):                                   # warm-up: every shape the timed window uses, both sides
        image(); sweep_and_sum()
    if before is None:
        before = clocks()
    times = {"image": [], "sweep_sum": []}
    device = {"image_das": [], "image_decode": [], "image_push": [], "sweep_das": [], "sweep_push": []}
    for _ in range(args.repeats):                        # alternating
        assert L.beamformer_hip_synchronize()
        t0 = time.perf_counter()
        image()
        times["image"].append(time.perf_counter() - t0)
        info = lib.last_readi_image_info()
        device["image_das"].append(stage_ms(info, DAS)); device["image_decode"].append(stage_ms(info, DECODE)); device["image_push"].append(float(info.image_ms))
        assert L.beamformer_hip_synchronize()
        t0 = time.perf_counter()
        sweep_and_sum()
        times["sweep_sum"].append(time.perf_counter() - t0)
        burst = lib.last_burst_info()                    # (the sum queues no frame: the sweep is still the newest push)
        device["sweep_das"].append(stage_ms(burst, DAS)); device["sweep_push"].append(float(burst.burst_ms))
    for side, t in times.items():
        row[side + "_ms"] = statistics.median(t) * 1e3
        row[side + "_spread_ms"] = (max(t) - min(t)) * 1e3
        row[side + "_runs_ms"] = [v * 1e3 for v in t]
    for key, v in device.items():
        row[key + "_device_ms"] = statistics.median(v)
    row["image_over_sweep_sum"] = row["image_ms"] / row["sweep_sum_ms"]
    row["image_das_over_sweep_das"] = row["image_das_device_ms"] / row["sweep_das_device_ms"]
    # the decode moves N DAS inputs in and G x A transmits out, float32 complex
    das_samples = int(acq.bp.sample_count) // 2
    moved = (n + G) * int(acq.bp.channel_count) * int(acq.bp.acquisition_count) * das_samples * 8
    row["decode_bytes"] = moved
    row["decode_tb_per_s"] = moved / (row["image_decode_device_ms"] * 1e-3) / 1e12
    # the results at the size timed: the sum call returns the average of the N frames
    scale = float(np.abs(image_out).max())
    row["max_abs_image"] = scale
    row["sweep_sum_against_image"] = float(np.abs(sum_out * np.float32(n) - image_out).max() / scale) if scale > 0 else None
    rows.append(row)
    print(json.dumps({k: v for k, v in row.items() if not k.endswith("_runs_ms")}), flush=True)

result = {"commit": args.commit, "repeats": args.repeats, "scale": args.scale,
          "timing": "wall clock, fence to fence, upload and read-back included, the two sides alternating; median; spread: largest minus smallest run; *_device_ms: hipEvent pairs, median of the same runs",
          "clocks_idle": idle, "clocks_before": before, "clocks_after": clocks(), "rows": rows}
if args.json:
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1)
