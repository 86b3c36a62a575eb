"""DAS time of the real-sample staged kernel (das_staged_real.hip) at full size: config 4's geometry (256 channels, 75 plane waves,
512^3 voxels, coherency weighting) with real samples straight into DAS -- no Demodulate stage; 2048 samples at 12.5 MHz, the rate
and row length config 4's DAS sees behind its demodulation, so the delay spread per tile is config 4's.  Prints one JSON line:
the DAS path that ran and the DAS stage's milliseconds per push (beamformer_hip_get_last_frame_timings).
Run from the repository root on a GPU box:  PYTHONPATH=. python tools/staged_real_rate.py [--pushes 5] [--planes 0]"""
import argparse
import ctypes as C
import json
import statistics

import numpy as np
import torch

from ogl_beamforming_amd import configs, lib, params as P


def acquisition():
    Cn, A, S, fs = 256, 75, 2048, 12.5e6
    half = (Cn - 1) / 2 * 0.15e-3
    path = S / fs * configs.SPEED_OF_SOUND
    z0, z1 = 0.12 * path, 0.30 * path
    return configs.rca("config4_real", Cn, A, S, (512, 512, 512), (-half, -half, z0), (half, half, z1), seed=4, cw=True, pitch=0.15e-3,
                       orientation=0x12, f_number=0.5, angles=np.linspace(-18.5, 18.5, A), demodulate=False, data_kind=P.DataKind.Float32,
                       fs=fs, fd=0.0)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--pushes", type=int, default=5)
    ap.add_argument("--planes", type=int, default=0, help="beamform only this many centre z-planes")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    L = lib.library()
    L.beamformer_set_global_timeout(0xFFFFFFFF)
    acq = acquisition()
    assert L.beamformer_push_simple_parameters(C.byref(acq.bp)), lib.last_error()
    if args.planes:
        assert L.beamformer_hip_set_output_shard(0, 256 - args.planes // 2, args.planes), lib.last_error()
    dev = torch.from_numpy(np.ascontiguousarray(acq.rf).view(np.uint8).reshape(-1)).cuda()
    t = P.HipFrameTimings()
    ms = []
    for k in range(args.pushes + 1):                      # the first push plans and allocates: not timed
        assert L.beamformer_hip_push_device_data_with_compute(C.c_void_p(dev.data_ptr()), dev.numel(), 0, 0), lib.last_error()
        assert L.beamformer_hip_get_last_frame_timings(C.byref(t)), lib.last_error()
        kinds = [int(t.stage_kind[i]) for i in range(int(t.stage_count))]
        if k:
            ms.append(float(t.stage_ms[kinds.index(int(P.ShaderKind.DAS))]))
    print(json.dumps({"das_path": int(t.das_path), "das_ms": ms, "das_ms_median": statistics.median(ms), "planes": args.planes or 512}))
