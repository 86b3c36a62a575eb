"""What a variants push buys (beamformer_hip_push_data_variants_with_compute): wall time per push, fence to fence with the upload, of
ONE RF frame beamformed under K candidate speeds of sound (a) through the variants kernel (csrc/das_variants.hip; das path flag 0x8000:
whatever the tile count), (b) down the per-variant route (flag 0x4000: each variant's single-frame launch on the shared DAS input),
(c) by K x (parameter push with the candidate's speed + beamformer_push_data_with_compute) -- what a caller had before the variants
push, and the baseline the feature is reported against.  The three are timed in turn, the median of --repeats runs after two warm-up
runs each; a route's run-to-run spread is the largest minus the smallest of its runs.  Beside them the device-side DAS time of (a)
and (b) (beamformer_hip_get_last_variants_info, median of the same runs).

Acquisition: BASELINE config 1 (ogl_beamforming_amd/configs.py: 64 channels, one transmit, its own RF) on its own 256 x 256 plane, and
-- for the threshold, which counts variants x 256-voxel tiles -- on patches of 16 x 16 and 32 x 32 voxels inside it (1 and 4 tiles);
K = 1, 2, 4, 8, 16, 64 speeds spread over 1400 .. 1680 m/s.

csrc/das_select.h's two thresholds are read off this table by one rule: the smallest measured count from which (a) is not slower than
(b) by more than three times (b)'s spread in every row at that count and above -- kVariantsMinTiles with variants x tiles as the count
("min_tiles_from_this_table"), kVariantsMinVariants with the number of variants ("min_variants_from_this_table").  Run from the
repository root on a GPU box:
PYTHONPATH=. python tools/variants_rate.py --json profiles/variants_rate.json [--commit ID]"""
import argparse
import ctypes as C
import json
import statistics
import subprocess
import time

import numpy as np

from ogl_beamforming_amd import configs, lib, params as P

ap = argparse.ArgumentParser()
ap.add_argument("--counts", default="1,2,4,8,16,64")
ap.add_argument("--patches", default="16,32", help="square patches (voxels a side) measured beside config 1's own plane")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--json", default="")
ap.add_argument("--commit", default="")
args = ap.parse_args()

L = lib.library()
L.beamformer_set_global_timeout(0xFFFFFFFF)
DAS = int(P.ShaderKind.DAS)
PREFER, NO_KERNEL = P.HIP_DAS_PATH_PREFER_VARIANTS_KERNEL, P.HIP_DAS_PATH_NO_VARIANTS_KERNEL


def clocks():
    """what rocm-smi reports about the clocks right now (a query only), or the reason it could not be asked"""
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--showperflevel", "--json"], capture_output=True, text=True, timeout=20)
        d = json.loads(r.stdout)
        card = next(iter(d.values())) if d else {}
        return {k: str(v) for k, v in card.items() if any(w in k.lower() for w in ("sclk", "mclk", "performance"))}
    except Exception as e:
        return {"error": str(e)[:200]}


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


def on_patch(bp, side):
    """config 1's block on a patch of side x side voxels in the middle of its plane (side 0: the plane itself)"""
    out = type(bp).from_buffer_copy(bp)
    if side:
        m = list(bp.das_voxel_transform)          # das_transform_2d_xz: x extent m[0] from m[12], depth extent m[6] from m[14]
        fx, fz = side / bp.output_points[0], side / bp.output_points[1]
        m[12] += m[0] * (0.5 - fx / 2); m[0] *= fx
        m[14] += m[6] * (0.5 - fz / 2); m[6] *= fz
        out.das_voxel_transform[:] = m
        out.output_points[:3] = [side, side, 1]
    return out


acq = configs.config(1)
rf = np.ascontiguousarray(acq.rf)
ptr, size = rf.ctypes.data_as(C.c_void_p), rf.nbytes
for s, fp in enumerate(acq.filters):
    assert L.beamformer_create_filter(C.byref(fp), s, 0), lib.last_error()
rows = []
idle = clocks()
before = None
for side in [int(v) for v in args.patches.split(",") if v] + [0]:
    bp = on_patch(acq.bp, side)
    assert L.beamformer_push_simple_parameters(C.byref(bp)), lib.last_error()
    L.beamformer_hip_set_das_path(0)
    single_path = lib.describe_das(bp, acq.filters)[0]
    t0 = time.perf_counter()                       # single pushes for a second: the clocks leave their idle state before anything is timed
    while time.perf_counter() - t0 < 1.0:
        assert L.beamformer_push_data_with_compute(ptr, size, 0, 0), lib.last_error()
    assert L.beamformer_hip_synchronize()
    if before is None:
        before = clocks()
    for K in (int(v) for v in args.counts.split(",")):
        speeds = [1400.0 + 280.0 * (k + 0.5) / K for k in range(K)]
        variants = [lib.variant_of(bp, speed_of_sound=c) for c in speeds]
        array = (P.HipDasVariant * K)(*variants)
        blocks = [lib.with_variant(bp, v) for v in variants]          # (c)'s parameter pushes
        L.beamformer_hip_set_das_path(PREFER)
        described = lib.describe_variants(bp, variants, acq.filters)
        tiles = int(described.kernel_tiles) // K if described.kernel_variants else 0
        row = {"acquisition": acq.name, "points": [int(n) for n in bp.output_points[:3]], "variants": K, "tiles": tiles, "variants_x_tiles": K * tiles,
               "single_path": single_path, "rf_bytes": size}

        def push():
            assert L.beamformer_hip_push_data_variants_with_compute(ptr, size, array, K, 0, 0), lib.last_error()
            assert L.beamformer_hip_synchronize()

        def pushes():
            for k in range(K):
                assert L.beamformer_push_simple_parameters(C.byref(blocks[k])), lib.last_error()
                assert L.beamformer_push_data_with_compute(ptr, size, 0, 0), lib.last_error()
            assert L.beamformer_hip_synchronize()

        assert L.beamformer_push_simple_parameters(C.byref(bp)), lib.last_error()
        for label, mode in (("kernel", PREFER), ("per_variant", NO_KERNEL)):
            L.beamformer_hip_set_das_path(mode)
            infos = []
            times = runs_seconds(push, args.repeats, lambda: infos.append(lib.last_variants_info()))
            row[label + "_us_per_push"] = statistics.median(times) * 1e6
            row[label + "_spread_us_per_push"] = (max(times) - min(times)) * 1e6
            row[label + "_kernel_variants"] = int(infos[-1].route.kernel_variants)
            row[label + "_das_us_per_push"] = statistics.median(das_ms(i) for i in infos) * 1e3
            row[label + "_device_us_per_push"] = statistics.median(float(i.variants_ms) for i in infos) * 1e3
            row[label + "_decide_us"] = statistics.median(float(i.decide_us) for i in infos)
        L.beamformer_hip_set_das_path(0)
        times = runs_seconds(pushes, args.repeats)
        row["pushes_us_per_push"] = statistics.median(times) * 1e6
        row["pushes_spread_us_per_push"] = (max(times) - min(times)) * 1e6
        assert L.beamformer_push_simple_parameters(C.byref(bp)), lib.last_error()
        row["kernel_over_per_variant"] = row["kernel_us_per_push"] / row["per_variant_us_per_push"]
        row["kernel_over_pushes"] = row["kernel_us_per_push"] / row["pushes_us_per_push"]
        row["per_variant_over_pushes"] = row["per_variant_us_per_push"] / row["pushes_us_per_push"]
        row["not_slower_than_per_variant"] = bool(row["kernel_us_per_push"] <= row["per_variant_us_per_push"] + 3 * row["per_variant_spread_us_per_push"])
        rows.append(row)
        print(json.dumps(row), flush=True)



def smallest_from_which_not_slower(key):
    """the smallest measured row[key] from which the kernel is not slower in every row at that count and above (none: None)"""
    chosen = None
    for n in sorted({r[key] for r in rows}, reverse=True):
        at_n = [r for r in rows if r[key] == n]
        if not all(r["kernel_kernel_variants"] == r["variants"] and r["not_slower_than_per_variant"] for r in at_n):
            break
        chosen = n
    return chosen


result = {"commit": args.commit, "repeats": args.repeats, "timing": "wall clock per push, fence to fence, upload included, median; spread: largest minus smallest run",
          "threshold_rule": "smallest count (variants x tiles; variants) from which (a) <= (b) + 3 x (b)'s spread, in every row measured at that count and above",
          "min_tiles_in_force": int(lib.describe_variants(acq.bp, [lib.variant_of(acq.bp)], acq.filters).min_tiles),
          "min_variants_in_force": int(lib.describe_variants(acq.bp, [lib.variant_of(acq.bp)], acq.filters).min_variants),
          "min_tiles_from_this_table": smallest_from_which_not_slower("variants_x_tiles"),
          "min_variants_from_this_table": smallest_from_which_not_slower("variants"), "clocks_idle": idle, "clocks_before": before, "clocks_after": clocks(), "rows": rows}
print(json.dumps({k: v for k, v in result.items() if k != "rows"}))
if args.json:
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1)
