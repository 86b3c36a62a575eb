"""Out-of-sample fuzz beyond the fixed seeds of tests/test_gpu_random.py and tests/test_gpu_staged_paired.py: seeds FIRST..LAST of the
generators of tests/draws.py, every draw against the oracle with the SUITE'S comparison (tests/parity.py compare(): the tolerance of the
pipeline's arithmetic; on the flip set -- the voxels where the float oracle and its double twin keep a row-end term differently -- the
first bar against the float oracle; elsewhere, for a voxel over the first bar, the double-precision truth -- never another kernel of
the library):
  general    draws on the automatic path
  separable  draws on the automatic path, and where the LDS-staged kernel ran, again with every staged term range-checked
  tile       draws with the block-staged factored kernel asked for (flags 0x10 | 0x100)
  plane      view planes as the reference's harness beamforms them, without the small-frame channel split (0x10: the kernels a full-size plane gets)
  plane_hercules   the HERCULES-family draws of `plane` with the aligned-grid kernel asked for (6)
  paired     draw_paired with the LDS-staged kernel asked for in 32 x 32 tiles with 32-sample windows (3, STAGED_SHAPE 5,5,5): the
             channel-paired form; draws it is not planned for are skipped and counted; again with every staged term range-checked
Writes a JSON summary: draws, failures, kernels taken, planes the row-end rule re-routed, and per generator the draws that needed the
second bar, the flip-set voxels and the largest excess over the oracle's own distance from the truth among the second-bar voxels.
PYTHONPATH=. python tools/auto_fuzz.py 72 1200 [--json fuzz.json] [--generators general,separable,tile]"""
import argparse
import json
import sys
import traceback

import numpy as np

from ogl_beamforming_amd import lib as bflib
from oracle import binding as oracle
from tests import draws as R, parity
from tests.das_push import last_timings
from tests.parity import reference

ap = argparse.ArgumentParser()
ap.add_argument("first", type=int)
ap.add_argument("last", type=int)
ap.add_argument("--json", default="")
ap.add_argument("--generators", default="general,separable,tile,plane,plane_hercules,paired")
args = ap.parse_args()
L = bflib.library()
GENERATORS = {"general": (R.draw, 0), "separable": (R.draw_separable, 0), "tile": (R.draw_tile, 0x110), "plane": (R.draw_plane, 0x10),
              "plane_hercules": (R.draw_plane, 6), "paired": (R.draw_paired, 3)}
summary = {"seeds": [args.first, args.last], "comparison": "tests/parity.py compare(): tolerance of the pipeline; first bar on the flip set; "
           "elsewhere second bar against the oracle's double twin with the oracle's largest distance from it off the flip set",
           "generators": {}, "failures": []}
total = failed_total = 0
for name in args.generators.split(","):
    gen, mode = GENERATORS[name]
    hooks = {"STAGED_SHAPE": "5,5,5"} if name == "paired" else {}
    ran = failed = row_end_draws = second_bar = flip_voxels = not_planned = 0
    worst_excess = None
    second_bar_list = []
    paths = {}
    for key, value in hooks.items():
        bflib.set_hook(key, value)
    for seed in range(args.first, args.last):
        try:
            acq = gen(seed)
            if name == "plane_hercules" and int(acq.bp.acquisition_kind) not in (int(R.K.HERCULES), int(R.K.UHERCULES)):
                continue
            if name == "paired":
                L.beamformer_hip_set_das_path(mode)
                try:
                    if int(bflib.describe_das(acq.bp, acq.filters)[4].uniform_tables) != 2:
                        not_planned += 1
                        continue
                finally:
                    L.beamformer_hip_set_das_path(0)
            ref, pairs, flags = reference(oracle, acq)
        except Exception:                               # a draw the generator or the oracle's planner cannot build
            continue
        ok = ~np.isnan(ref)
        if not ok.any() or np.max(np.abs(ref[ok])) == 0:
            continue
        path = -1
        verdicts = []
        try:
            L.beamformer_hip_set_das_path(mode)
            gpu = bflib.beamform(acq.bp, acq.rf, acq.filters)
            t = last_timings(bflib)
            path = int(t.das_path)
            paths[path] = paths.get(path, 0) + 1
            row_end_draws += int(t.das_row_end_planes) > 0
            ran += 1
            if name == "paired":
                assert path == 2, f"the paired form was planned, path {path} ran"
            verdicts.append(parity.compare(gpu, ref, acq, flags, path=path, label=f"{name}/{seed}"))
            if path == 2:
                bflib.set_hook("STAGED_CHECKED", "1")
                try:
                    checked = bflib.beamform(acq.bp, acq.rf, acq.filters)
                    assert int(last_timings(bflib).staged_window_violations) == 0, "window violation"
                    if name == "paired":
                        assert np.array_equal(checked.view(np.uint32), gpu.view(np.uint32)), "range-checked frame differs from the plain one"
                    verdicts.append(parity.compare(checked, ref, acq, flags, path=path, label=f"{name}/{seed}/checked"))
                finally:
                    bflib.set_hook("STAGED_CHECKED", None)
        except AssertionError as e:
            failed += 1
            what = str(e)[:200] or traceback.format_exc(limit=-1).strip().splitlines()[-2].strip()[:200]
            summary["failures"].append({"generator": name, "seed": seed, "path": path, "what": what})
            print(name, "seed", seed, "path", path, "FAIL:", what, flush=True)
        except Exception:
            failed += 1
            summary["failures"].append({"generator": name, "seed": seed, "path": path, "what": "exception"})
            print(name, "seed", seed, "ERROR", flush=True); traceback.print_exc(limit=1)
        finally:
            L.beamformer_hip_set_das_path(0)
        if verdicts:
            flip_voxels += verdicts[0].flip_voxels
            second = [v for v in verdicts if v.bar == "second"]
            if second:
                second_bar += 1
                excess = max(v.worst_excess for v in second)
                worst_excess = excess if worst_excess is None else max(worst_excess, excess)
                second_bar_list.append({"seed": seed, "path": path, "voxels": max(v.second_bar_voxels for v in second), "worst_excess": excess,
                                        "max_rel_err": max(v.max_rel_err for v in second), "flip_voxels": verdicts[0].flip_voxels})
        if ran and ran % 100 == 0:
            print(f"{name}: {ran} draws, {failed} failures so far", flush=True)
    for key in hooks:
        bflib.set_hook(key, None)
    summary["generators"][name] = {"draws": ran, "failures": failed, "das_paths_taken": {str(k): v for k, v in sorted(paths.items())},
                                   "draws_with_planes_rerouted_by_the_row_end_rule": row_end_draws, "second_bar_draws": second_bar,
                                   "flip_voxels": flip_voxels, "worst_excess": worst_excess, "second_bar": second_bar_list}
    if name == "paired":
        summary["generators"][name]["skipped_not_planned_paired"] = not_planned
    total += ran; failed_total += failed
    print(f"{name}: {ran} draws, {failed} failures, DAS paths taken: {dict(sorted(paths.items()))}, row-end re-routed draws: {row_end_draws}, "
          f"second bar: {second_bar} draws (worst excess {worst_excess}), flip-set voxels: {flip_voxels}"
          + (f", not planned paired: {not_planned}" if name == "paired" else ""), flush=True)
summary["draws"] = total; summary["failed"] = failed_total
if args.json:
    json.dump(summary, open(args.json, "w"), indent=1)
print(f"{total} draws, {failed_total} failures")
sys.exit(1 if failed_total else 0)
