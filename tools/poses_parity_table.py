#!/usr/bin/env python3
"""Runs tests/test_gpu_poses.py on the device and reduces every compare() of the run (tests/parity.py LOG) to one row per
(kernel, pose): frames, worst max_rel_err (linear and cubic interpolation: the figure compare() holds against its bars; frames with
nearest interpolation, where a flipped tap is a whole sample and the oracle's ambiguity budget is the bar, are counted and their worst
figure kept apart), frames that needed the second bar, flip-set voxels -- profiles/poses_parity.json.

    python tools/poses_parity_table.py OUT.json [pytest arguments]

"kernel" is the DAS path that computed the frame (0 general, 1 gather, 2 LDS-staged, 3 factored, 4 HERCULES, 5 block-staged), or the
fused multi-frame kernel the test drove (burst, views, burst views, variants).  The run stops at the first failure that is not a
failed assertion -- an error of the device or of the library: nothing more is launched on a device that reported one."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PATHS = {0: "0 general", 1: "1 gather", 2: "2 LDS-staged", 3: "3 factored", 4: "4 HERCULES", 5: "5 block-staged"}
FUSED = (("/burst views fused kernel/", "burst views kernel"), ("/views kernel/", "views kernel"), ("/per-view route/", "views push, per-view route"),
         ("/variants kernel/", "variants kernel"), ("/burst5/", "burst kernel"))


class StopOnDeviceError:
    """a test that fails with anything but an AssertionError ends the session"""

    def pytest_runtest_makereport(self, item, call):
        if call.excinfo is not None and not call.excinfo.errisinstance((AssertionError, pytest.skip.Exception)):
            item.session.shouldstop = f"{item.nodeid}: {call.excinfo.typename}: not a failed assertion -- stopping"


def classify(entry):
    from tests import poses
    label = entry["test"] or ""
    kernel = next((name for mark, name in FUSED if mark in label), None) or PATHS.get(entry["das_path"], str(entry["das_path"]))
    if label.startswith("draw_posed/"):
        return kernel, label.split("/")[1]
    for pose in poses.ALL:
        if f"@{pose}" in label or f"[{pose}-" in label:
            return kernel, pose
    return kernel, "?"


def reduce(log):
    from tests import poses
    rows = {}
    for e in log:
        kernel, pose = classify(e)
        row = rows.setdefault((kernel, pose), {"kernel": kernel, "pose": pose, "frames": 0, "worst_max_rel_err": 0.0, "second_bar_frames": 0, "flip_voxels": 0,
                                               "nearest_frames": 0, "nearest_worst_max_rel_err": 0.0})
        row["frames"] += 1
        if e["rule"] == "nearest":
            row["nearest_frames"] += 1
            row["nearest_worst_max_rel_err"] = max(row["nearest_worst_max_rel_err"], e["max_rel_err"])
        else:
            row["worst_max_rel_err"] = max(row["worst_max_rel_err"], e["max_rel_err"])
        row["second_bar_frames"] += e["bar"] == "second"
        row["flip_voxels"] += e["flip_voxels"]
    classes = {}
    for (kernel, pose), row in rows.items():
        kind = "general" if pose in poses.GENERAL or pose == "random_rotation" else "special"
        classes.setdefault(kind, {}).setdefault(kernel, 0)
        classes[kind][kernel] += row["frames"]
    return sorted(rows.values(), key=lambda r: (r["kernel"], r["pose"])), classes


def main():
    out = sys.argv[1]
    status = pytest.main(["-m", "gpu", "-q", "-p", "no:cacheprovider", os.path.join(ROOT, "tests", "test_gpu_poses.py")] + sys.argv[2:],
                         plugins=[StopOnDeviceError()])
    from tests import parity
    rows, classes = reduce(parity.LOG)
    with open(out, "w") as f:
        json.dump({"pytest_exit_status": int(status), "frames": len(parity.LOG), "frames_by_pose_class_and_kernel": classes, "rows": rows}, f, indent=1)
    print(f"{len(parity.LOG)} frames compared, {len(rows)} (kernel, pose) rows -> {out}")
    return int(status)


if __name__ == "__main__":
    sys.exit(main())
