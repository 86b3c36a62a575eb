"""What the device is asked to do by the peak calls (csrc/frame_ops.cpp), for comparing two builds of the library call for call.
Without arguments: three planted real frames of 24 x 1 x 40 (tests/planted.py: three spots that move one voxel a frame, one that stands
still) are pushed as one burst, and every peak call, map reset, map copy and queue call runs TWICE on them, the peak calls on each of
their paths: records downloaded and not, every deposit value, a threshold nothing exceeds (no peak at all), and thresholds that leave
the middle frame without a peak (no frame pair with peaks on both sides).  Run it under `rocprofv3 --hip-trace --stats` once a
library (OGL_BEAMFORMER_LIB selects one):
  rocprofv3 --hip-trace --stats --output-format csv -d OUT_A -- python tools/peak_api_calls.py
With --compare OUT_A OUT_B: reads the HIP API statistics of both runs and fails unless hipMemcpyAsync, hipMemsetAsync, the kernel launch
entry points, hipEventRecord, hipStreamSynchronize and hipEventSynchronize were called equally often; every other HIP function whose
count differs is listed (allocations may differ; the reader judges).  --json keeps both tables."""
import argparse
import csv
import glob
import json
import os
import re
import sys

EQUAL = re.compile(r"^hip(MemcpyAsync|MemsetAsync|EventRecord|StreamSynchronize|EventSynchronize|\w*LaunchKernel\w*)$")


def run():
    import numpy as np
    from ogl_beamforming_amd import lib, params as P
    from tests import planted

    K, (X, _, Z), height = 3, planted.PLANE, float(planted.HEIGHT)
    stack = np.zeros((K, Z, 1, X), np.float32)
    for k in range(K):
        for x, z in ((2, 2 + k), (10, 20), (18, 30 - k), (6 + k, 10)):
            stack[k, z, 0, x] = height
    blocks = [planted.block(values) for values in stack]
    lib.library().beamformer_set_global_timeout(0xFFFFFFFF)
    frames = lib.beamform_burst(blocks[0].bp, np.stack([acq.rf for acq in blocks]), blocks[0].filters)
    assert all(planted.same(frames[k], planted.expected(stack[k])) for k in range(K))
    level, nothing, identity, field = 0.5 * height, 2.0 * height, np.eye(3, 4), (X, 1, Z)
    both = P.HIP_TRACK_DEPOSIT_POINTS | P.HIP_TRACK_DEPOSIT_LINKS
    seen = {}
    for _ in range(2):
        lib.localisation_map_reset(field)
        lib.track_map_reset(field)
        for threshold in (level, nothing, (level, nothing, level)):
            rows, peaks, _ = lib.find_peaks_last_frames(K, threshold, 16)
            seen.setdefault("peaks", []).append(len(peaks))
            lib.accumulate_peaks_last_frames(K, threshold, identity)
            for records in (True, False):
                for deposit in (False, True):
                    rows, pairs, _ = lib.pair_peaks_last_frames(K, threshold, identity, 1.5, 16, deposit=deposit, records=records)
                    seen.setdefault("pairs", []).append(sum(int(r.pairs) for r in rows))
                for deposit in (0, P.HIP_TRACK_DEPOSIT_POINTS, P.HIP_TRACK_DEPOSIT_LINKS, both):
                    rows, tracks, points, _ = lib.track_peaks_last_frames(K, threshold, identity, 1.5, 16, 2, deposit=deposit, records=records)
                    seen.setdefault("tracks", []).append(sum(int(r.kept_heads) for r in rows))
            for deposit in (0, P.HIP_TRACK_DEPOSIT_POINTS, P.HIP_TRACK_DEPOSIT_LINKS, both):
                for smooth in (0, 1):
                    rows, _ = lib.draw_tracks_last_frames(K, threshold, identity, 1.5, 16, 2, smooth=smooth, deposit=deposit)
                    seen.setdefault("samples", []).append(sum(int(r.samples) for r in rows))
        for _ in range(2):
            lib.localisation_map_copy(field)
            lib.track_map_copy(field)
            lib.queue_localisation_map(1.0)
            lib.queue_track_map(3)
    lib.localisation_map_reset(None)
    lib.track_map_reset(None)
    # every path was taken: peaks and none, pairs and none, kept tracks and none, samples and none
    assert all(max(v) > 0 and min(v) == 0 for v in seen.values()), seen
    print(json.dumps({"library": lib.LIBRARY_PATH, **{k: v[:len(v) // 2] for k, v in seen.items()}}))


def api_counts(directory):
    """{HIP function: calls} of a rocprofv3 --hip-trace --stats run"""
    counts = {}
    for path in sorted(glob.glob(os.path.join(directory, "**", "*stats*.csv"), recursive=True)):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name, calls = row.get("Name"), row.get("Calls")
                if name and calls and name.startswith("hip"):
                    counts[name] = max(counts.get(name, 0), int(calls))
    assert counts, f"no HIP API statistics under {directory}"
    return counts


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--compare", nargs=2, metavar=("PARENT_DIR", "THIS_DIR"))
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not args.compare:
        run()
        sys.exit(0)
    parent, this = (api_counts(d) for d in args.compare)
    names = sorted(set(parent) | set(this))
    must = [n for n in names if EQUAL.match(n)]
    unequal = [n for n in must if parent.get(n, 0) != this.get(n, 0)]
    others = [n for n in names if n not in must and parent.get(n, 0) != this.get(n, 0)]
    result = {"what": "HIP API call counts of tools/peak_api_calls.py under rocprofv3 --hip-trace --stats, the parent's library and this one's",
              "must_be_equal": {n: [parent.get(n, 0), this.get(n, 0)] for n in must}, "equal": not unequal,
              "others_that_differ": {n: [parent.get(n, 0), this.get(n, 0)] for n in others}, "parent": parent, "this": this}
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({k: result[k] for k in ("must_be_equal", "equal", "others_that_differ")}))
    sys.exit(1 if unequal or not must else 0)
