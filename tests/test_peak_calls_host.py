"""The order in which the five peak calls (find_peaks, accumulate_peaks, pair_peaks, track_peaks, draw_tracks) and the two map resets
refuse their arguments (include/ogl_beamformer_hip.h).  The host tests of each call give it one bad argument at a time; with two bad
arguments at once it is the ORDER of the checks that decides which error kind the caller sees, and that order is part of what a caller
can observe.  Every call here gets every pair of the faults its own test file uses; the kind it answers with is compared against a
table recorded from the library as it was before the calls shared one checker (BUFFER_OVERFLOW below: every other pair is refused with
InvalidAccess).  A refused call leaves its outputs and device_ms alone.  No device is needed, and none is started."""
import ctypes as C
import itertools

import numpy as np
import pytest

from ogl_beamforming_amd import lib as bf
from ogl_beamforming_amd import params as P

E = P.LibError
LEVEL = (C.c_float * 4)(0.0, 0.0, 0.0, 0.0)
IDENTITY = np.tile(np.eye(3, 4).reshape(-1), 4)
BROKEN = IDENTITY.copy()
BROKEN[12 * 2 + 7] = float("inf")                                      # in the third of three placements
GOOD = dict(count=3, thresholds=LEVEL, threshold_count=1, placements=IDENTITY, placement_count=1, reach=2.0, cap=16, min_length=2, smooth=1,
            deposit=0)

# a fault: the arguments it replaces.  The lists are those of the calls' own test files (test_refusals_that_need_no_device)
FAULTS = {
    "count": dict(count=0),
    "cap": dict(cap=0),
    "min_length": dict(min_length=0),
    "thresholds null": dict(thresholds=None),
    "placements null": dict(placements=None),
    "threshold_count": dict(threshold_count=2),
    "placement_count": dict(placement_count=2),
    "threshold NaN": dict(thresholds=(C.c_float * 1)(float("nan"))),
    "placement inf": dict(placements=BROKEN, placement_count=3),
    "reach": dict(reach=-1.0),
    "deposit bits": dict(deposit=4),
    "smooth": dict(smooth=P.HIP_MAX_TRACK_SMOOTH + 1),
}


class Outputs:
    """a call's output arrays, filled with a pattern, and its counts, preset; `null` names the one passed as NULL"""

    def __init__(self, arrays, totals):
        self.arrays = {name: (kind * n)() for name, (kind, n) in arrays.items()}
        for a in self.arrays.values():
            C.memset(a, 0xA5, C.sizeof(a))
        self.totals = {name: C.c_uint32(77 + k) for k, name in enumerate(totals)}
        self.ms = C.c_float(-1.0)
        self.before = self.state()

    def state(self):
        return [bytes(a) for a in self.arrays.values()], [t.value for t in self.totals.values()], self.ms.value

    def of(self, name, null):
        if name == null:
            return None
        return self.arrays[name] if name in self.arrays else C.byref(self.totals[name])


def pointer(placements):
    return None if placements is None else np.ascontiguousarray(placements, np.float64).ctypes.data_as(C.POINTER(C.c_double))


def find(L, a, o, null):
    return L.beamformer_hip_find_peaks_last_frames(a["count"], None, a["thresholds"], a["threshold_count"], a["cap"], o.of("rows", null),
                                                   o.of("peaks", null), o.of("total", null), C.byref(o.ms))


def accumulate(L, a, o, null):
    return L.beamformer_hip_accumulate_peaks_last_frames(a["count"], None, a["thresholds"], a["threshold_count"], pointer(a["placements"]),
                                                         a["placement_count"], 1, o.of("rows", null), C.byref(o.ms))


def pair(L, a, o, null):
    return L.beamformer_hip_pair_peaks_last_frames(a["count"], None, a["thresholds"], a["threshold_count"], pointer(a["placements"]),
                                                   a["placement_count"], 1, a["reach"], a["cap"], a["deposit"], o.of("rows", null),
                                                   o.of("pairs", null), o.of("total", null), C.byref(o.ms))


def track(L, a, o, null):
    return L.beamformer_hip_track_peaks_last_frames(a["count"], None, a["thresholds"], a["threshold_count"], pointer(a["placements"]),
                                                    a["placement_count"], 1, a["reach"], a["cap"], a["min_length"], a["deposit"],
                                                    o.of("rows", null), o.of("tracks", null), o.of("points", null), o.of("track_total", null),
                                                    o.of("point_total", null), C.byref(o.ms))


def draw(L, a, o, null):
    return L.beamformer_hip_draw_tracks_last_frames(a["count"], None, a["thresholds"], a["threshold_count"], pointer(a["placements"]),
                                                    a["placement_count"], 1, a["reach"], a["cap"], a["min_length"], a["smooth"], a["deposit"],
                                                    o.of("rows", null), C.byref(o.ms))


# call: (the function, its faults by name, its output arrays, its counts, the outputs whose NULL is a fault)
CALLS = {
    "find": (find, ("count", "cap", "thresholds null", "threshold_count", "threshold NaN"),
             dict(rows=(P.HipFramePeaks, 4), peaks=(P.HipFramePeak, 64)), ("total",), ("rows", "peaks", "total")),
    "accumulate": (accumulate, ("count", "thresholds null", "placements null", "threshold_count", "placement_count", "threshold NaN", "placement inf"),
                   dict(rows=(P.HipMapDeposits, 4)), (), ()),
    "pair": (pair, ("count", "cap", "thresholds null", "placements null", "threshold_count", "placement_count", "threshold NaN", "placement inf",
                    "reach"), dict(rows=(P.HipPeakPairs, 4), pairs=(P.HipPeakPair, 64)), ("total",), ("rows", "total")),
    "track": (track, ("count", "cap", "min_length", "thresholds null", "placements null", "threshold_count", "placement_count", "threshold NaN",
                      "placement inf", "reach", "deposit bits"),
              dict(rows=(P.HipTrackedFrame, 4), tracks=(P.HipPeakTrack, 64), points=(P.HipTrackPoint, 64)), ("track_total", "point_total"),
              ("rows", "track_total", "point_total")),
    "draw": (draw, ("count", "cap", "min_length", "thresholds null", "placements null", "threshold_count", "placement_count", "threshold NaN",
                    "placement inf", "reach", "deposit bits", "smooth"), dict(rows=(P.HipDrawnFrame, 4)), (), ("rows",)),
}


def faults_of(name):
    """the call's faults: (label, replaced arguments, the output passed as NULL)"""
    run, names, arrays, totals, nullable = CALLS[name]
    return [(n, FAULTS[n], None) for n in names] + [(f"{n} null", {}, n) for n in nullable]


def refusal(name, replaced, null=None):
    """the call with `replaced` arguments: refused, its outputs untouched; the error kind's name"""
    run, names, arrays, totals, nullable = CALLS[name]
    L = bf.library()
    o = Outputs(arrays, totals)
    assert not run(L, dict(GOOD, **replaced), o, null)
    kind = bf.last_error()[0]
    assert o.state() == o.before, (name, replaced)
    return E(kind).name


def pairs_refused_with(name, wanted):
    found = []
    for (a, first, null_a), (b, second, null_b) in itertools.combinations(faults_of(name), 2):
        if null_a and null_b:
            continue                                                   # one NULL output a call
        if refusal(name, dict(first, **second), null_a or null_b) == wanted:
            found.append(f"{a} + {b}")
    return found


# recorded from the library of the commit before the shared checker, selected with OGL_BEAMFORMER_LIB; not produced by the code under test
PAIRS = {"find": 25, "accumulate": 21, "pair": 54, "track": 88, "draw": 78}
BUFFER_OVERFLOW = {
    "find": ["count + cap", "count + thresholds null", "count + threshold_count", "count + threshold NaN", "count + rows null", "count + peaks null",
             "count + total null", "cap + thresholds null", "cap + threshold_count", "cap + threshold NaN", "cap + rows null", "cap + peaks null",
             "cap + total null"],
    "accumulate": ["count + thresholds null", "count + placements null", "count + threshold_count", "count + placement_count",
                   "count + threshold NaN", "count + placement inf"],
    "pair": ["count + cap", "count + thresholds null", "count + placements null", "count + threshold_count", "count + placement_count",
             "count + threshold NaN", "count + placement inf", "count + reach", "count + rows null", "count + total null", "cap + thresholds null",
             "cap + placements null", "cap + threshold_count", "cap + placement_count", "cap + threshold NaN", "cap + placement inf", "cap + reach",
             "cap + rows null", "cap + total null"],
    "track": ["count + cap", "count + min_length", "count + thresholds null", "count + placements null", "count + threshold_count",
              "count + placement_count", "count + threshold NaN", "count + placement inf", "count + reach", "count + deposit bits",
              "count + rows null", "count + track_total null", "count + point_total null", "cap + min_length", "cap + thresholds null",
              "cap + placements null", "cap + threshold_count", "cap + placement_count", "cap + threshold NaN", "cap + placement inf", "cap + reach",
              "cap + deposit bits", "cap + rows null", "cap + track_total null", "cap + point_total null", "min_length + thresholds null",
              "min_length + placements null", "min_length + threshold_count", "min_length + placement_count", "min_length + threshold NaN",
              "min_length + placement inf", "min_length + reach", "min_length + deposit bits", "min_length + rows null",
              "min_length + track_total null", "min_length + point_total null"],
    "draw": ["count + cap", "count + min_length", "count + thresholds null", "count + placements null", "count + threshold_count",
             "count + placement_count", "count + threshold NaN", "count + placement inf", "count + reach", "count + deposit bits", "count + smooth",
             "count + rows null", "cap + min_length", "cap + thresholds null", "cap + placements null", "cap + threshold_count",
             "cap + placement_count", "cap + threshold NaN", "cap + placement inf", "cap + reach", "cap + deposit bits", "cap + smooth",
             "cap + rows null", "min_length + thresholds null", "min_length + placements null", "min_length + threshold_count",
             "min_length + placement_count", "min_length + threshold NaN", "min_length + placement inf", "min_length + reach",
             "min_length + deposit bits", "min_length + smooth", "min_length + rows null"],
}
# both faults in one grid -- an extent of 0, and a plane or a volume over either map's voxel limit --, recorded likewise
RESETS = (((1 << 15, 1 << 15, 0), "InvalidAccess"), ((0, 1 << 15, 1 << 15), "InvalidAccess"), ((0xFFFFFFFF, 0xFFFFFFFF, 0), "InvalidAccess"),
          ((1 << 16, 0, 1 << 16), "InvalidAccess"))


@pytest.mark.parametrize("name", list(CALLS))
def test_every_pair_of_faults_is_refused_with_the_recorded_kind(name):
    assert L_has_no_maps()
    overflow = pairs_refused_with(name, "BufferOverflow")
    invalid = pairs_refused_with(name, "InvalidAccess")
    assert len(overflow) + len(invalid) == PAIRS[name]
    assert overflow == BUFFER_OVERFLOW[name]
    # one fault at a time, as the calls' own files have it, and none: no device is in use, so there is no frame
    for label, replaced, null in faults_of(name):
        assert refusal(name, replaced, null) == ("BufferOverflow" if label in ("count", "cap", "min_length", "smooth") else "InvalidAccess"), label
    assert refusal(name, {}) == "InvalidAccess"


def L_has_no_maps():
    L = bf.library()
    return L.beamformer_hip_track_map_reset(None) and L.beamformer_hip_localisation_map_reset(None)


def test_the_resets_judge_a_missing_extent_before_the_voxel_limit():
    L = bf.library()
    for reset in (L.beamformer_hip_localisation_map_reset, L.beamformer_hip_track_map_reset):
        for points, kind in RESETS:
            assert not reset((C.c_uint32 * 3)(*points)) and E(bf.last_error()[0]).name == kind, points
