"""The host side of the peak tracks (beamformer_hip_track_peaks_last_frames, include/ogl_beamformer_hip.h): the numpy reference
(tests/track_chains_ref.py) against an independent formulation -- union-find over the pair records, then a sort --, the layouts of the
three records, the refusals that are decided before any device state is looked at, and the planted plans of
tests/test_gpu_track_chains.py, checked here for what they claim.  No device is needed.  Every comparison is of integers or bit
patterns."""
import ctypes as C
import os
import subprocess

import numpy as np

from ogl_beamforming_amd import lib as bf
from ogl_beamforming_amd import params as P
from tests import frame_peaks_ref, tracks_ref
from tests import track_chains_ref as ref
from tests.track_plans import HEIGHT, IDENTITY, LEVEL, REACH, ROOT, coordinates_of, plane_plan, teeth, volume_plan

E = P.LibError


# ----------------------------------------------------------------------------- the planted plans


def test_the_plane_plan_is_what_it_claims():
    stack, spots = plane_plan()
    for k, where in spots.items():                                    # isolated: at least 2 voxels from any other
        assert all(max(abs(a[0] - b[0]), abs(a[1] - b[1])) >= 2 for n, a in enumerate(where) for b in where[n + 1:])
        assert frame_peaks_ref.peaks(stack[k], LEVEL)["found"] == len(where) == int((stack[k] == HEIGHT).sum())
    coordinates = coordinates_of(stack, IDENTITY)
    everything = ref.chain_positions(coordinates, REACH, 1)
    assert sorted(everything["lengths"]) == [1, 1, 2, 3, 5, 6, 8, 9, 11]
    assert len(everything["pairs"]) == 37 and ref.one_sided(everything["pair_rows"]) == 1
    assert len(everything["tracks"]) == 9 and len(everything["points"]) == 46
    for min_length in (3, 9):
        teeth(ref.chain_positions(coordinates, REACH, min_length), min_length, len(stack))
    assert len(ref.chain_positions(coordinates, REACH, 12)["tracks"]) == 0
    # lengths 8, 9 and 11 straddle the jump rounds 2^3 .. 2^4
    assert {8, 9, 11} <= set(everything["lengths"])


def test_the_volume_plan_is_what_it_claims():
    stack, placements = volume_plan()
    coordinates = coordinates_of(stack, placements)
    assert all(len(m) > 512 for m in coordinates)
    out = ref.chain_positions(coordinates, 1.0, 3)
    firsts = np.concatenate([[0], np.cumsum([len(m) for m in coordinates])])
    assert len(out["tracks"]) > 256 and set(out["lengths"]) >= {1, 2, 3, 4, 5}
    blocks = 0
    for t in out["tracks"]:
        run = out["points"][int(t["first"]):int(t["first"]) + int(t["length"])]
        index = firsts[run["frame"]] + run["rank"]
        assert (index[1:] >> 8 != index[:-1] >> 8).all()              # a point and its successor lie in different blocks of 256 records
        blocks = max(blocks, int(index[0]) >> 8)
    assert blocks >= 2 and int(out["tracks"]["first"][-1]) >> 8 >= 4   # kept heads, and the points before them, in several blocks


# ----------------------------------------------------------------------------- the reference against union-find

def by_union_find(coordinates, max_distance, min_length):
    """the kept tracks from the pair records alone: union-find over (frame, rank), every placed peak a set; a set sorted by frame is a
    track, the sets sorted by their first member are the list"""
    records, _ = tracks_ref.pair_positions(coordinates, max_distance)
    parent = {(n, k): (n, k) for n, m in enumerate(coordinates) for k in range(len(m)) if not np.isnan(m[k, 0])}

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v
    for r in records:
        parent[find((int(r["frame"]), int(r["a"])))] = find((int(r["frame"]) + 1, int(r["b"])))
    sets = {}
    for v in parent:
        sets.setdefault(find(v), []).append(v)
    return sorted(sorted(s) for s in sets.values() if len(s) >= min_length)


def test_the_reference_against_union_find():
    rng = np.random.default_rng(9700)
    longest = 0
    for case in range(16):
        K = int(rng.integers(2, 9))
        # peaks that drift slowly on a coarse lattice: chains, equal distances, births and deaths
        base = rng.integers(0, 12, (int(rng.integers(4, 30)), 3)).astype(np.float64)
        coordinates = []
        for n in range(K):
            here = base + n * np.array([0.5, 0.0, 0.25])
            here = here[rng.random(len(here)) < 0.85]
            if case % 3 == 0 and len(here):
                here[rng.integers(0, len(here))] = np.nan              # an unplaced peak
            coordinates.append(here[np.argsort(rng.random(len(here)))])
        for min_length in (1, 2, 3):
            out = ref.chain_positions(coordinates, 0.75, min_length)
            want = by_union_find(coordinates, 0.75, min_length)
            got = [[(int(p["frame"]), int(p["rank"])) for p in out["points"][int(t["first"]):int(t["first"]) + int(t["length"])]] for t in out["tracks"]]
            assert got == want
            # one peak a frame in consecutive frames, the records say what the runs say, every placed peak in exactly one track
            for t, run in zip(out["tracks"], got):
                assert [n for n, _ in run] == list(range(run[0][0], run[0][0] + len(run))) and (int(t["frame"]), int(t["rank"])) == run[0]
                assert int(t["flags"]) == (1 if run[0][0] == 0 else 0) | (2 if run[-1][0] == K - 1 else 0)
                assert np.array_equal(t["displacement"], coordinates[run[-1][0]][run[-1][1]] - coordinates[run[0][0]][run[0][1]])
            assert (out["points"]["track"] == np.repeat(np.arange(len(got)), [len(r) for r in got])).all()
            longest = max(longest, max(out["lengths"], default=0))
        placed = sum(int((~np.isnan(m[:, 0])).sum()) for m in coordinates)
        everything = ref.chain_positions(coordinates, 0.75, 1)
        assert len(everything["points"]) == placed == sum(everything["lengths"])
        rows = everything["rows"]
        assert sum(r["heads"] for r in rows) == len(everything["tracks"]) and sum(r["kept_links"] for r in rows) == len(everything["pairs"])
        # (iii): the links of all tracks are the pair call's records
        assert ref.links_as_pairs(everything) == [(int(r["frame"]), int(r["a"]), int(r["b"])) for r in everything["pairs"]]
    assert longest >= 5


def test_the_deposits_of_the_reference():
    stack, _ = plane_plan()
    coordinates = coordinates_of(stack, IDENTITY)
    field = (20, 1, 40)                                               # the spots at x = 20, 21 and 22 lie outside
    shape = field[::-1]
    # (i): with min_length <= 2 the links are the pair call's deposits
    for min_length in (1, 2):
        counts, sums = tracks_ref.empty_map(field)
        out = ref.chain_positions(coordinates, REACH, min_length, ref.LINKS, counts=counts, sums=sums)
        pair_counts, pair_sums = tracks_ref.empty_map(field)
        _, pair_rows = tracks_ref.pair_positions(coordinates, REACH, pair_counts, pair_sums)
        assert counts.tobytes() == pair_counts.tobytes() and sums.tobytes() == pair_sums.tobytes() and int(counts.sum()) == 35
        assert [r["links_deposited"] for r in out["rows"]][:-1] == [w["deposited"] for w in pair_rows]
        assert sum(r["links_outside"] for r in out["rows"]) == 2
    # (ii): with min_length 1 the points are the localisation map's deposits
    density = np.zeros(shape, np.uint32)
    out = ref.chain_positions(coordinates, REACH, 1, ref.POINTS, point_map=density)
    assert int(density.sum()) == 46 - 4 == sum(r["points_deposited"] for r in out["rows"]) and sum(r["points_outside"] for r in out["rows"]) == 4
    assert density[30, 0, 14] == 1 and density[20, 0, 6] == 8
    # kept by length: the lone spot and the short tracks are gone, in both maps
    density = np.zeros(shape, np.uint32)
    counts, sums = tracks_ref.empty_map(field)
    out = ref.chain_positions(coordinates, REACH, 5, ref.POINTS | ref.LINKS, point_map=density, counts=counts, sums=sums)
    assert sorted(out["tracks"]["length"].tolist()) == [5, 6, 8, 9, 11] and int(density.sum()) == 39 and int(counts.sum()) == 34
    assert density[30, 0, 14] == 0 and (out["points"]["deposited"] & 1).all()
    assert int((out["points"]["deposited"] >> 1).sum()) == 34


# ----------------------------------------------------------------------------- the records and the refusals

def test_the_records_have_the_headers_layout(tmp_path):
    assert C.sizeof(P.HipPeakTrack) == 48 and C.sizeof(P.HipTrackPoint) == 40 and C.sizeof(P.HipTrackedFrame) == 56
    for cls, dtype in ((P.HipPeakTrack, ref.TRACK), (P.HipTrackPoint, ref.POINT)):
        assert np.dtype(cls).itemsize == dtype.itemsize and [np.dtype(cls).fields[n][1] for n in dtype.names] == [dtype.fields[n][1] for n in dtype.names]
    fields = {"BeamformerHipPeakTrack": P.HipPeakTrack, "BeamformerHipTrackPoint": P.HipTrackPoint, "BeamformerHipTrackedFrame": P.HipTrackedFrame}
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "ogl_beamformer_hip.h"', "int main(void) {",
             '  printf("points %u\\n", (unsigned)BEAMFORMER_HIP_TRACK_DEPOSIT_POINTS);',
             '  printf("links %u\\n", (unsigned)BEAMFORMER_HIP_TRACK_DEPOSIT_LINKS);']
    for struct, cls in fields.items():
        lines.append(f'  printf("{struct} %zu\\n", sizeof({struct}));')
        lines += [f'  printf("{struct}.{name} %zu\\n", offsetof({struct}, {name}));' for name, _ in cls._fields_]
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    said = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(said["points"]) == P.HIP_TRACK_DEPOSIT_POINTS == ref.POINTS == 1 and int(said["links"]) == P.HIP_TRACK_DEPOSIT_LINKS == ref.LINKS == 2
    for struct, cls in fields.items():
        assert int(said[struct]) == C.sizeof(cls)
        for name, kind in cls._fields_:
            assert int(said[f"{struct}.{name}"]) == getattr(cls, name).offset, (struct, name)
        assert sum(C.sizeof(kind) for _, kind in cls._fields_) == C.sizeof(cls)              # no padding: the fields fill the struct
    # the rows' counters are the kernels' tally, in its order
    assert [name for name, _ in P.HipTrackedFrame._fields_][4:12] == list(ref.COUNTERS)


def test_refusals_that_need_no_device():
    L = bf.library()
    assert L.beamformer_hip_track_map_reset(None) and L.beamformer_hip_localisation_map_reset(None)
    rows, tracks, points = (P.HipTrackedFrame * 4)(), (P.HipPeakTrack * 64)(), (P.HipTrackPoint * 64)()
    for out in (rows, tracks, points):
        C.memset(out, 0xA5, C.sizeof(out))
    untouched = bytes(rows), bytes(tracks), bytes(points)
    track_total, point_total, ms = C.c_uint32(77), C.c_uint32(78), C.c_float(-1.0)
    level, identity = (C.c_float * 4)(0.0, 0.0, 0.0, 0.0), np.tile(np.eye(3, 4).reshape(-1), 4)

    def refused(kind, count=3, thresholds=level, threshold_count=1, placements=identity, placement_count=1, reach=2.0, cap=16, min_length=2,
                deposit=0, out_rows=rows, out_tracks=C.byref(track_total), out_points=C.byref(point_total)):
        pointer = None if placements is None else np.ascontiguousarray(placements, np.float64).ctypes.data_as(C.POINTER(C.c_double))
        assert not L.beamformer_hip_track_peaks_last_frames(count, None, thresholds, threshold_count, pointer, placement_count, 1, reach, cap,
                                                            min_length, deposit, out_rows, tracks, points, out_tracks, out_points, C.byref(ms))
        assert bf.last_error()[0] == kind and (bytes(rows), bytes(tracks), bytes(points)) == untouched
        assert (track_total.value, point_total.value, ms.value) == (77, 78, -1.0)

    # everything the pair call refuses, with its error kinds
    for count in (0, 1, P.HIP_MAX_SCORED_FRAMES + 1):
        refused(E.BufferOverflow, count=count)
    refused(E.BufferOverflow, cap=0)
    refused(E.BufferOverflow, cap=P.HIP_MAX_PEAKS_PER_FRAME + 1)
    refused(E.InvalidAccess, thresholds=None)
    refused(E.InvalidAccess, placements=None)
    refused(E.InvalidAccess, threshold_count=2)
    refused(E.InvalidAccess, placement_count=2)
    refused(E.InvalidAccess, placement_count=0)
    refused(E.InvalidAccess, thresholds=(C.c_float * 1)(-1.0))
    refused(E.InvalidAccess, thresholds=(C.c_float * 1)(float("nan")))
    for bad in (float("nan"), float("inf"), -float("inf")):
        broken = identity.copy()
        broken[12 * 2 + 7] = bad                                         # in the third of three placements
        refused(E.InvalidAccess, placements=broken, placement_count=3)
        refused(E.InvalidAccess, reach=bad)
    refused(E.InvalidAccess, reach=-1.0)
    refused(E.InvalidAccess, reach=float(np.nextafter(np.float32(1048576.0), np.float32(np.inf))))
    # the call's own
    refused(E.BufferOverflow, min_length=0)
    refused(E.BufferOverflow, min_length=P.HIP_MAX_SCORED_FRAMES + 1)
    for deposit in (4, 7, 0x80000000, 0xFFFFFFFF):
        refused(E.InvalidAccess, deposit=deposit)
    refused(E.InvalidAccess, out_rows=None)
    refused(E.InvalidAccess, out_tracks=None)
    refused(E.InvalidAccess, out_points=None)
    for deposit in (1, 2, 3):
        refused(E.InvalidAccess, deposit=deposit)                        # no maps: both were released above
