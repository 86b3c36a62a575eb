"""The host side of the peak pairs and the track map (include/ogl_beamformer_hip.h): the numpy reference (tests/tracks_ref.py) against an
independent formulation and against the properties the definition promises, the sums' fixed point, the layouts of the three records,
and the refusals that are decided before any device state is looked at.  No device is needed; on a machine with one, in a process that
has used it, every case still holds: the cases that need "no map" release the map first (that call always succeeds)."""
import ctypes as C
import os
import subprocess

import numpy as np

from ogl_beamforming_amd import lib as bf
from ogl_beamforming_amd import params as P
from tests import tracks_ref as ref

E = P.LibError
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def by_matrix(ma, mb, max_distance):
    """the pairs from the all-pairs distance matrix: per row and per column the argmin under the key (d2, rank), then mutuality"""
    r2 = float(np.float32(max_distance)) ** 2
    d = mb[None, :, :] - ma[:, None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        d2 = ((d[..., 0] * d[..., 0]) + (d[..., 1] * d[..., 1])) + (d[..., 2] * d[..., 2])
        reach = d2 <= r2

    def best(keys, ok):
        order = np.lexsort((np.arange(len(keys)), keys))             # by d2, ties by rank
        order = [k for k in order if ok[k]]
        return order[0] if order else ref.NONE

    f = [best(d2[a], reach[a]) for a in range(len(ma))]
    g = [best(d2[:, b], reach[:, b]) for b in range(len(mb))]
    return [(a, f[a]) for a in range(len(ma)) if f[a] != ref.NONE and g[f[a]] == a], f, g


def test_the_reference_against_the_distance_matrix():
    rng = np.random.default_rng(9300)
    most = 0
    for case in range(24):
        na, nb = int(rng.integers(0, 40)), int(rng.integers(0, 40))
        # half the cases on a coarse lattice: many exactly equal distances
        draw = (lambda n: rng.integers(0, 6, (n, 3)).astype(np.float64)) if case % 2 else (lambda n: rng.uniform(0.0, 8.0, (n, 3)))
        ma, mb = draw(na), draw(nb)
        if case % 3 == 0 and na:
            ma[rng.integers(0, na)] = np.nan                           # an unplaced peak
        reach = float(rng.uniform(0.5, 4.0))
        linked = ref.link(ma, mb, reach)
        pairs, f, g = by_matrix(ma, mb, reach)
        assert list(zip(linked["a"].tolist(), linked["b"].tolist())) == pairs
        assert linked["f"].tolist() == f and linked["g"].tolist() == g
        # every peak in at most one pair, the list in ascending a, each pair within reach
        assert len(set(linked["a"].tolist())) == len(pairs) == len(set(linked["b"].tolist())) and sorted(linked["a"].tolist()) == linked["a"].tolist()
        assert (linked["distance2"] <= ref.reach2(reach)).all()
        assert np.array_equal(linked["displacement"], mb[linked["b"]] - ma[linked["a"]])
        most = max(most, len(pairs))
    assert most >= 8


def test_reach_is_inclusive_nan_is_unplaced_and_ties_go_to_the_lowest_rank():
    # d2 == R2 is within reach; the next double above is not
    ma, mb = np.array([[0.0, 0.0, 0.0]]), np.array([[3.0, 0.0, 4.0]])
    assert ref.link(ma, mb, 5.0)["a"].tolist() == [0] and ref.link(ma, mb, np.nextafter(np.float32(5.0), np.float32(0.0)))["a"].tolist() == []
    # a NaN placement row: the peak is unplaced, neither a query nor a candidate
    A = np.eye(3, 4)
    A[1, 1] = np.nan
    index, offset = np.array([[1, 2, 3], [4, 5, 6]], np.uint32), np.zeros((2, 3), np.float32)
    assert np.isnan(ref.positions(index, offset, A)).all()
    good = ref.positions(index, offset, np.eye(3, 4))
    assert np.array_equal(good, index.astype(np.float64))
    records, rows = ref.pair_positions([good, np.array([[1.0, 2.0, 3.0], [np.nan] * 3])], 1.0)
    assert rows[0]["unplaced"] == [0, 1] and rows[0]["unpaired"] == [1, 0] and records["a"].tolist() == [0] and records["b"].tolist() == [0]
    # planted ties on integer positions: four candidates at distance 1 of the query, and two queries at distance 1 of one candidate
    centre = np.array([[5.0, 5.0, 5.0]])
    ring = np.array([[5.0, 5.0, 6.0], [6.0, 5.0, 5.0], [5.0, 4.0, 5.0], [4.0, 5.0, 5.0]])
    forward = ref.link(centre, ring, 2.0)
    assert forward["f"].tolist() == [0] and forward["g"].tolist() == [0, 0, 0, 0] and forward["b"].tolist() == [0]
    backward = ref.link(ring, centre, 2.0)
    assert backward["g"].tolist() == [0] and backward["f"].tolist() == [0, 0, 0, 0] and backward["a"].tolist() == [0]
    # a forward choice that is not mutual: b's nearest is another a
    ma, mb = np.array([[0.0, 0.0, 0.0], [3.0, 0.0, 0.0]]), np.array([[2.0, 0.0, 0.0]])
    linked = ref.link(ma, mb, 2.5)
    assert linked["f"].tolist() == [0, 0] and linked["g"].tolist() == [1] and linked["a"].tolist() == [1]


def test_the_fixed_point_of_the_sums_and_their_wrap():
    rng = np.random.default_rng(9301)
    d = np.concatenate([rng.uniform(-1048576.0, 1048576.0, 64), [0.0, -0.0, 0.5 / 1048576.0, -0.5 / 1048576.0, 1048576.0, -1048576.0, 1e-9, -1e-9]])
    q = ref.fixed(d)
    assert q.dtype == np.int64 and np.array_equal(q, np.floor(d * 1048576.0 + 0.5).astype(np.int64))
    assert ref.fixed(0.5 / 1048576.0) == 1 and ref.fixed(-0.5 / 1048576.0) == 0 and ref.fixed(1048576.0) == 1 << 40
    # a deposit: the count and the sums of the midpoint's bin; the sums wrap as int64 does
    counts, sums = ref.empty_map((4, 1, 4))
    ma, mb = np.array([[1.0, 0.0, 1.0]]), np.array([[2.0, 0.0, 1.5]])
    records, rows = ref.pair_positions([ma, mb], 2.0, counts, sums)
    assert rows[0]["deposited"] == 1 and records["deposited"].tolist() == [1] and counts[1, 0, 2] == 1 and int(counts.sum()) == 1      # floor(1.5 + 0.5), floor(1.25 + 0.5)
    assert sums[:, 1, 0, 2].tolist() == [1 << 20, 0, 1 << 19]
    sums[0, 1, 0, 2] = np.iinfo(np.int64).max
    ref.pair_positions([ma, mb], 2.0, counts, sums)
    assert sums[0, 1, 0, 2] == np.iinfo(np.int64).min + (1 << 20) - 1 and counts[1, 0, 2] == 2
    # a midpoint outside: counted, nothing written
    before = counts.copy(), sums.copy()
    records, rows = ref.pair_positions([ma + 10.0, mb + 10.0], 2.0, counts, sums)
    assert rows[0]["outside"] == 1 and rows[0]["deposited"] == 0 and records["deposited"].tolist() == [0]
    assert np.array_equal(counts, before[0]) and np.array_equal(sums, before[1])
    # the queued components
    frame = ref.queued_frame(counts, sums, 2, 3.0, min_pairs=2)
    assert frame[1, 0, 2] == np.float32(np.float64(sums[2, 1, 0, 2]) / 1048576.0 / 2.0) * np.float32(3.0) and np.count_nonzero(frame) == 1
    assert not ref.queued_frame(counts, sums, 2, 3.0, min_pairs=3).any() and ref.queued_frame(counts, sums, 3, 0.5)[1, 0, 2] == 1.0


def test_the_records_have_the_headers_layout(tmp_path):
    assert C.sizeof(P.HipPeakPair) == 48 and C.sizeof(P.HipPeakPairs) == 72 and C.sizeof(P.HipTrackMapInfo) == 40
    assert np.dtype(P.HipPeakPair).itemsize == ref.PAIR.itemsize and [np.dtype(P.HipPeakPair).fields[n][1] for n in ref.PAIR.names] == [ref.PAIR.fields[n][1] for n in ref.PAIR.names]
    fields = {"BeamformerHipPeakPair": P.HipPeakPair, "BeamformerHipPeakPairs": P.HipPeakPairs, "BeamformerHipTrackMapInfo": P.HipTrackMapInfo}
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "ogl_beamformer_hip.h"', "int main(void) {",
             '  printf("voxels %llu\\n", (unsigned long long)BEAMFORMER_HIP_MAX_TRACK_MAP_VOXELS);',
             '  printf("distance %.1f\\n", (double)BEAMFORMER_HIP_MAX_PAIR_DISTANCE);',
             '  printf("components %u\\n", (unsigned)BEAMFORMER_HIP_TRACK_MAP_COMPONENTS);']
    for struct, cls in fields.items():
        lines.append(f'  printf("{struct} %zu\\n", sizeof({struct}));')
        lines += [f'  printf("{struct}.{name} %zu\\n", offsetof({struct}, {name}));' for name, _ in cls._fields_]
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    said = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(said["voxels"]) == P.HIP_MAX_TRACK_MAP_VOXELS == 1 << 26 and float(said["distance"]) == P.HIP_MAX_PAIR_DISTANCE == 1048576.0
    assert int(said["components"]) == P.HIP_TRACK_MAP_COMPONENTS == 5
    for struct, cls in fields.items():
        assert int(said[struct]) == C.sizeof(cls)
        for name, kind in cls._fields_:
            assert int(said[f"{struct}.{name}"]) == getattr(cls, name).offset, (struct, name)
        # no padding: the fields fill the struct
        assert sum(C.sizeof(kind) for _, kind in cls._fields_) == C.sizeof(cls)


def test_refusals_that_need_no_device():
    L = bf.library()
    for points, kind in (((0, 4, 4), E.InvalidAccess), ((4, 4, 0), E.InvalidAccess), ((1 << 13, 1 << 13, 2), E.BufferOverflow),
                         ((0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), E.BufferOverflow), ((1 << 16, 1 << 16, 1 << 16), E.BufferOverflow)):
        assert not L.beamformer_hip_track_map_reset((C.c_uint32 * 3)(*points))
        assert bf.last_error()[0] == kind, points
    assert L.beamformer_hip_track_map_reset(None)                        # releasing a map that is not there succeeds

    rows = (P.HipPeakPairs * 4)()
    pairs = (P.HipPeakPair * 64)()
    C.memset(rows, 0xA5, C.sizeof(rows))
    C.memset(pairs, 0xA5, C.sizeof(pairs))
    untouched = bytes(rows), bytes(pairs)
    total, ms = C.c_uint32(77), C.c_float(-1.0)
    level, identity = (C.c_float * 4)(0.0, 0.0, 0.0, 0.0), np.tile(np.eye(3, 4).reshape(-1), 4)

    def refused(kind, count=3, thresholds=level, threshold_count=1, placements=identity, placement_count=1, reach=2.0, cap=16, deposit=0,
                out_rows=rows, out_total=C.byref(total)):
        pointer = None if placements is None else np.ascontiguousarray(placements, np.float64).ctypes.data_as(C.POINTER(C.c_double))
        assert not L.beamformer_hip_pair_peaks_last_frames(count, None, thresholds, threshold_count, pointer, placement_count, 1, reach, cap, deposit,
                                                           out_rows, pairs, out_total, C.byref(ms))
        assert bf.last_error()[0] == kind and (bytes(rows), bytes(pairs)) == untouched and total.value == 77 and ms.value == -1.0

    for count in (0, 1, P.HIP_MAX_SCORED_FRAMES + 1):
        refused(E.BufferOverflow, count=count)
    refused(E.BufferOverflow, cap=0)
    refused(E.BufferOverflow, cap=P.HIP_MAX_PEAKS_PER_FRAME + 1)
    refused(E.InvalidAccess, out_rows=None)
    refused(E.InvalidAccess, out_total=None)
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
    refused(E.InvalidAccess, deposit=1)                                  # no track map: it was released above

    counts, sums, info = (C.c_uint32 * 4)(9, 9, 9, 9), (C.c_int64 * 12)(*([9] * 12)), P.HipTrackMapInfo()
    C.memset(C.byref(info), 0x5A, C.sizeof(info))
    assert not L.beamformer_hip_track_map_copy(None, sums, 4, C.byref(info)) and bf.last_error()[0] == E.InvalidAccess
    assert not L.beamformer_hip_track_map_copy(counts, None, 4, C.byref(info)) and bf.last_error()[0] == E.InvalidAccess
    assert not L.beamformer_hip_track_map_copy(counts, sums, 4, C.byref(info)) and bf.last_error()[0] == E.InvalidAccess      # no map
    assert list(counts) == [9] * 4 and list(sums) == [9] * 12 and bytes(info) == b"\x5A" * C.sizeof(info)

    frame = C.c_uint32(77)
    for component, scale in ((0, float("nan")), (3, float("inf")), (4, -float("inf")), (5, 1.0), (0xFFFFFFFF, 1.0), (0, 1.0)):       # the last: no map
        assert not L.beamformer_hip_queue_track_map(component, scale, 1, 0, C.byref(frame), C.byref(ms))
        assert bf.last_error()[0] == E.InvalidAccess and frame.value == 77 and ms.value == -1.0
