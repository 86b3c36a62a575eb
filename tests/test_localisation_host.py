"""The host side of the localisation map (include/ogl_beamformer_hip.h): beamformer_hip_map_placement against its numpy restatement
(tests/localisation_ref.py), its round trip with beamformer_hip_peaks_to_views, the refusals that are decided before any device state
is looked at, and the layouts of the two records.  No device is needed; on a machine with one, in a process that has used it, every
case still holds: the cases that need "no map" release the map first (that call always succeeds)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from ogl_beamforming_amd import configs as cfg
from ogl_beamforming_amd import lib as bf
from ogl_beamforming_amd import params as P
from tests import localisation_ref as ref

E = P.LibError
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LO, HI = (-12e-3, -4e-3, 5e-3), (12e-3, 4e-3, 45e-3)
SOURCE, FINE = (32, 8, 48), (125, 29, 189)              # the map: 4 x finer an axis over the same box


def regular_transform(rng):
    """a column-major float32 voxel transform: a rotation times extents of 5 .. 25 mm, an origin within 30 mm"""
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    m = np.zeros((4, 4))
    m[:3, :3] = q @ np.diag(rng.uniform(5e-3, 25e-3, 3))
    m[:3, 3] = rng.uniform(-30e-3, 30e-3, 3)
    m[3, 3] = 1.0
    return m.T.reshape(-1).astype(np.float32)


def test_map_placement_against_numpy():
    rng = np.random.default_rng(9100)
    worst = 0.0
    for case in range(16):
        frame, grid = regular_transform(rng), regular_transform(rng)
        frame_points = [int(v) for v in rng.integers(1, 200, 3)]
        map_points = [int(v) for v in rng.integers(1, 800, 3)]
        if case == 0:
            frame_points, map_points = [1, 1, 1], [1, 1, 1]          # max(1, P - 1) on every axis
        got = bf.map_placement(frame, frame_points, grid, map_points)
        expected = ref.map_placement(frame, frame_points, grid, map_points)
        error = np.abs(got - expected).max() / np.abs(expected).max()
        worst = max(worst, error)
        assert error <= 1e-12, (case, error)
    print(f"  map_placement: worst error {worst:.3e} of the largest entry (bar 1e-12)")
    # the grids of the tests: axis-aligned boxes, a map 4 x finer -- 4 on the diagonal, nothing else
    a, b = cfg.das_transform_3d(LO, HI), cfg.das_transform_3d(LO, HI)
    got = bf.map_placement(a, SOURCE, b, FINE)
    assert np.allclose(got, np.concatenate([np.diag([4.0, 4.0, 4.0]), np.zeros((3, 1))], axis=1), rtol=0, atol=1e-12)


def test_round_trip_with_peaks_to_views():
    """the view peaks_to_views makes for a peak is a patch centred on it: the patch's centre voxel, placed with the VIEW's placement,
    lands where the peak itself lands under the source grid's placement.  The view's transform is float32: each of its entries is off by
    at most 2^-24 of its magnitude, the translation's magnitude at most W = the largest world coordinate of the box (45 mm), the
    columns' (times the centre's normalised coordinate 1/2) less than that; four such terms a row, divided by the map's smallest pitch:
    the bar is 4 x 2^-24 x W / pitch map voxels."""
    source = cfg.das_transform_3d(LO, HI)
    rng = np.random.default_rng(9101)
    peaks = []
    for _ in range(12):
        index = [int(rng.integers(0, n)) for n in SOURCE]
        peaks.append(P.HipFramePeak((C.c_uint32 * 3)(*index), 1.0, (C.c_float * 3)(*rng.uniform(-0.5, 0.5, 3).astype(np.float32)), 7))
    patch, extent = (17, 5, 17), (4.0, 2.0, 4.0)
    pitch = min((HI[a] - LO[a]) / (FINE[a] - 1) for a in range(3))
    bar = 4 * 2.0 ** -24 * max(abs(v) for v in LO + HI) / pitch
    whole = bf.map_placement(source, SOURCE, source, FINE)
    for use_offsets in (True, False):
        views = bf.peaks_to_views(source, SOURCE, peaks, patch, extent, use_offsets=use_offsets)
        worst = 0.0
        for p, v in zip(peaks, views):
            at = np.array(p.index, np.float64) + (np.array(p.offset, np.float32).astype(np.float64) if use_offsets else 0.0)
            expected = whole[:, :3] @ at + whole[:, 3]
            mine = bf.map_placement(list(v.das_voxel_transform), patch, source, FINE)
            centre = np.array([(n - 1) / 2 for n in patch])
            got = mine[:, :3] @ centre + mine[:, 3]
            worst = max(worst, np.abs(got - expected).max())
        print(f"  round trip, offsets {use_offsets}: worst {worst:.3e} map voxels (bar {bar:.3e})")
        assert worst <= bar


def placement_refused(frame, frame_points, grid, map_points):
    out = (C.c_double * 12)(*([7.0] * 12))
    arrays = [None if frame is None else (C.c_float * 16)(*frame), None if frame_points is None else (C.c_uint32 * 3)(*frame_points),
              None if grid is None else (C.c_float * 16)(*grid), None if map_points is None else (C.c_uint32 * 3)(*map_points)]
    assert not bf.library().beamformer_hip_map_placement(*arrays, out)
    assert bf.last_error()[0] == E.InvalidAccess and list(out) == [7.0] * 12


def test_singular_transforms_and_zero_extents_are_refused():
    good = [float(v) for v in cfg.das_transform_3d(LO, HI)]
    flat = [float(v) for v in cfg.das_transform_3d(LO, (HI[0], LO[1], HI[2]))]          # a plane's: no extent along y
    twin = list(good)
    twin[4:8] = twin[0:4]                                                               # two equal columns
    skew = list(good)
    skew[4:7] = [good[0] * 0.5, 0.0, good[10] * 0.25]                                   # column y in the plane of x and z
    placement_refused(good, SOURCE, flat, FINE)
    placement_refused(good, SOURCE, twin, FINE)
    placement_refused(good, SOURCE, skew, FINE)
    placement_refused(good, SOURCE, [0.0] * 16, FINE)
    placement_refused(good, (32, 0, 48), good, FINE)
    placement_refused(good, SOURCE, good, (125, 29, 0))
    placement_refused(None, SOURCE, good, FINE)
    placement_refused(good, None, good, FINE)
    placement_refused(good, SOURCE, None, FINE)
    placement_refused(good, SOURCE, good, None)
    assert not bf.library().beamformer_hip_map_placement((C.c_float * 16)(*good), (C.c_uint32 * 3)(*SOURCE), (C.c_float * 16)(*good),
                                                         (C.c_uint32 * 3)(*FINE), None)
    # the FRAME's transform may be singular: a plane's peaks are placed in a map that has a y extent
    got = bf.map_placement(flat, (32, 1, 48), good, (125, 3, 189))
    assert np.isfinite(got).all() and not got[:, 1].any()


def test_refusals_that_need_no_device():
    L = bf.library()
    # reset: the extents are judged before anything else
    for points, kind in (((0, 4, 4), E.InvalidAccess), ((4, 4, 0), E.InvalidAccess), ((1 << 14, 1 << 14, 2), E.BufferOverflow),
                         ((0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), E.BufferOverflow), ((1 << 16, 1 << 16, 1 << 16), E.BufferOverflow)):
        assert not L.beamformer_hip_localisation_map_reset((C.c_uint32 * 3)(*points))
        assert bf.last_error()[0] == kind, points
    assert L.beamformer_hip_localisation_map_reset(None)                 # releasing a map that is not there succeeds

    rows = (P.HipMapDeposits * 4)()
    C.memset(rows, 0xA5, C.sizeof(rows))
    untouched = bytes(rows)
    ms = C.c_float(-1.0)
    level, identity = (C.c_float * 4)(0.0, 0.0, 0.0, 0.0), np.tile(np.eye(3, 4).reshape(-1), 4)

    def refused(kind, count=3, thresholds=level, threshold_count=1, placements=identity, placement_count=1):
        pointer = None if placements is None else np.ascontiguousarray(placements, np.float64).ctypes.data_as(C.POINTER(C.c_double))
        assert not L.beamformer_hip_accumulate_peaks_last_frames(count, None, thresholds, threshold_count, pointer, placement_count, 1, rows, C.byref(ms))
        assert bf.last_error()[0] == kind and bytes(rows) == untouched and ms.value == -1.0

    refused(E.BufferOverflow, count=0)
    refused(E.BufferOverflow, count=P.HIP_MAX_SCORED_FRAMES + 1)
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
    refused(E.InvalidAccess)                                             # no map: it was released above

    out, info = (C.c_uint32 * 4)(9, 9, 9, 9), P.HipMapInfo()
    C.memset(C.byref(info), 0x5A, C.sizeof(info))
    assert not L.beamformer_hip_localisation_map_copy(None, 4, C.byref(info)) and bf.last_error()[0] == E.InvalidAccess
    assert not L.beamformer_hip_localisation_map_copy(out, 4, C.byref(info)) and bf.last_error()[0] == E.InvalidAccess      # no map
    assert list(out) == [9] * 4 and bytes(info) == b"\x5A" * C.sizeof(info)

    frame = C.c_uint32(77)
    for scale in (float("nan"), float("inf"), -float("inf"), 1.0):       # 1.0: no map
        assert not L.beamformer_hip_queue_localisation_map(scale, 0, C.byref(frame), C.byref(ms))
        assert bf.last_error()[0] == E.InvalidAccess and frame.value == 77 and ms.value == -1.0


def test_the_records_have_the_headers_layout(tmp_path):
    assert C.sizeof(P.HipMapDeposits) == 96 and C.sizeof(P.HipMapInfo) == 32
    assert P.HIP_MAX_MAP_VOXELS == 1 << 28
    fields = {"BeamformerHipMapDeposits": (P.HipMapDeposits, [name for name, _ in P.HipMapDeposits._fields_]),
              "BeamformerHipMapInfo": (P.HipMapInfo, [name for name, _ in P.HipMapInfo._fields_])}
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "ogl_beamformer_hip.h"', "int main(void) {",
             '  printf("limit %llu\\n", (unsigned long long)BEAMFORMER_HIP_MAX_MAP_VOXELS);']
    for struct, (_, names) in fields.items():
        lines.append(f'  printf("{struct} %zu\\n", sizeof({struct}));')
        lines += [f'  printf("{struct}.{name} %zu\\n", offsetof({struct}, {name}));' for name in names]
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    said = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(said["limit"]) == P.HIP_MAX_MAP_VOXELS
    for struct, (cls, names) in fields.items():
        assert int(said[struct]) == C.sizeof(cls)
        for name in names:
            assert int(said[f"{struct}.{name}"]) == getattr(cls, name).offset, (struct, name)
        # no padding: the fields fill the struct
        assert sum(C.sizeof(kind) for _, kind in cls._fields_) == C.sizeof(cls)
