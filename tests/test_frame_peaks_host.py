"""Frame peaks on the CPU (beamformer_hip_find_peaks_last_frames, beamformer_hip_peaks_to_views): the structs the binding mirrors are
the header's, field by field, as gcc lays them out; the kernels DESIGN 3.7b lists are in the library without spills or scratch; every
refusal that needs no device holds, with its error kind, and leaves the outputs alone; the numpy reference the device tests judge against
(tests/frame_peaks_ref.py) gives the lists of frames small enough to work out by hand; and the host-only patch placement lands every
patch voxel where a float64 restatement puts it."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from ogl_beamforming_amd import configs as cfg
from ogl_beamforming_amd import lib
from ogl_beamforming_amd import params as P
from tests import frame_peaks_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = P.LibError
STRUCTS = {"BeamformerHipFramePeak": P.HipFramePeak, "BeamformerHipFramePeaks": P.HipFramePeaks}
SYMBOLS = ("beamformer_hip_find_peaks_last_frames", "beamformer_hip_peaks_to_views")


def test_the_structs_are_the_headers_field_by_field(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ogl_beamformer_hip.h"', 'int main(void) {']
    for name, cls in STRUCTS.items():
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        for field, _ in cls._fields_:
            lines.append(f'printf("{name}.{field} %zu\\n", offsetof({name}, {field}));')
    lines += ['printf("MAX %u\\n", BEAMFORMER_HIP_MAX_PEAKS_PER_FRAME);', 'return 0; }']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    printed = dict(line.split(" ", 1) for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    checked = 0
    for name, cls in STRUCTS.items():
        assert C.sizeof(cls) == int(printed[name]) == sum(C.sizeof(t) for _, t in cls._fields_), name      # no padding
        for field, _ in cls._fields_:
            assert getattr(cls, field).offset == int(printed[f"{name}.{field}"]), (name, field)
            checked += 1
    assert checked == 4 + 12
    assert C.sizeof(P.HipFramePeak) == 32 and C.sizeof(P.HipFramePeaks) == 80
    assert [f for f, _ in P.HipFramePeak._fields_] == ["index", "magnitude", "offset", "fitted"]
    assert [f for f, _ in P.HipFramePeaks._fields_] == ["frame_id", "parameter_block", "data_kind", "image_plane_tag", "points", "region_first",
                                                        "region_count", "threshold", "first", "stored", "found", "above_threshold"]
    assert int(printed["MAX"]) == P.HIP_MAX_PEAKS_PER_FRAME == 65536


def test_the_two_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "ogl_beamformer_hip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", lib.LIBRARY_PATH], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in nm.stdout.splitlines() if " T " in line}
    for name in SYMBOLS:
        assert re.search(r"BEAMFORMER_LIB_EXPORT uint32_t " + name + r"\(", header), name
        assert name in exported and name in lib.exported_symbols(), name
        assert getattr(lib.library(), name).argtypes is not None


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="needs the ROCm LLVM binutils")
def test_the_kernels_design_lists_are_in_the_library_without_spills_or_scratch():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    listed = set(re.findall(r"frame_peaks_\w+_kernel", open(os.path.join(ROOT, "DESIGN.md")).read()))
    assert len(listed) == 3, listed
    kernels = [k for k in kernel_resources.kernels_of(lib.LIBRARY_PATH) if "frame_peaks_" in k["demangled"]]
    names = {k["demangled"] for k in kernels}
    assert len(names) == 3 and all(sum(want in name for name in names) == 1 for want in listed), (names, listed)
    for k in kernels:
        assert not k["vgpr_spill_count"] and not k["private_segment_fixed_size"], k["demangled"]


def test_every_refusal_that_needs_no_device():
    L = lib.library()
    L.beamformer_hip_shutdown()                       # (no device in use from here on: none of the calls below starts one)
    rows = (P.HipFramePeaks * 2)()
    peaks = (P.HipFramePeak * 8)()
    C.memset(rows, 0x5A, C.sizeof(rows))
    C.memset(peaks, 0x5A, C.sizeof(peaks))
    untouched = bytes(rows), bytes(peaks)
    total, ms = C.c_uint32(77), C.c_float(-1.0)
    one, two = (C.c_float * 1)(0.5), (C.c_float * 2)(0.5, 0.25)

    def refused(kind, count=1, thresholds=one, threshold_count=1, cap=4, frames=rows, out=peaks, n=C.byref(total)):
        assert not L.beamformer_hip_find_peaks_last_frames(count, None, thresholds, threshold_count, cap, frames, out, n, C.byref(ms))
        assert lib.last_error()[0] == kind
        assert (bytes(rows), bytes(peaks)) == untouched and total.value == 77 and ms.value == -1.0

    for count in (0, P.HIP_MAX_SCORED_FRAMES + 1):
        refused(E.BufferOverflow, count=count)
    for cap in (0, P.HIP_MAX_PEAKS_PER_FRAME + 1):
        refused(E.BufferOverflow, cap=cap)
    # BufferOverflow is decided first, whatever else is wrong
    refused(E.BufferOverflow, count=0, thresholds=None)
    # NULL pointers other than region and device_ms
    refused(E.InvalidAccess, thresholds=None)
    refused(E.InvalidAccess, frames=None)
    refused(E.InvalidAccess, out=None)
    refused(E.InvalidAccess, n=None)
    # threshold_count neither 1 nor count
    refused(E.InvalidAccess, count=2, thresholds=two, threshold_count=0)
    refused(E.InvalidAccess, count=1, thresholds=two, threshold_count=2)
    refused(E.InvalidAccess, count=2, thresholds=two, threshold_count=3)
    # a threshold that is negative or not finite -- the second of two as well
    for bad in (-1.0, -1e-30, float("nan"), float("inf"), float("-inf")):
        refused(E.InvalidAccess, thresholds=(C.c_float * 1)(bad))
        refused(E.InvalidAccess, count=2, thresholds=(C.c_float * 2)(0.5, bad), threshold_count=2)
    # and with every argument good: no device yet, so there is no frame -- InvalidAccess, after the argument checks, device_ms NULL or not
    refused(E.InvalidAccess)
    refused(E.InvalidAccess, count=2, thresholds=two, threshold_count=2)
    assert not L.beamformer_hip_find_peaks_last_frames(1, None, one, 1, 4, rows, peaks, C.byref(total), None) and lib.last_error()[0] == E.InvalidAccess
    region = lib.frame_region((0, 0, 0), (1, 1, 1))
    assert not L.beamformer_hip_find_peaks_last_frames(1, C.byref(region), one, 1, 4, rows, peaks, C.byref(total), None)
    assert lib.last_error()[0] == E.InvalidAccess and (bytes(rows), bytes(peaks)) == untouched


# ---- the reference on synthetic arrays ----

def listed(r):
    return [tuple(int(v) for v in i) for i in r["index"]]


def test_the_reference_on_all_zero_frames():
    for frame in (np.zeros((4, 3, 5), np.float32), np.zeros((4, 3, 5), np.complex64), np.zeros((7, 1, 6), np.float32)):
        r = ref.peaks(frame, 0.0)
        assert r["found"] == 1 and listed(r) == [(0, 0, 0)] and r["above_threshold"] == frame.size
        assert r["fitted"][0] == 0 and not r["offset"].any() and r["magnitude"][0] == 0.0        # den is 0 on a plateau: no axis fitted
        off = ref.peaks(frame, 0.0, first=(1, 0, 0), count=(frame.shape[2] - 1, frame.shape[1], frame.shape[0]))
        assert off["found"] == 0 and off["stored"] == 0 and off["above_threshold"] == frame.size - frame.shape[1] * frame.shape[0]
    # nothing is eligible above a positive threshold
    assert ref.peaks(np.zeros((4, 3, 5), np.float32), 1e-3)["found"] == 0


@pytest.mark.parametrize("n", [1, 2, 7, 8, 65])
def test_the_reference_on_a_row_of_alternating_values(n):
    row = np.where(np.arange(n) % 2 == 0, 2.0, 1.0).astype(np.float32).reshape(1, 1, n)
    r = ref.peaks(row, 0.0)
    assert r["found"] == (n + 1) // 2 and listed(r) == [(x, 0, 0) for x in range(0, n, 2)]
    assert r["above_threshold"] == n
    # interior peaks are fitted along x with offset 0 (symmetric), the ends are not; y and z have no neighbours
    for (x, _, _), fitted, offset in zip(listed(r), r["fitted"], r["offset"]):
        assert fitted == (1 if 0 < x < n - 1 else 0) and not offset.any()
    # the same along z, and negated (a real frame is judged by |v|)
    assert listed(ref.peaks(-row.reshape(n, 1, 1), 0.0)) == [(0, 0, z) for z in range(0, n, 2)]
    # a threshold between the two values leaves the peaks, one above them none
    assert ref.peaks(row, 1.5)["found"] == (n + 1) // 2 and ref.peaks(row, 1.5)["above_threshold"] == (n + 1) // 2
    assert ref.peaks(row, 2.5)["found"] == 0


def test_the_reference_on_plateaus_nan_neighbours_box_faces_and_fits():
    frame = np.zeros((3, 4, 6), np.float32)
    frame[1, 2, 2] = frame[1, 2, 3] = 5.0                          # a two-voxel plateau along x
    r = ref.peaks(frame, 1.0)
    assert listed(r) == [(2, 2, 1)] and r["above_threshold"] == 2
    # ... along z and along a diagonal: the lower flat index
    frame = np.zeros((3, 4, 6), np.float32)
    frame[0, 1, 4] = frame[1, 1, 4] = 5.0
    assert listed(ref.peaks(frame, 1.0)) == [(4, 1, 0)]
    frame = np.zeros((3, 4, 6), np.float32)
    frame[1, 1, 4] = frame[2, 2, 3] = 5.0
    assert listed(ref.peaks(frame, 1.0)) == [(4, 1, 1)]
    # no two adjacent voxels are both peaks, whatever the frame: random small integers, many ties
    rng = np.random.default_rng(11)
    frame = rng.integers(0, 3, (6, 5, 7)).astype(np.float32)
    mask, _ = ref.peak_mask(frame, 0.0)
    z, y, x = np.nonzero(mask)
    for a in range(len(x)):
        for b in range(a + 1, len(x)):
            assert max(abs(int(z[a]) - int(z[b])), abs(int(y[a]) - int(y[b])), abs(int(x[a]) - int(x[b]))) > 1
    assert len(x) >= 2
    # a NaN (and an infinite) neighbour is ignored: the voxel beside it is judged by the rest; a larger finite neighbour still beats it
    frame = np.ones((1, 3, 5), np.complex64)
    frame[0, 1, 2] = 3.0
    frame[0, 1, 3] = complex(np.nan, 0.0)
    frame[0, 0, 2] = complex(0.0, np.inf)
    frame[0, 2, 1] = 2e20                                          # q overflows float32: not finite, although re and im are
    r = ref.peaks(frame, 2.0)
    assert listed(r) == [(2, 1, 0)] and r["above_threshold"] == 1 and r["magnitude"][0] == 3.0
    assert r["fitted"][0] == 0                                     # x: the +1 neighbour is NaN; y: the -1 neighbour is infinite; z: none
    frame[0, 1, 1] = 4.0
    assert listed(ref.peaks(frame, 2.0)) == [(1, 1, 0)]
    # a voxel on the face of a box is beaten by a voxel outside the box; clipping the neighbourhood to the box would invent it
    frame = np.zeros((1, 5, 8), np.float32)
    frame[0, 2, 3], frame[0, 2, 4] = 2.0, 3.0
    box = ((0, 0, 0), (4, 5, 1))                                   # x 0 .. 3: the 3.0 lies just outside
    assert listed(ref.peaks(frame, 1.0, *box)) == [] and ref.peaks(frame, 1.0, *box)["above_threshold"] == 1
    assert listed(ref.peaks(frame, 1.0, *box, clip_to_box=True)) == [(3, 2, 0)]
    assert listed(ref.peaks(frame, 1.0)) == [(4, 2, 0)]
    # tiling the frame into two boxes neither invents nor doubles a peak
    frame = rng.random((3, 6, 9)).astype(np.float32)
    whole = listed(ref.peaks(frame, 0.2))
    halves = listed(ref.peaks(frame, 0.2, (0, 0, 0), (4, 6, 3))) + listed(ref.peaks(frame, 0.2, (4, 0, 0), (5, 6, 3)))
    assert sorted(halves) == sorted(whole) and len(whole) >= 2
    # the cap keeps the first in flat order and leaves found alone
    capped = ref.peaks(frame, 0.2, cap=2)
    assert capped["found"] == len(whole) and capped["stored"] == 2 and listed(capped) == whole[:2]
    # the fit: magnitudes 1, 4, 2 along x -> den = 3 - 8 = -5, offset = 0.5 * (1 - 2) / -5 = 0.1; a steep side clamps to 0.5
    frame = np.zeros((1, 1, 5), np.float32)
    frame[0, 0, 1:4] = (1.0, 4.0, 2.0)
    r = ref.peaks(frame, 3.0)
    assert listed(r) == [(2, 0, 0)] and r["fitted"][0] == 1 and r["offset"][0, 0] == np.float32(0.5) * np.float32(-1.0) / np.float32(-5.0)
    cplx = (frame * (0.6 + 0.8j)).astype(np.complex64)             # |v| within rounding of the same magnitudes: the threshold is on |v|
    r = ref.peaks(cplx, 3.0)
    assert listed(r) == [(2, 0, 0)] and abs(float(r["offset"][0, 0]) - 0.1) < 1e-6 and ref.peaks(cplx, 4.5)["found"] == 0


# ---- peaks_to_views against a float64 restatement ----

def point64(m, v):
    """the kernels' m4_point in float64: column-major m, normalised voxel v"""
    m = np.asarray(m, np.float64).reshape(4, 4).T                  # rows x columns
    return (m @ np.array([v[0], v[1], v[2], 1.0]))[:3]


def peak(index, offset=(0.0, 0.0, 0.0)):
    p = P.HipFramePeak()
    p.index[:] = index
    p.offset[:] = offset
    p.fitted = 7
    return p


GRIDS = [("plane", (65, 1, 96), (-8e-3, 0.0, 2e-3), (8e-3, 0.0, 30e-3)), ("volume", (24, 17, 40), (-6e-3, -4e-3, 1e-3), (6e-3, 5e-3, 21e-3))]


@pytest.mark.parametrize("name,points,lo,hi", GRIDS, ids=[g[0] for g in GRIDS])
@pytest.mark.parametrize("use_offsets", [True, False], ids=["offsets", "whole voxels"])
def test_peaks_to_views_lands_every_patch_voxel_where_float64_puts_it(name, points, lo, hi, use_offsets):
    source = [float(v) for v in cfg._voxel_transform(points, lo, hi)]
    peaks = [peak((0, 0, 0)), peak((points[0] - 1, points[1] - 1, points[2] - 1), (-0.5, 0.0, 0.5)),
             peak((points[0] // 2, points[1] // 2, points[2] // 3), (0.31, -0.27 if points[1] > 1 else 0.0, -0.44))]
    worst = 0.0
    for patch, extent in (((17, 1, 17), (4.0, 0.0, 4.0)), ((9, 5, 1), (2.0, 1.0, 3.0)), ((1, 1, 1), (0.0, 0.0, 0.0)), ((16, 3, 16), (3.75, 0.5, 2.5))):
        views = lib.peaks_to_views(source, points, peaks, patch, extent, use_offsets=use_offsets, tag=2)
        assert len(views) == len(peaks)
        for p, v in zip(peaks, views):
            assert tuple(v.output_points) == patch and v.image_plane_tag == 2
            m = list(v.das_voxel_transform)
            assert np.linalg.matrix_rank(np.asarray(m, np.float64).reshape(4, 4), tol=1e-12) == np.linalg.matrix_rank(np.asarray(source).reshape(4, 4), tol=1e-12)
            last = [max(1, n - 1) for n in points]
            centre = [p.index[a] + (float(p.offset[a]) if use_offsets else 0.0) for a in range(3)]
            # the world extent of the source grid: what the rounding of a transform entry is relative to
            size = max(np.abs(point64(source, c)).max() for c in ((0, 0, 0), (1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)))
            # Bar.  The patch's 12 entries are float64 results rounded ONCE to float32: 2^-24 relative each.  point64 adds four products
            # of an entry with a coordinate in [0, 1]: at most 4 x 2^-24 x the largest entry involved, itself at most `size` (entries are
            # extents and origins of the grid) times the patch's scale <= 1, plus the float32 inputs being exact.  2^-21 x size is that
            # with a factor 2 in hand.
            bar = 2.0 ** -21 * size
            for j in {(0, 0, 0), tuple(n - 1 for n in patch), tuple(n // 2 for n in patch)}:
                inside = [j[a] / max(1, patch[a] - 1) for a in range(3)]
                got = point64(m, inside)
                voxel = [centre[a] - extent[a] / 2 + j[a] * extent[a] / (patch[a] - 1) if patch[a] > 1 else centre[a] for a in range(3)]
                expected = point64(source, [voxel[a] / last[a] for a in range(3)])
                worst = max(worst, float(np.abs(got - expected).max()) / bar)
                assert np.abs(got - expected).max() <= bar, (name, patch, j, got, expected)
    print(f"  {name}: worst deviation {worst:.3f} of the bar")


def test_peaks_to_views_refusals_and_the_empty_list():
    L = lib.library()
    source = (C.c_float * 16)(*[float(v) for v in cfg._voxel_transform((24, 1, 40), (-6e-3, 0, 1e-3), (6e-3, 0, 21e-3))])
    points, patch, extent = (C.c_uint32 * 3)(24, 1, 40), (C.c_uint32 * 3)(5, 1, 5), (C.c_float * 3)(2.0, 0.0, 2.0)
    peaks = (P.HipFramePeak * 1)(peak((3, 0, 4)))
    out = (P.HipView * 1)()
    C.memset(out, 0x5A, C.sizeof(out))
    untouched = bytes(out)

    def refused(*args):
        assert not L.beamformer_hip_peaks_to_views(*args) and lib.last_error()[0] == E.InvalidAccess and bytes(out) == untouched

    refused(None, points, peaks, 1, patch, extent, 1, 0, out)
    refused(source, None, peaks, 1, patch, extent, 1, 0, out)
    refused(source, points, None, 1, patch, extent, 1, 0, out)
    refused(source, points, peaks, 1, None, extent, 1, 0, out)
    refused(source, points, peaks, 1, patch, None, 1, 0, out)
    refused(source, points, peaks, 1, patch, extent, 1, 0, None)
    for axis in range(3):
        zero = (C.c_uint32 * 3)(5, 1, 5)
        zero[axis] = 0
        refused(source, points, peaks, 1, zero, extent, 1, 0, out)
        for bad in (-1.0, float("nan"), float("inf")):
            wrong = (C.c_float * 3)(2.0, 0.0, 2.0)
            wrong[axis] = bad
            refused(source, points, peaks, 1, patch, wrong, 1, 0, out)
    assert L.beamformer_hip_peaks_to_views(source, points, peaks, 0, patch, extent, 1, 0, out) and bytes(out) == untouched
    assert L.beamformer_hip_peaks_to_views(source, points, peaks, 1, patch, extent, 1, 0, out) and tuple(out[0].output_points) == (5, 1, 5)
    assert lib.peaks_to_views(list(source), (24, 1, 40), [], (5, 1, 5), (2.0, 0.0, 2.0)) == []
