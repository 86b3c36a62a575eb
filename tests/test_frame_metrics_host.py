"""Frame metrics on the CPU (beamformer_hip_score_last_frames, beamformer_hip_copy_frame, beamformer_hip_get_frame_info,
beamformer_hip_rank_frames): the structs the binding mirrors are the header's, field by field, as gcc lays them out; the host-only
ranking computes the four criteria as written in the header; with no device in use the device calls refuse; and the numpy reference
the device tests judge against (tests/frame_metrics_ref.py) gives the sums of a frame small enough to work out by hand."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from ogl_beamforming_amd import lib
from ogl_beamforming_amd import params as P
from tests import frame_metrics_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = P.LibError
S = P.FrameScore
STRUCTS = {"BeamformerHipFrameRegion": P.HipFrameRegion, "BeamformerHipFrameMetrics": P.HipFrameMetrics, "BeamformerHipFrameInfo": P.HipFrameInfo}


def test_the_structs_are_the_headers_field_by_field(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ogl_beamformer_hip.h"', 'int main(void) {']
    for name, cls in STRUCTS.items():
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        for field, _ in cls._fields_:
            lines.append(f'printf("{name}.{field} %zu\\n", offsetof({name}, {field}));')
    lines += ['printf("MAX %u\\n", BEAMFORMER_HIP_MAX_SCORED_FRAMES);',
              'printf("SCORES %d %d %d %d %d\\n", BeamformerHipFrameScore_Energy, BeamformerHipFrameScore_MeanMagnitude, '
              'BeamformerHipFrameScore_Sharpness, BeamformerHipFrameScore_GradientEnergy, BeamformerHipFrameScore_Count);',
              'return 0; }']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    printed = dict(line.split(" ", 1) for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    checked = 0
    for name, cls in STRUCTS.items():
        assert C.sizeof(cls) == int(printed[name]), name
        for field, _ in cls._fields_:
            assert getattr(cls, field).offset == int(printed[f"{name}.{field}"]), (name, field)
            checked += 1
    assert checked == 2 + 17 + 6
    # no padding in a metrics row: rows compare byte for byte
    assert C.sizeof(P.HipFrameMetrics) == sum(C.sizeof(t) for _, t in P.HipFrameMetrics._fields_) == 160
    assert int(printed["MAX"]) == P.HIP_MAX_SCORED_FRAMES == P.HIP_MAX_VIEWS
    assert printed["SCORES"].split() == [str(int(v)) for v in (S.Energy, S.MeanMagnitude, S.Sharpness, S.GradientEnergy)] + ["4"]


def test_the_four_symbols_are_exported_and_bound():
    nm = subprocess.run(["nm", "-D", "--defined-only", lib.LIBRARY_PATH], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in nm.stdout.splitlines() if " T " in line}
    for name in ("beamformer_hip_score_last_frames", "beamformer_hip_copy_frame", "beamformer_hip_get_frame_info", "beamformer_hip_rank_frames"):
        assert name in exported and name in lib.exported_symbols(), name


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="needs the ROCm LLVM binutils")
def test_the_two_kernels_are_in_the_library_without_spills_or_scratch():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    kernels = [k for k in kernel_resources.kernels_of(lib.LIBRARY_PATH) if "frame_metrics_" in k["demangled"]]
    assert len({k["demangled"] for k in kernels}) == 2, sorted(k["demangled"] for k in kernels)
    for k in kernels:
        assert not k["vgpr_spill_count"] and not k["private_segment_fixed_size"], k["demangled"]


def row(voxels, s1, s2, s4, g=(0.0, 0.0, 0.0)):
    r = P.HipFrameMetrics()
    r.voxels, r.sum_abs, r.sum_abs2, r.sum_abs4 = voxels, s1, s2, s4
    r.gradient2[:] = g
    return r


ROWS = [row(960, 3100.5, 11810.25, 331000.0, (40.5, 0.0, 90.25)), row(900, 2900.0, 11760.0, 300100.0, (10.0, 2.0, 30.0)),
        row(7, 1e-3, 1e-7, 3e-15, (1e-9, 2e-9, 3e-9)), row(960, 4100.0, 22240.0, 1.2e6, (400.0, 1.0, 9.0))]


@pytest.mark.parametrize("criterion", list(S))
def test_rank_frames_computes_each_criterion_as_the_header_writes_it(criterion):
    scores, best = lib.rank_frames(ROWS, criterion)
    v = np.array([r.voxels for r in ROWS], np.float64)
    s1, s2, s4 = (np.array([getattr(r, k) for r in ROWS], np.float64) for k in ("sum_abs", "sum_abs2", "sum_abs4"))
    g = np.array([list(r.gradient2) for r in ROWS], np.float64)
    expected = {S.Energy: s2, S.MeanMagnitude: s1 / v, S.Sharpness: v * s4 / (s2 * s2), S.GradientEnergy: (g[:, 0] + g[:, 1] + g[:, 2]) / s2}[criterion]
    assert np.allclose(scores, expected, rtol=4e-16, atol=0.0), (scores, expected)
    assert best == int(np.argmax(expected))
    # and the reference module's own formula, which the device tests rank with
    assert np.allclose(scores, [ref.score(r, criterion) for r in ROWS], rtol=4e-16, atol=0.0)


def test_rank_frames_ties_empty_rows_and_refusals():
    L = lib.library()
    # ties go to the lowest index
    scores, best = lib.rank_frames([ROWS[1], ROWS[0], ROWS[0], ROWS[1]], S.Sharpness)
    assert best == 1 and scores[1] == scores[2] > scores[0]
    # a row without finite voxels, or without energy, scores -inf and is never best -- whatever its other fields say
    empty, dark = row(0, 9e9, 9e9, 9e99, (9e9, 9e9, 9e9)), row(10, 0.0, 0.0, 0.0)
    for criterion in S:
        scores, best = lib.rank_frames([empty, dark, ROWS[2]], criterion)
        assert best == 2 and scores[0] == scores[1] == -math.inf and math.isfinite(scores[2])
    # every row empty: 0, and the scores are filled all the same
    array = (P.HipFrameMetrics * 2)(empty, dark)
    scores = (C.c_double * 2)(1.0, 1.0)
    best = C.c_uint32(77)
    assert not L.beamformer_hip_rank_frames(array, 2, int(S.Energy), scores, C.byref(best)) and lib.last_error()[0] == E.InvalidAccess
    assert list(scores) == [-math.inf, -math.inf] and best.value == 77
    # unknown criterion, no rows, NULL arguments other than scores
    good = (P.HipFrameMetrics * 1)(ROWS[0])
    assert not L.beamformer_hip_rank_frames(good, 1, 4, None, C.byref(best)) and lib.last_error()[0] == E.InvalidAccess
    assert not L.beamformer_hip_rank_frames(good, 0, 0, None, C.byref(best)) and lib.last_error()[0] == E.InvalidAccess
    assert not L.beamformer_hip_rank_frames(None, 1, 0, None, C.byref(best)) and lib.last_error()[0] == E.InvalidAccess
    assert not L.beamformer_hip_rank_frames(good, 1, 0, None, None) and lib.last_error()[0] == E.InvalidAccess
    assert L.beamformer_hip_rank_frames(good, 1, 0, None, C.byref(best)) and best.value == 0


def test_with_no_device_in_use_the_device_calls_refuse():
    L = lib.library()
    L.beamformer_hip_shutdown()                       # (no device in use from here on: none of the calls below starts one)
    rows = (P.HipFrameMetrics * 1)()
    untouched = bytes(rows)
    ms = C.c_float(-1.0)
    for count in (0, P.HIP_MAX_SCORED_FRAMES + 1):
        assert not L.beamformer_hip_score_last_frames(count, None, rows, C.byref(ms)) and lib.last_error()[0] == E.BufferOverflow, count
    assert not L.beamformer_hip_score_last_frames(1, None, rows, C.byref(ms)) and lib.last_error()[0] == E.InvalidAccess
    assert not L.beamformer_hip_score_last_frames(1, None, None, None) and lib.last_error()[0] == E.InvalidAccess
    assert bytes(rows) == untouched and ms.value == -1.0
    out = np.zeros(16, np.float32)
    assert not L.beamformer_hip_copy_frame(0, out.ctypes.data_as(C.c_void_p), out.nbytes) and lib.last_error()[0] == E.InvalidAccess
    assert not L.beamformer_hip_copy_frame(0, None, 64) and lib.last_error()[0] == E.InvalidAccess
    info = P.HipFrameInfo()
    assert not L.beamformer_hip_get_frame_info(0, C.byref(info)) and lib.last_error()[0] == E.InvalidAccess


def test_the_reference_on_a_frame_worked_out_by_hand():
    """3 x 2 x 4 (x, y, z) complex voxels: |v| = 5 k for voxel k = x + 3 y + 6 z through v = (3 k, 4 k) -- exact in float32 --, voxel
    (1, 1, 2), k = 16, NaN.  Sums over k = 0 .. 23 without 16, times the powers of 5."""
    k = np.arange(24, dtype=np.float32).reshape(4, 2, 3)
    frame = (3 * k + 4j * k).astype(np.complex64)
    frame[2, 1, 1] = complex(np.nan, 1.0)
    r = ref.metrics(frame)
    ks = [n for n in range(24) if n != 16]
    assert r["points"] == (3, 2, 4) and r["region_first"] == (0, 0, 0) and r["region_count"] == (3, 2, 4)
    assert r["voxels"] == 23 and r["non_finite"] == 1
    assert r["sum_abs"] == 5.0 * (276 - 16) == 1300.0                               # 0 + 1 + ... + 23 = 276
    assert r["sum_abs2"] == 25.0 * (4324 - 256) == 101700.0                         # sum of squares to 23: 23 * 24 * 47 / 6 = 4324
    assert r["sum_abs4"] == 625.0 * sum(n ** 4 for n in ks)
    # x pairs: 2 a row, 8 rows, each (5)^2; the NaN at x = 1 takes both pairs of its row.  y pairs: 3 a plane, 4 planes, each (15)^2,
    # one lost.  z pairs: 6 a plane step, 3 steps, each (30)^2; the NaN takes the one below it and the one above it
    assert r["gradient_pairs"] == [16 - 2, 12 - 1, 18 - 2]
    assert r["gradient2"] == [14 * 25.0, 11 * 225.0, 16 * 900.0]
    assert r["max_abs"] == 115.0 and r["max_index"] == (2, 1, 3)
    # a box: x 1..2, y 1, z 1..2 -- voxels k = 10, 11, 16 (NaN), 17
    b = ref.metrics(frame, first=(1, 1, 1), count=(2, 1, 2))
    assert b["voxels"] == 3 and b["non_finite"] == 1 and b["sum_abs"] == 5.0 * (10 + 11 + 17)
    assert b["gradient_pairs"] == [1, 0, 1] and b["gradient2"] == [25.0, 0.0, 900.0]      # (10, 11); none; (11, 17)
    assert b["max_abs"] == 85.0 and b["max_index"] == (2, 1, 2)
    # ties: the first maximum in flat order; a real frame: abs; no finite voxel: zeros
    real = np.array([[[-2.0, 1.0, 2.0]], [[2.0, -np.inf, 0.5]]], np.float32)
    t = ref.metrics(real)
    assert t["max_abs"] == 2.0 and t["max_index"] == (0, 0, 0) and t["voxels"] == 5 and t["non_finite"] == 1
    assert t["sum_abs"] == 7.5 and t["gradient_pairs"] == [2, 0, 2] and t["gradient2"] == [1.0 + 1.0, 0.0, 0.0 + 1.5 * 1.5]
    none = ref.metrics(np.full((1, 1, 2), np.nan, np.float32))
    assert none["voxels"] == 0 and none["non_finite"] == 2 and none["max_abs"] == 0.0 and none["max_index"] == (0, 0, 0) and none["sum_abs2"] == 0.0
    assert ref.score(none, S.Sharpness) == -np.inf
