"""Frame quantiles on the CPU (beamformer_hip_quantiles_last_frames, beamformer_hip_peak_threshold_of): the structs the binding mirrors
are the header's, field by field, as gcc lays them out; the kernels are in the library without spills or scratch; with no device in use
every refusal comes back with its error kind and leaves the outputs alone; the host-only threshold rule holds across the exponent
range; and the numpy reference the device tests judge against (tests/frame_quantiles_ref.py) gives the order statistics of a frame
small enough to work out by hand."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from ogl_beamforming_amd import lib
from ogl_beamforming_amd import params as P
from tests import frame_quantiles_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = P.LibError
STRUCTS = {"BeamformerHipFrameQuantile": P.HipFrameQuantile, "BeamformerHipFrameQuantiles": P.HipFrameQuantiles}
SYMBOLS = ("beamformer_hip_quantiles_last_frames", "beamformer_hip_peak_threshold_of")
REAL, COMPLEX = int(P.DataKind.Float32), int(P.DataKind.Float32Complex)


def test_the_structs_are_the_headers_field_by_field(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ogl_beamformer_hip.h"', 'int main(void) {']
    for name, cls in STRUCTS.items():
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        for field, _ in cls._fields_:
            lines.append(f'printf("{name}.{field} %zu\\n", offsetof({name}, {field}));')
    lines += ['printf("LIMITS %u %u\\n", BEAMFORMER_HIP_MAX_QUANTILES, BEAMFORMER_HIP_QUANTILE_BINS);', 'return 0; }']
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
        # no padding: records compare byte for byte
        assert C.sizeof(cls) == sum(C.sizeof(t) for _, t in cls._fields_), name
    assert checked == 8 + 12
    assert C.sizeof(P.HipFrameQuantile) == 48 and C.sizeof(P.HipFrameQuantiles) == 80
    assert printed["LIMITS"].split() == [str(P.HIP_MAX_QUANTILES), str(P.HIP_QUANTILE_BINS)] == ["16", "2048"] and ref.BINS == P.HIP_QUANTILE_BINS


def test_the_two_symbols_are_exported_and_bound():
    nm = subprocess.run(["nm", "-D", "--defined-only", lib.LIBRARY_PATH], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in nm.stdout.splitlines() if " T " in line}
    for name in SYMBOLS:
        assert name in exported and name in lib.exported_symbols(), name


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="needs the ROCm LLVM binutils")
def test_the_kernels_are_in_the_library_without_spills_or_scratch():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    kernels = [k for k in kernel_resources.kernels_of(lib.LIBRARY_PATH) if "frame_quantiles_" in k["demangled"]]
    # the first count pass, the two digit passes behind it, the pick
    assert len({k["demangled"] for k in kernels}) == 4, sorted(k["demangled"] for k in kernels)
    for k in kernels:
        assert not k["vgpr_spill_count"] and not k["private_segment_fixed_size"], k["demangled"]
        assert k["group_segment_fixed_size"] <= 64 * 1024, k["demangled"]


def test_with_no_device_in_use_every_refusal_leaves_the_outputs_alone():
    L = lib.library()
    L.beamformer_hip_shutdown()                       # (no device in use from here on: none of the calls below starts one)
    K = P.HIP_MAX_QUANTILES
    frames, records = (P.HipFrameQuantiles * 2)(), (P.HipFrameQuantile * (2 * K))()
    tables = np.full((2, P.HIP_QUANTILE_BINS), 0xA5A5A5A5, np.uint32)
    C.memset(frames, 0x5A, C.sizeof(frames))
    C.memset(records, 0x5A, C.sizeof(records))
    untouched = (bytes(frames), bytes(records), tables.tobytes())
    ms = C.c_float(-1.0)
    histograms = tables.ctypes.data_as(C.POINTER(C.c_uint32))

    def refused(kind, count, fractions, frames_out=frames, records_out=records, region=None, given=None):
        values = (C.c_double * max(1, len(fractions)))(*fractions)
        assert not L.beamformer_hip_quantiles_last_frames(count, None if region is None else C.byref(region), values if given is None else given,
                                                          len(fractions), frames_out, records_out, histograms, C.byref(ms))
        assert lib.last_error()[0] == kind, (lib.last_error(), count, fractions)
        assert (bytes(frames), bytes(records), tables.tobytes()) == untouched and ms.value == -1.0

    refused(E.BufferOverflow, 0, [0.5])
    refused(E.BufferOverflow, P.HIP_MAX_SCORED_FRAMES + 1, [0.5])
    refused(E.BufferOverflow, 1, [])
    refused(E.BufferOverflow, 1, [0.5] * (K + 1))
    assert not L.beamformer_hip_quantiles_last_frames(1, None, None, 1, frames, records, histograms, C.byref(ms)) and lib.last_error()[0] == E.InvalidAccess
    refused(E.InvalidAccess, 1, [0.5], frames_out=None)
    refused(E.InvalidAccess, 1, [0.5], records_out=None)
    for bad in (float("nan"), -1e-300, 1.0 + 2.0 ** -52, float("inf"), -float("inf")):
        refused(E.InvalidAccess, 1, [0.0, bad, 1.0])
    # well-formed arguments: there is no frame, as for beamformer_hip_score_last_frames
    refused(E.InvalidAccess, 1, [0.0, 0.5, 1.0])
    refused(E.InvalidAccess, 2, [0.5] * K, region=lib.frame_region((0, 0, 0), (1, 1, 1)))
    assert (bytes(frames), bytes(records), tables.tobytes()) == untouched and ms.value == -1.0


def bits_of(values):
    return np.asarray(values, np.float32).view(np.uint32)


def floats_of(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def test_peak_threshold_of_brackets_the_value_across_the_exponent_range():
    rng = np.random.default_rng(20261)
    largest = np.finfo(np.float32).max
    exact_roots = np.float32([1.0, 4.0, 9.0, 2.25, 2.0 ** -40, 2.0 ** 100, 1e4]) ** 1            # squares of floats
    # no float's rounded square: for t in [1, sqrt 2) x 2^k the squares of neighbouring floats lie 2 t > 2.2 floats of t * t apart, so
    # after rounding at least two: the float behind fl(t * t) is the square of none
    t = np.float32([1.1, 1.3 * 2.0 ** -20, 1.2 * 2.0 ** 30])
    with np.errstate(over="ignore", under="ignore"):
        gaps = floats_of(bits_of(t * t) + np.uint32(1))
        assert all(not (np.float32(s * s) == g) for g in gaps for s in floats_of(bits_of(np.sqrt(g)) + np.arange(-2, 3).astype(np.uint32)))
    special = np.concatenate([np.float32([0.0, largest]), floats_of([1, 2, 3, 0x007FFFFF, 0x00800000]), exact_roots, gaps])
    seeded = floats_of(rng.integers(0, 0x7F800000, 4000, dtype=np.uint32))
    values = np.concatenate([special, seeded])
    assert np.isfinite(values).all() and (values >= 0).all()
    T = np.float32([lib.peak_threshold_of(q, COMPLEX) for q in values])
    up = np.nextafter(T, np.float32(np.inf))
    with np.errstate(over="ignore", under="ignore"):
        assert (T >= 0).all() and (T * T <= values).all()
        assert (T.dtype, (T * T).dtype) == (np.float32, np.float32)
        above = up * up                                  # inf for the largest float: above every finite value
        assert (values < above).all(), values[~(values < above)]
    # the reference's own rule agrees bit for bit
    for q, t in zip(values[:len(special) + 200], T):
        assert bits_of(ref.threshold_of(q, True)) == bits_of(t), q
    # exact roots come back as they are; zero takes every T whose square rounds to zero
    for q in exact_roots:
        assert lib.peak_threshold_of(q, COMPLEX) == np.sqrt(q)
    assert lib.peak_threshold_of(0.0, COMPLEX) == 2.0 ** -75
    # the real kind returns the value itself
    for q in values[:64]:
        assert bits_of(lib.peak_threshold_of(q, REAL)) == bits_of(q)


def test_peak_threshold_of_refusals():
    L = lib.library()
    out = C.c_float(-7.0)
    assert not L.beamformer_hip_peak_threshold_of(1.0, COMPLEX, None) and lib.last_error()[0] == E.InvalidAccess
    for bad in (-1.0, -1e-45, float("nan"), float("inf"), -float("inf")):
        for kind in (REAL, COMPLEX):
            assert not L.beamformer_hip_peak_threshold_of(bad, kind, C.byref(out)) and lib.last_error()[0] == E.InvalidAccess, (bad, kind)
    for kind in set(range(8)) - {REAL, COMPLEX}:
        assert not L.beamformer_hip_peak_threshold_of(1.0, kind, C.byref(out)) and lib.last_error()[0] == E.InvalidAccess, kind
    assert out.value == -7.0
    assert L.beamformer_hip_peak_threshold_of(4.0, COMPLEX, C.byref(out)) and out.value == 2.0


def test_the_reference_on_a_frame_worked_out_by_hand():
    """3 x 2 x 4 (x, y, z) complex voxels v = (3 m, 4 m) with m = k // 2 for voxel k = x + 3 y + 6 z: q = 25 m^2, exact in float32, every
    value twice (ties); voxel (1, 1, 2), k = 16, NaN.  The finite values in order: m = 0, 0, 1, 1, ..., 7, 7, 8 (once: k = 17), 9, 9, 10,
    10, 11, 11 -- 23 of them."""
    m = (np.arange(24) // 2).astype(np.float32).reshape(4, 2, 3)
    frame = (3 * m + 4j * m).astype(np.complex64)
    frame[2, 1, 1] = complex(np.nan, 1.0)
    ms = sorted(n // 2 for n in range(24) if n != 16)
    r = ref.quantiles(frame, [0.0, 1.0, 0.5, 0.5, 0.26])
    assert r["points"] == (3, 2, 4) and r["region_first"] == (0, 0, 0) and r["region_count"] == (3, 2, 4)
    assert r["voxels"] == 23 and r["non_finite"] == 1
    rows = r["rows"]
    # f = 0: the minimum, 0, twice; f = 1: the maximum, 25 * 121, twice, 21 below
    assert (rows[0]["rank"], rows[0]["value"], rows[0]["below"], rows[0]["equal"]) == (0, 0.0, 0, 2)
    assert (rows[1]["rank"], rows[1]["value"], rows[1]["below"], rows[1]["equal"]) == (22, 25.0 * 121, 21, 2)
    assert rows[1]["magnitude"] == 55.0 and rows[1]["threshold"] == 55.0
    # f = 0.5: rank floor(11 + 0.5) = 11, the twelfth value: m = 5 (ms[11]), ten below, two equal
    assert ms[11] == 5
    assert (rows[2]["rank"], rows[2]["value"], rows[2]["below"], rows[2]["equal"]) == (11, 625.0, 10, 2) and rows[2]["magnitude"] == 25.0
    assert rows[3] == rows[2]
    # f = 0.26: floor(5.72 + 0.5) = 6: m = 3
    assert (rows[4]["rank"], rows[4]["value"], rows[4]["below"], rows[4]["equal"]) == (6, 225.0, 6, 2)
    # the histogram: bits >> 20 of each value; the two zeros in bin 0; sums to n
    assert int(r["histogram"].sum()) == 23 and r["histogram"][0] == 2 and not r["histogram"][2040:].any()
    assert r["histogram"][int(bits_of([225.0])[0]) >> 20] >= 2
    # a box: x 1..2, y 1, z 1..2 -- voxels k = 10, 11, 16 (NaN), 17: m = 5, 5, 8
    b = ref.quantiles(frame, [0.0, 0.5, 1.0], first=(1, 1, 1), count=(2, 1, 2))
    assert b["voxels"] == 3 and b["non_finite"] == 1
    assert [(q["rank"], q["value"], q["below"], q["equal"]) for q in b["rows"]] == [(0, 625.0, 0, 2), (1, 625.0, 0, 2), (2, 1600.0, 2, 1)]
    # a real frame: abs, and -0 is +0
    real = np.array([[[-2.0, 1.0, 2.0]], [[-0.0, -np.inf, 0.5]]], np.float32)
    t = ref.quantiles(real, [1.0, 0.0, 0.5])
    assert t["voxels"] == 5 and t["non_finite"] == 1
    assert [(q["rank"], q["value"], q["below"], q["equal"]) for q in t["rows"]] == [(4, 2.0, 3, 2), (0, 0.0, 0, 1), (2, 1.0, 2, 1)]
    assert t["rows"][0]["magnitude"] == t["rows"][0]["threshold"] == 2.0 and t["rows"][1]["value_bits"] == 0
    # no finite voxel
    none = ref.quantiles(np.full((1, 1, 2), np.nan, np.float32), [0.0, 0.5, 1.0])
    assert none["voxels"] == 0 and none["non_finite"] == 2 and not none["histogram"].any()
    empty = ref.quantiles(np.full((2, 1, 1), complex(np.inf, 0.0), np.complex64), [0.0, 0.5, 1.0])
    assert empty["voxels"] == 0 and empty["non_finite"] == 2
    for q in none["rows"] + empty["rows"]:
        assert (q["rank"], q["below"], q["equal"], q["value"], q["magnitude"], q["threshold"]) == (0, 0, 0, 0.0, 0.0, 0.0)
    # (an all-zero complex frame is another matter: its value 0 is a voxel's, and every T whose square rounds to 0 is below it)
    zero = ref.quantiles(np.zeros((1, 1, 2), np.complex64), [0.5])["rows"][0]
    assert (zero["value"], zero["below"], zero["equal"], zero["threshold"]) == (0.0, 0, 2, 2.0 ** -75)
