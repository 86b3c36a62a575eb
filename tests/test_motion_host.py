"""The shift correlation on the CPU (beamformer_hip_correlate_last_frames, beamformer_hip_displacements_from_correlation): the two
symbols are exported and bound; the three structs the binding mirrors are the header's, field by field, as gcc lays them out; the
kernels are in the library without spills or scratch; every refusal that needs no device holds, with its error kind, and leaves the
outputs alone; and the host-only helper agrees with its numpy restatement (tests/motion_ref.py) on synthetic tables built to reach every
rule: a clean peak, a tie, a peak at the window's edge, a flat axis, entries without terms beside the peak, a table without a candidate,
a table on which the normalised and the plain score choose different peaks, and an exactly parabolic profile."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from ogl_beamforming_amd import lib
from ogl_beamforming_amd import params as P
from tests import motion_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = P.LibError
SYMBOLS = ("beamformer_hip_correlate_last_frames", "beamformer_hip_displacements_from_correlation")
ENTRY = np.dtype(P.HipShiftCorrelation)


def test_the_two_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "ogl_beamformer_hip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", lib.LIBRARY_PATH], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in nm.stdout.splitlines() if " T " in line}
    for name in SYMBOLS:
        assert re.search(r"BEAMFORMER_LIB_EXPORT uint32_t " + name + r"\(", header), name
        assert name in exported and name in lib.exported_symbols(), name
        assert getattr(lib.library(), name).argtypes is not None


def test_the_structs_are_the_headers_field_by_field(tmp_path):
    structs = {"BeamformerHipShiftCorrelation": (P.HipShiftCorrelation, 40), "BeamformerHipCorrelationInfo": (P.HipCorrelationInfo, 56),
               "BeamformerHipDisplacement": (P.HipDisplacement, 40)}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ogl_beamformer_hip.h"', 'int main(void) {']
    for name, (cls, _) in structs.items():
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        for field, _ in cls._fields_:
            lines.append(f'printf("{name}.{field} %zu\\n", offsetof({name}, {field}));')
    lines += ['printf("LIMITS %u %u %u %u\\n", BEAMFORMER_HIP_MAX_SHIFT, BEAMFORMER_HIP_MAX_SHIFTS, BEAMFORMER_HIP_MAX_CORRELATION_REGIONS, '
              'BEAMFORMER_HIP_MAX_CORRELATION_ENTRIES);', 'return 0; }']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    printed = dict(line.split(" ", 1) for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    for name, (cls, size) in structs.items():
        assert C.sizeof(cls) == int(printed[name]) == sum(C.sizeof(t) for _, t in cls._fields_) == size, name      # no padding
        for field, _ in cls._fields_:
            assert getattr(cls, field).offset == int(printed[f"{name}.{field}"]), (name, field)
    assert ENTRY.itemsize == ref.ENTRY.itemsize == 40 and ENTRY.names == ref.ENTRY.names
    assert np.dtype(P.HipDisplacement).itemsize == ref.ROW.itemsize == 40 and np.dtype(P.HipDisplacement).names == ref.ROW.names
    assert [int(v) for v in printed["LIMITS"].split()] == [P.HIP_MAX_SHIFT, P.HIP_MAX_SHIFTS, P.HIP_MAX_CORRELATION_REGIONS,
                                                           P.HIP_MAX_CORRELATION_ENTRIES] == [16, 1089, 256, 1 << 20]


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="needs the ROCm LLVM binutils")
def test_the_kernels_are_in_the_library_without_spills_or_scratch():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    kernels = [k for k in kernel_resources.kernels_of(lib.LIBRARY_PATH) if "correlate_" in k["demangled"]]
    names = sorted(k["demangled"] for k in kernels)
    print(f"  {[(k['demangled'], k['vgpr_count'], k['sgpr_count'], k['group_segment_fixed_size']) for k in kernels]}")
    assert len(kernels) == 3, names                    # correlate_partial_kernel<true>, <false> and correlate_fold_kernel
    assert sum("correlate_partial_kernel" in n for n in names) == 2 and sum("correlate_fold_kernel" in n for n in names) == 1
    for k in kernels:
        assert not k["vgpr_spill_count"] and not k["sgpr_spill_count"] and not k["private_segment_fixed_size"], k["demangled"]
        assert k["group_segment_fixed_size"] <= 64 * 1024


def test_every_refusal_of_the_device_call_that_needs_no_device():
    L = lib.library()
    L.beamformer_hip_shutdown()                       # (no device in use from here on: the calls below start none)
    table = np.full(9, -7.0, np.float64).view(np.uint8).copy()          # canary bytes where a table would go
    room = (P.HipShiftCorrelation * 1).from_buffer(table)
    info = P.HipCorrelationInfo()
    C.memset(C.byref(info), 0x5A, C.sizeof(info))
    untouched = table.tobytes(), bytes(info)
    ms = C.c_float(-1.0)
    one = (P.HipFrameRegion * 1)(lib.frame_region((0, 0, 0), (1, 1, 1)))
    zero = (C.c_uint32 * 3)(0, 0, 0)

    def refused(kind, count=1, reference=0, regions=None, region_count=0, window=zero, out=room):
        assert not L.beamformer_hip_correlate_last_frames(count, reference, regions, region_count, window, out, C.byref(info), C.byref(ms))
        assert lib.last_error()[0] == kind, lib.last_error()
        assert (table.tobytes(), bytes(info)) == untouched and ms.value == -1.0

    # (the count, the outputs, a reference past the frames and the good call without a device: tests/test_frame_ops_contract_host.py)
    for n in (0, P.HIP_MAX_CORRELATION_REGIONS + 1):
        refused(E.BufferOverflow, regions=one, region_count=n)
    for axis in range(3):
        window = [0, 0, 0]
        window[axis] = P.HIP_MAX_SHIFT + 1
        refused(E.BufferOverflow, window=(C.c_uint32 * 3)(*window))
    refused(E.BufferOverflow, window=(C.c_uint32 * 3)(16, 16, 1))        # T = 33 * 33 * 3
    refused(E.BufferOverflow, window=(C.c_uint32 * 3)(5, 5, 5))          # T = 11 * 11 * 11 (11 * 11 * 9 = 1089 is legal: below)
    refused(E.BufferOverflow, count=256, window=(C.c_uint32 * 3)(16, 0, 16), regions=(P.HipFrameRegion * 4)(*([one[0]] * 4)), region_count=4)   # 4 * 256 * 1089 > 2^20
    refused(E.InvalidAccess, out=None)
    refused(E.InvalidAccess, window=None)
    refused(E.InvalidAccess, count=1, reference=1)
    # every argument good, the limits themselves among them: no device, so there is no frame -- InvalidAccess, never a crash
    refused(E.InvalidAccess, regions=one, region_count=1, window=(C.c_uint32 * 3)(16, 0, 16))
    refused(E.InvalidAccess, count=3, reference=2, window=(C.c_uint32 * 3)(4, 4, 4))
    refused(E.InvalidAccess, window=(C.c_uint32 * 3)(5, 5, 4))
    assert not L.beamformer_hip_correlate_last_frames(1, 0, None, 0, zero, room, None, None) and lib.last_error()[0] == E.InvalidAccess
    assert table.tobytes() == untouched[0]
    with pytest.raises(lib.BeamformerError):
        lib.correlate_last_frames(2, 0, (17, 0, 0))


def test_the_numpy_reference_against_the_definition_spelled_out_voxel_by_voxel():
    rng = np.random.default_rng(8100)
    frames = (rng.standard_normal((3, 4, 2, 5)) + 1j * rng.standard_normal((3, 4, 2, 5))).astype(np.complex64)
    frames[0, 1, 1, 2] = np.nan
    frames[2, 3, 0, 4] = complex(1.0, np.inf)
    window, boxes = (2, 1, 1), [((0, 0, 0), (5, 2, 4)), ((1, 1, 1), (3, 1, 2)), ((4, 1, 3), (1, 1, 1))]
    for reference in (0, 2):
        table, bars = ref.correlate(list(frames), reference, window, boxes)
        assert table.shape == (3, 3, 3, 3, 5) and bars.shape == table.shape + (3,)
        for b, ((x0, y0, z0), (nx, ny, nz)) in enumerate(boxes):
            for k in range(3):
                for sz in range(-1, 2):
                    for sy in range(-1, 2):
                        for sx in range(-2, 3):
                            c, er, ef, terms = 0j, 0.0, 0.0, 0
                            for z in range(z0, z0 + nz):
                                for y in range(y0, y0 + ny):
                                    for x in range(x0, x0 + nx):
                                        if not (0 <= x + sx < 5 and 0 <= y + sy < 2 and 0 <= z + sz < 4):
                                            continue
                                        r, f = complex(frames[reference, z, y, x]), complex(frames[k, z + sz, y + sy, x + sx])
                                        if not (np.isfinite(r.real) and np.isfinite(r.imag) and np.isfinite(f.real) and np.isfinite(f.imag)):
                                            continue
                                        c += r.conjugate() * f
                                        er += abs(r) ** 2
                                        ef += abs(f) ** 2
                                        terms += 1
                            e = table[b, k, sz + 1, sy + 1, sx + 2]
                            assert int(e["terms"]) == terms
                            assert np.allclose([e["re"], e["im"], e["energy_reference"], e["energy_frame"]], [c.real, c.imag, er, ef], rtol=1e-13, atol=1e-13)
                            assert (bars[b, k, sz + 1, sy + 1, sx + 2] > 0).all() == (terms > 0)
        # the sign convention: frame 1 := the reference moved by d = (1, 0, -1) peaks at s = d
    moved = np.zeros_like(frames[0])
    moved[:-1, :, 1:] = frames[1][1:, :, :-1]                   # moved[v + d] = ref[v]
    table, _ = ref.correlate([frames[1], moved], 0, (2, 0, 1), [((1, 0, 1), (3, 2, 2))])
    rows, found = ref.displacements(table, (2, 0, 1), True)
    assert found and tuple(rows[0, 1]["shift"]) == (1, 0, -1) and abs(rows[0, 1]["coefficient"] - 1.0) < 1e-6


# ---- the helper ----

def table_of(magnitudes, terms=1, energy=1.0):
    """a table of ENTRY with re = the magnitudes (array of shape (2 Sz + 1, 2 Sy + 1, 2 Sx + 1)), unit energies"""
    m = np.asarray(magnitudes, np.float64)
    t = np.zeros(m.shape, ref.ENTRY)
    t["re"], t["energy_reference"], t["energy_frame"], t["terms"] = m, energy, energy, terms
    return t


def window_of(table):
    return tuple((n - 1) // 2 for n in table.shape[::-1])


def helper(tables, window, normalised=1):
    """the library's rows for a list of tables of one window, and its return value"""
    flat = np.ascontiguousarray(np.stack([np.asarray(t) for t in tables])).view(ENTRY)
    out = np.full(len(tables), 0x5A5A5A5A, np.uint32).repeat(10).view(np.dtype(P.HipDisplacement)).copy()
    ok = lib.library().beamformer_hip_displacements_from_correlation(flat.ctypes.data_as(C.POINTER(P.HipShiftCorrelation)), len(tables),
                                                                     (C.c_uint32 * 3)(*window), normalised,
                                                                     out.ctypes.data_as(C.POINTER(P.HipDisplacement)))
    return out, ok


def agree(tables, window, normalised=1):
    """the library against the restatement: integers exactly, floats to float32 rounding; returns the library's rows"""
    got, ok = helper(tables, window, normalised)
    want, found = ref.displacements(np.stack(tables), window, bool(normalised))
    print(f"  window {window} normalised {normalised}: {[(tuple(r['shift']), tuple(r['displacement']), float(r['coefficient']), int(r['fitted']), int(r['at_window_edge'])) for r in got]}")
    assert bool(ok) == found
    for name in ("shift", "fitted", "at_window_edge"):
        assert np.array_equal(got[name], want[name]), name
    for name in ("displacement", "coefficient", "phase"):
        assert np.allclose(got[name], want[name], rtol=2.0 ** -22, atol=2.0 ** -22), name
    return got


def gaussian(window, centre, width=1.3):
    Sx, Sy, Sz = window
    z, y, x = np.meshgrid(np.arange(-Sz, Sz + 1), np.arange(-Sy, Sy + 1), np.arange(-Sx, Sx + 1), indexing="ij")
    return np.exp(-((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) / (2 * width ** 2))


def test_a_clean_peak_a_tie_an_edge_and_a_flat_axis():
    # a clean peak between voxels: the integer part is the nearest voxel, the offset points towards the true centre
    window = (4, 0, 3)
    rows = agree([table_of(gaussian(window, (1.3, 0.0, -1.8)))], window)
    r = rows[0]
    assert tuple(r["shift"]) == (1, 0, -2) and int(r["fitted"]) == 0b101 and int(r["at_window_edge"]) == 0
    assert 1.0 < r["displacement"][0] < 1.5 and -2.0 < r["displacement"][2] < -1.5 and r["displacement"][1] == 0.0
    assert abs(r["coefficient"] - gaussian(window, (1.3, 0.0, -1.8)).max()) < 1e-6 and r["phase"] == 0.0
    # the phase and the coefficient of a complex peak
    t = table_of(gaussian(window, (0.0, 0.0, 0.0)))
    t["im"], t["re"] = t["re"], 0.0
    t["energy_reference"], t["energy_frame"] = 4.0, 0.25
    r = agree([t], window)[0]
    assert tuple(r["shift"]) == (0, 0, 0) and abs(r["phase"] - np.pi / 2) < 1e-6 and abs(r["coefficient"] - 1.0) < 1e-6
    # a tie: two equal maxima, the lowest flat index wins (z slowest: the one at the lower z, whatever its x)
    m = np.zeros((5, 1, 5))
    m[1, 0, 3] = m[3, 0, 1] = 2.0
    m[1, 0, 2] = m[1, 0, 4] = m[0, 0, 3] = m[2, 0, 3] = 1.0
    r = agree([table_of(m)], (2, 0, 2))[0]
    assert tuple(r["shift"]) == (1, 0, -1) and int(r["fitted"]) == 0b101 and tuple(r["displacement"]) == (1.0, 0.0, -1.0)
    # a peak at the window's edge: the bits are set, the axis is not fitted
    window = (2, 1, 2)
    r = agree([table_of(gaussian(window, (2.6, -1.4, 0.2)))], window)[0]
    assert tuple(r["shift"]) == (2, -1, 0) and int(r["at_window_edge"]) == 0b011 and int(r["fitted"]) == 0b100
    assert r["displacement"][0] == 2.0 and r["displacement"][1] == -1.0
    # a flat axis, S = 0: never fitted, never at an edge
    r = agree([table_of(gaussian((0, 3, 0), (0.0, 0.4, 0.0)))], (0, 3, 0))[0]
    assert tuple(r["shift"]) == (0, 0, 0) and int(r["fitted"]) == 0b010 and int(r["at_window_edge"]) == 0
    # several tables in one call, each judged on its own
    window = (3, 0, 3)
    rows = agree([table_of(gaussian(window, c)) for c in ((-2.2, 0, 1.1), (0.4, 0, 0.4), (3.0, 0, -3.0))], window)
    assert [tuple(r["shift"]) for r in rows] == [(-2, 0, 1), (0, 0, 0), (3, 0, -3)]


def test_entries_without_terms_beside_the_peak_and_a_table_without_a_candidate():
    window = (3, 0, 3)
    t = table_of(gaussian(window, (0.3, 0.0, 0.3)))
    t["terms"][3, 0, 4] = 0                 # the +x neighbour of the peak at (0, 0, 0): x is not fitted, z still is
    r = agree([t], window)[0]
    assert tuple(r["shift"]) == (0, 0, 0) and int(r["fitted"]) == 0b100 and r["displacement"][0] == 0.0 and r["displacement"][2] > 0.0
    t["re"][2, 0, 3] = np.inf               # the -z neighbour is not finite: no candidate either
    r = agree([t], window)[0]
    assert tuple(r["shift"]) == (0, 0, 0) and int(r["fitted"]) == 0
    # an entry without terms is no candidate, however large
    t = table_of(gaussian(window, (1.0, 0.0, 1.0)))
    t["re"][0, 0, 0], t["terms"][0, 0, 0] = 1e9, 0
    assert tuple(agree([t], window)[0]["shift"]) == (1, 0, 1)
    # no candidate at all: the row is zero and the call returns 0 with InvalidAccess; beside a good table it returns 1
    empty = np.zeros((7, 1, 7), ref.ENTRY)
    got, ok = helper([empty], window)
    assert not ok and lib.last_error()[0] == E.InvalidAccess and not got.tobytes().strip(b"\0")
    nan = table_of(np.full((7, 1, 7), np.nan))
    got, ok = helper([nan, empty], window)
    assert not ok and not got.tobytes().strip(b"\0")
    rows = agree([empty, table_of(gaussian(window, (1.0, 0.0, 1.0))), nan], window)
    assert not rows[0].tobytes().strip(b"\0") and not rows[2].tobytes().strip(b"\0") and tuple(rows[1]["shift"]) == (1, 0, 1)
    # zero energies: no candidate when normalised; a candidate with coefficient 0 when not
    dark = table_of(gaussian(window, (0.0, 0.0, 0.0)), energy=0.0)
    got, ok = helper([dark], window, normalised=1)
    assert not ok and not got.tobytes().strip(b"\0")
    r = agree([dark], window, normalised=0)[0]
    assert tuple(r["shift"]) == (0, 0, 0) and r["coefficient"] == 0.0 and int(r["fitted"]) == 0b101


def test_normalised_and_plain_scores_choose_different_peaks():
    window = (2, 0, 0)
    t = table_of([[[1.0, 2.0, 8.0, 2.0, 1.0]]])
    t["energy_reference"] = [[[1.0, 1.0, 100.0, 1.0, 1.0]]]           # the brightest shift is the least correlated
    t["energy_frame"] = [[[1.0, 4.0, 100.0, 16.0, 1.0]]]
    plain = agree([t], window, normalised=0)[0]
    normal = agree([t], window, normalised=1)[0]
    assert tuple(plain["shift"]) == (0, 0, 0) and abs(plain["coefficient"] - 0.08) < 1e-7
    assert tuple(normal["shift"]) == (-2, 0, 0) and abs(normal["coefficient"] - 1.0) < 1e-7 and int(normal["at_window_edge"]) == 0b001
    t["re"][0, 0, 0] = 0.5                                           # -2 drops out of the tie: of -1 and +2 the lower index wins
    assert tuple(agree([t], window, normalised=1)[0]["shift"]) == (-1, 0, 0)


def test_an_exactly_parabolic_profile_gives_back_its_vertex():
    for centre in (0.0, 0.125, -0.375, 0.4999, -0.4999):
        x = np.arange(-3, 4, dtype=np.float64)
        m = 100.0 - (x - (1.0 + centre)) ** 2         # |C| itself is the parabola (positive all over the window): the helper fits m = sqrt(q)
        t = table_of(m.reshape(1, 1, 7))
        t["energy_reference"], t["energy_frame"] = 1.0, 1.0
        for normalised in (0, 1):
            lo, m0, hi = np.sqrt(m[3] ** 2), np.sqrt(m[4] ** 2), np.sqrt(m[5] ** 2)
            offset = 0.5 * (lo - hi) / ((lo + hi) - (m0 + m0))
            print(f"  vertex {centre}: offset {offset!r}, off by {abs(offset - centre):.3e}")
            assert abs(offset - centre) <= 1e-12
            r = agree([t], (3, 0, 0), normalised)[0]
            assert tuple(r["shift"]) == (1, 0, 0) and int(r["fitted"]) == 0b001
            assert r["displacement"][0] == np.float32(1.0 + offset)


def test_every_refusal_of_the_helper():
    L = lib.library()
    t = table_of(gaussian((1, 0, 1), (0, 0, 0))).view(ENTRY)
    tables = t.ctypes.data_as(C.POINTER(P.HipShiftCorrelation))
    out = (P.HipDisplacement * 1)()
    C.memset(out, 0x5A, C.sizeof(out))
    untouched = bytes(out)
    window = (C.c_uint32 * 3)(1, 0, 1)

    def refused(kind, tables=tables, count=1, window=window, rows=out):
        assert not L.beamformer_hip_displacements_from_correlation(tables, count, window, 1, rows)
        assert lib.last_error()[0] == kind and bytes(out) == untouched

    refused(E.InvalidAccess, tables=None)
    refused(E.InvalidAccess, window=None)
    refused(E.InvalidAccess, rows=None)
    refused(E.BufferOverflow, count=0)
    refused(E.BufferOverflow, window=(C.c_uint32 * 3)(17, 0, 0))
    refused(E.BufferOverflow, window=(C.c_uint32 * 3)(0, 0, 17))
    refused(E.BufferOverflow, window=(C.c_uint32 * 3)(16, 16, 1))
    assert L.beamformer_hip_displacements_from_correlation(tables, 1, window, 1, out) and bytes(out) != untouched
    with pytest.raises(lib.BeamformerError):
        lib.displacements_from_correlation(np.zeros((1, 1, 3, 1, 3), ENTRY), (1, 0, 1))
    rows = lib.displacements_from_correlation(np.stack([t, t]).reshape(2, 1, 3, 1, 3), (1, 0, 1))
    assert rows.shape == (2, 1) and not rows["shift"].any()
