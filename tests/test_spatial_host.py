"""The spatial filter on the CPU (beamformer_hip_convolve_last_frames): the symbol is declared, exported and bound; the kernels DESIGN 3.7e
lists are in the library, twelve instantiations without spills or scratch; every refusal that needs no device holds, with its error
kind, and leaves the outputs alone; and the numpy reference the device tests judge against (tests/spatial_ref.py) gives cases small
enough to work out by hand, holds a float32 restatement inside its own bound, and tells the definition from the three mistakes nearest
to it."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from ogl_beamforming_amd import lib
from ogl_beamforming_amd import params as P
from tests import spatial_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = P.LibError
NAME = "beamformer_hip_convolve_last_frames"
MAX = P.HIP_MAX_ENSEMBLE_FRAMES
TAPS = P.HIP_MAX_SPATIAL_TAPS


def test_the_symbol_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "ogl_beamformer_hip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", lib.LIBRARY_PATH], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in nm.stdout.splitlines() if " T " in line}
    assert re.search(r"BEAMFORMER_LIB_EXPORT uint32_t " + NAME + r"\(", header)
    assert NAME in exported and NAME in lib.exported_symbols()
    assert len(getattr(lib.library(), NAME).argtypes) == 7
    assert re.search(r"#define BEAMFORMER_HIP_MAX_SPATIAL_TAPS (\d+)u", header).group(1) == str(TAPS) == "33"
    assert [(m.name, int(m)) for m in P.HipSpatialMode] == [("Zero", 0), ("Normalised", 1)]
    assert re.search(r"BeamformerHipSpatialMode_Zero\s*= 0,\s*BeamformerHipSpatialMode_Normalised = 1,\s*BeamformerHipSpatialMode_Count", header)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="needs the ROCm LLVM binutils")
def test_the_kernels_design_lists_are_in_the_library_without_spills_or_scratch():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "spatial_row_kernel" in design and "spatial_run_kernel" in design
    kernels = [k for k in kernel_resources.kernels_of(lib.LIBRARY_PATH) if "spatial_" in k["demangled"]]
    names = sorted(k["demangled"].split("(")[0] for k in kernels)
    assert len(kernels) == 12, names                                     # row / run x complex / real x Zero / Normalised first / Normalised later
    assert sum("spatial_row_kernel" in n for n in names) == 6 and sum("spatial_run_kernel" in n for n in names) == 6
    for k in kernels:
        print(f"  {k['demangled'].split('(')[0]}: {k['vgpr_count']} VGPRs, {k['group_segment_fixed_size']} bytes of LDS")
        assert not k["vgpr_spill_count"] and not k["private_segment_fixed_size"], k["demangled"]
        assert k["vgpr_count"] <= 128, k["demangled"]                     # four waves a SIMD at the least
        if "spatial_run_kernel" in k["demangled"]:
            assert not k["group_segment_fixed_size"], k["demangled"]
        else:
            assert 0 < k["group_segment_fixed_size"] <= 768 * 12, k["demangled"]        # 768 voxels of 8 bytes and their D


def floats(values):
    return (C.c_float * len(values))(*values)


def call(L, count, taps, counts, mode, first, ms):
    pointers = None if taps is None else (C.POINTER(C.c_float) * 3)(*[None if h is None else C.cast(h, C.POINTER(C.c_float)) for h in taps])
    tap_counts = None if counts is None else (C.c_uint32 * 3)(*counts)
    return getattr(L, NAME)(count, pointers, tap_counts, mode, 0, None if first is None else C.byref(first), None if ms is None else C.byref(ms))


def test_every_refusal_that_needs_no_device():
    L = lib.library()
    L.beamformer_hip_shutdown()                       # (no device in use from here on: none of the calls below starts one)
    first, ms = C.c_uint32(77), C.c_float(-1.0)
    h3, h33 = floats([0.25, 0.5, 0.25]), floats([1.0 / 33] * 33)

    def refused(kind, count=2, taps=(h3, None, h3), counts=(3, 0, 3), mode=0):
        assert not call(L, count, taps, counts, mode, first, ms)
        assert lib.last_error()[0] == kind
        assert first.value == 77 and ms.value == -1.0

    # (the count, the outputs and the good call without a device: tests/test_frame_ops_contract_host.py)
    refused(E.BufferOverflow, count=0, taps=None, counts=None)         # BufferOverflow on count is decided before the taps are looked at
    refused(E.BufferOverflow, taps=(floats([0.0] * 35), None, None), counts=(35, 0, 0))
    refused(E.BufferOverflow, counts=(3, 0, TAPS + 1))
    refused(E.InvalidAccess, taps=None)
    refused(E.InvalidAccess, counts=None)
    refused(E.InvalidAccess, counts=(2, 0, 3))                          # an even count
    refused(E.InvalidAccess, taps=(h33, None, None), counts=(32, 0, 0))
    refused(E.InvalidAccess, taps=(h3, None, None), counts=(3, 0, 3))   # a NULL axis with a nonzero count
    refused(E.InvalidAccess, taps=(h3, h3, h3), counts=(0, 0, 0))       # nothing to do
    refused(E.InvalidAccess, taps=(None, None, None), counts=(0, 0, 0))
    refused(E.InvalidAccess, mode=2)
    refused(E.InvalidAccess, mode=0xFFFFFFFF)
    for bad in (float("nan"), float("inf"), float("-inf")):
        for at in (0, 1, 2):
            refused(E.InvalidAccess, taps=(h3, None, floats([bad if n == at else 0.5 for n in range(3)])))
    refused(E.InvalidAccess, taps=(h3, None, floats([0.5, -1e-30, 0.5])), mode=1)     # a negative tap, Normalised mode only
    refused(E.InvalidAccess, taps=(floats([-1.0]), None, None), counts=(1, 0, 0), mode=1)
    # the limits themselves are legal: no device yet, so there is no frame
    refused(E.InvalidAccess, taps=(h3, None, floats([0.5, -1.0, 0.5])))              # negative taps are Zero mode's right
    refused(E.InvalidAccess, taps=(h33, h33, h33), counts=(33, 33, 33), count=MAX)
    with pytest.raises(lib.BeamformerError):
        lib.convolve_last_frames(1, [None, np.ones(3), np.ones(5)], mode=P.HipSpatialMode.Normalised)
    with pytest.raises(ValueError):
        lib.convolve_last_frames(2, [[1.0], None])


# ---- the reference by hand ----

def test_the_reference_by_hand():
    f = np.array([[[1.0, 2.0, 4.0, 8.0]]], np.float32)
    # a true convolution: taps (0, 0, 1) move the frame by +1 voxel, (1, 0, 0) by -1
    out, bound = ref.convolve(f, ([0, 0, 1], None, None))
    assert out.dtype == np.float64 and np.array_equal(out[0, 0], [0, 1, 2, 4])
    assert np.array_equal(bound[0, 0], 5 * ref.U * np.array([0, 1, 2, 4]))
    assert np.array_equal(ref.convolve(f, ([1, 0, 0], None, None))[0][0, 0], [2, 4, 8, 0])
    # asymmetric taps (1, 2, 3): g[i] = 1 f[i + 1] + 2 f[i] + 3 f[i - 1], the terms outside skipped
    out, bound = ref.convolve(f, ([1, 2, 3], None, None))
    assert np.array_equal(out[0, 0], [2 + 2, 4 + 4 + 3, 8 + 8 + 6, 16 + 12])
    assert np.array_equal(bound[0, 0], 5 * ref.U * out[0, 0])
    # the same frame as a column and as a stack: y and z taps
    assert np.array_equal(ref.convolve(f.reshape(1, 4, 1), (None, [1, 2, 3], None))[0][0, :, 0], out[0, 0])
    assert np.array_equal(ref.convolve(f.reshape(4, 1, 1), (None, None, [1, 2, 3]))[0][:, 0, 0], out[0, 0])
    # two passes: B_y = 5 u A_y(|g_x| + B_x) + A_y(B_x)
    g = np.array([[[1.0, 2.0], [3.0, 5.0]]], np.float32)
    out, bound = ref.convolve(g, ([1, 1, 1], [2, 0, 0], None))
    assert np.array_equal(out[0], [[16, 16], [0, 0]])
    bx = 5 * ref.U * 8
    assert bound[0, 0, 0] == 5 * ref.U * 2 * (8 + bx) + 2 * bx and bound[0, 1, 0] == 0
    # NaN, Zero mode: the support is poisoned, a zero tap's position included; a complex voxel's parts apart
    c = np.array([[[1 + 1j, np.nan + 2j, 3 + 3j, 4 + 4j]]], np.complex64)
    out, _ = ref.convolve(c, ([0, 1, 1], None, None))
    assert np.array_equal(np.isnan(out.real[0, 0]), [True, True, True, False]) and not np.isnan(out.imag).any()
    assert np.array_equal(out.imag[0, 0], [1, 3, 5, 7])
    # NaN, Normalised mode: the voxel counts as missing in both parts, the hole is filled, a constant stays constant up to the edges
    out, bound = ref.convolve(c, ([1, 2, 1], None, None), ref.NORMALISED)
    assert np.array_equal(out[0, 0], [1 + 1j, (1 + 1j + 3 + 3j) / 2, (6 + 6j + 4 + 4j) / 3, (3 + 3j + 8 + 8j) / 3])
    assert np.isfinite(bound.real).all() and (bound.real > 0).all()
    ones = np.ones((3, 4, 5), np.float32)
    ones[1, 2, 3] = np.inf
    out, bound = ref.convolve(ones, ([1, 2, 1], [0.5, 0.5, 3], [1, 1, 1, 1, 1]), ref.NORMALISED)
    assert np.abs(out - 1).max() < 1e-15 and bound.max() < 40 * ref.U
    # no finite voxel under a positive tap: 0 / 0
    hole = np.array([[[np.nan, np.nan, 1.0]]], np.float32)
    assert np.array_equal(np.isnan(ref.convolve(hole, ([0, 1, 1], None, None), ref.NORMALISED)[0][0, 0]), [True, True, False])


# ---- the reference on the device tests' kinds of input: a float32 restatement inside the bound, three mistakes outside it ----

def inputs():
    """(label, frame, taps, mode): frames of the device tests' shapes -- (z, y, x) of the plane (33, 1, 7), the volume (9, 5, 6), a real
    plane, the long rows -- with NaN holes in the Normalised cases"""
    rng = np.random.default_rng(9100)

    def frame(shape, cplx=True, holes=0):
        f = rng.standard_normal(shape) + 0.5
        if cplx:
            f = f + 1j * (rng.standard_normal(shape) - 0.5)
        f = f.astype(np.complex64 if cplx else np.float32)
        if holes:
            f.reshape(-1)[rng.choice(f.size, holes, replace=False)] = np.nan
        return f

    def taps(n, positive=False):
        h = rng.standard_normal(n) if not positive else rng.uniform(0.1, 1.0, n)
        return (h * np.linspace(1.0, 2.0, n)).astype(np.float32)           # asymmetric

    yield "plane", frame((7, 1, 33)), (taps(9), None, taps(3)), ref.ZERO
    yield "volume", frame((6, 5, 9)), (taps(3), taps(3), taps(5)), ref.ZERO
    yield "real", frame((7, 1, 33), cplx=False), (taps(33), None, taps(9)), ref.ZERO
    yield "rows", frame((5, 3, 273)), (taps(33), taps(3), taps(3)), ref.ZERO
    yield "plane normalised", frame((7, 1, 33), holes=20), (taps(9, True), None, taps(3, True)), ref.NORMALISED
    yield "volume normalised", frame((6, 5, 9), holes=30), (taps(3, True), taps(3, True), taps(5, True)), ref.NORMALISED
    yield "real normalised", frame((7, 1, 33), cplx=False, holes=20), (taps(5, True), None, taps(9, True)), ref.NORMALISED


def test_a_float32_restatement_stays_inside_the_bound():
    for label, frame, taps, mode in inputs():
        values, bound = ref.convolve(frame, taps, mode)
        got = ref.convolve_float32(frame, taps, mode)
        worst, inside = ref.share_of_bound(got, values, bound)
        finite = np.isfinite(values.real) & np.isfinite(values.imag)
        print(f"  {label}: float32 numpy at {worst:.3f} of the bound at the worst, {int((~finite).sum())} voxels not finite")
        assert inside and 0 < worst
        assert np.array_equal(np.isfinite(got.real) & np.isfinite(got.imag), finite)
        assert finite.mean() > 0.5


def moved_share(wrong, values, bound):
    parts = [(wrong.real, values.real, bound.real), (wrong.imag, values.imag, bound.imag)] if np.iscomplexobj(values) else [(wrong, values, bound)]
    shares = []
    for w, x, b in parts:
        f = np.isfinite(x) & np.isfinite(w)
        shares.append(float((np.abs(w[f] - x[f]) > b[f]).mean()))
    return min(shares)


def test_the_bound_tells_the_definition_from_three_mistakes():
    for label, frame, taps, mode in inputs():
        values, bound = ref.convolve(frame, taps, mode)
        mistakes = {"correlation": ref.convolve(frame, taps, mode, flip=True)[0], "centre off by one": ref.convolve(frame, taps, mode, centre=1)[0]}
        if mode == ref.NORMALISED:
            mistakes["plain tap sum"] = ref.convolve(frame, taps, mode, plain_sum=True)[0]
        for name, wrong in mistakes.items():
            share = moved_share(wrong, values, bound)
            print(f"  {label}, {name}: {share:.3f} of the floats leave the bound")
            assert share > 0.5, (label, name)
