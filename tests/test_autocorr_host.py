"""The slow-time autocorrelation on the CPU (beamformer_hip_autocorrelate_last_frames): the symbol is declared, exported and bound; the
kernel DESIGN 3.7d lists is in the library, sixteen instantiations without spills or scratch; every refusal that needs no device holds,
with its error kind, and leaves the outputs alone; and the numpy reference the device tests judge against (tests/autocorr_ref.py) gives a
case small enough to work out by hand, is far above its own bound on the device tests' shapes, and tells the definition from the two
mistakes nearest to it."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from ogl_beamforming_amd import lib
from ogl_beamforming_amd import params as P
from tests import autocorr_ref as ref
from tests.ring_frames import AUTOCORR_CASES as CASES, GRIDS, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = P.LibError
NAME = "beamformer_hip_autocorrelate_last_frames"
MAX = P.HIP_MAX_ENSEMBLE_FRAMES


def test_the_symbol_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "ogl_beamformer_hip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", lib.LIBRARY_PATH], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in nm.stdout.splitlines() if " T " in line}
    assert re.search(r"BEAMFORMER_LIB_EXPORT uint32_t " + NAME + r"\(", header)
    assert NAME in exported and NAME in lib.exported_symbols()
    assert len(getattr(lib.library(), NAME).argtypes) == 7
    assert re.search(r"#define BEAMFORMER_HIP_MAX_LAGS (\d+)u", header).group(1) == str(P.HIP_MAX_LAGS) == "4"


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="needs the ROCm LLVM binutils")
def test_the_kernel_design_lists_is_in_the_library_without_spills_or_scratch():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    assert "autocorr_kernel" in open(os.path.join(ROOT, "DESIGN.md")).read()
    kernels = [k for k in kernel_resources.kernels_of(lib.LIBRARY_PATH) if "autocorr_kernel" in k["demangled"]]    # (mangled where llvm-cxxfilt is missing)
    assert len(kernels) == 16, [k["demangled"] for k in kernels]               # lags 1 .. 4 x complex / real x weighted / identity
    for k in kernels:
        print(f"  {k['demangled'].split('(')[0]}: {k['vgpr_count']} VGPRs")
        assert not k["vgpr_spill_count"] and not k["private_segment_fixed_size"] and not k["group_segment_fixed_size"], k["demangled"]
        assert k["vgpr_count"] <= 128, k["demangled"]                         # four waves a SIMD at the least


def test_every_refusal_that_needs_no_device():
    L = lib.library()
    L.beamformer_hip_shutdown()                       # (no device in use from here on: none of the calls below starts one)
    first, ms = C.c_uint32(77), C.c_float(-1.0)
    good = (C.c_float * 8)(1, 0, 0, 0, 0, 0, 1, 0)

    def refused(kind, count=2, w=good, rows=2, lags=2):
        assert not getattr(L, NAME)(count, w, rows, lags, 0, C.byref(first), C.byref(ms))
        assert lib.last_error()[0] == kind
        assert first.value == 77 and ms.value == -1.0

    # (the count, the outputs, the lags against the rows and the good call without a device: tests/test_frame_ops_contract_host.py)
    for n in (0, MAX + 1):
        refused(E.BufferOverflow, rows=n)
    refused(E.InvalidAccess, lags=0xFFFFFFFF)
    refused(E.InvalidAccess, w=None, count=MAX, rows=MAX, lags=P.HIP_MAX_LAGS + 1)
    refused(E.InvalidAccess, w=None, count=1, rows=2, lags=1)  # the identity form with rows != count
    for bad in (float("nan"), float("inf"), float("-inf")):
        for at in (0, 3, 7):                                   # a real part, an imaginary part, the last float
            w = (C.c_float * 8)(*good)
            w[at] = bad
            refused(E.InvalidAccess, w=w)
    with pytest.raises(lib.BeamformerError):
        lib.autocorrelate_last_frames(2)                       # (the identity form through the helper)
    with pytest.raises(ValueError):
        lib.autocorrelate_last_frames(2, np.eye(3))


# ---- the reference by hand ----

def test_the_reference_on_three_rows_of_two_voxels_with_one_nan():
    f = [np.array([[[1 + 2j, np.nan + 0j]]], np.complex64), np.array([[[3 - 1j, 1 + 1j]]], np.complex64), np.array([[[0 + 1j, 2 + 0j]]], np.complex64)]
    out, bound = ref.autocorrelate(f, None, 3)
    assert out.shape == bound.shape == (3, 1, 1, 2) and out.dtype == np.complex128
    # R_0 = 5 + 10 + 1; R_1 = conj(1+2j)(3-1j) + conj(3-1j)(1j) = (1-7j) + (-1+3j) = -4j; R_2 = conj(1+2j)(1j) = 2 + 1j
    assert np.array_equal(out[:, 0, 0, 0], np.array([16, -4j, 2 + 1j]))
    assert np.isnan(out[:, 0, 0, 1].real).all() and np.isnan(out[:, 0, 0, 1].imag).all()      # lag 0's imaginary part too
    # the identity form: e = 0, a = (3, 4, 1): (2N + 2) u sum a_n a_(n+L)
    assert np.array_equal(bound[:, 0, 0, 0], np.array([8 * 26, 6 * 16, 4 * 3]) * 2.0 ** -24)
    # weights: rows (f0 + f1, 1j f2) -> y = (4 + 1j, -1); e_n = (2K + 2) u sum (|Wre| + |Wim|)(|re| + |im|) = 8 u (3 + 4), 8 u 1
    W = np.array([[1, 1, 0], [0, 0, 1j]], np.complex64)
    out, bound = ref.autocorrelate(f, W, 2)
    assert np.array_equal(out[:, 0, 0, 0], np.array([17 + 1, np.conj(4 + 1j) * -1]))
    u = 2.0 ** -24
    a0, a1, e0, e1 = 5.0, 1.0, 56 * u, 8 * u
    assert bound[1, 0, 0, 0] == 4 * u * ((a0 + e0) * (a1 + e1) + e0 * e1) + (a0 * e1 + a1 * e0 + 2 * e0 * e1)
    assert bound[0, 0, 0, 0] == 6 * u * (((a0 + e0) ** 2 + e0 * e0) + ((a1 + e1) ** 2 + e1 * e1)) + ((2 * a0 * e0 + 2 * e0 * e0) + (2 * a1 * e1 + 2 * e1 * e1))
    # real frames: float64, y_n y_(n+L)
    r = [np.array([[[1.0, np.inf]]], np.float32), np.array([[[2.0, 1.0]]], np.float32), np.array([[[-3.0, 1.0]]], np.float32)]
    out, bound = ref.autocorrelate(r, None, 2)
    assert out.dtype == np.float64 and np.array_equal(out[:, 0, 0, 0], [14.0, -4.0]) and not np.isfinite(out[:, 0, 0, 1]).any()


# ---- the reference on the device tests' shapes: above its bound, and apart from the mistakes nearest to the definition ----

def synthetic(which, K):
    """float32 frames of the grid's shape and kind from the seed tests/test_gpu_ensemble.py draws the ensemble's RF from"""
    points, iq = ((24, 1, 40), True) if which == "nan" else (GRIDS[which][0], GRIDS[which][3])      # "nan": the frame metrics tests' block D
    rng = np.random.default_rng(7600 + K)
    shape = (K,) + points[::-1]
    if iq:
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
    return rng.standard_normal(shape).astype(np.float32)


def inputs():
    """(label, frames, W, lags) of every value test of tests/test_gpu_autocorr.py"""
    for which in ("plane", "volume"):
        for K, rows, lags in CASES:
            yield f"{which} {K} {rows} {lags}", synthetic(which, K), weights(rows, K, 8100 + 100 * K + rows), lags
        yield f"{which} identity", synthetic(which, 17), None, 4
    yield "reversed", synthetic("plane", 5), weights(17, 5, 8200), 2
    yield "composition", synthetic("volume", 17), weights(17, 17, 8300), 4
    yield "repeat", synthetic("plane", 17), weights(33, 17, 8400), 4
    yield "real", synthetic("real", 5), weights(17, 5, 8500, real=True), 4
    yield "real identity", synthetic("real", 5), None, 3
    yield "nan", synthetic("nan", 5), weights(17, 5, 8600), 4


def shares(values, bound):
    """per lag and part, the share of the finite elements whose magnitude exceeds the bound (lag 0's imaginary part left out)"""
    out = {}
    for lag in range(len(values)):
        for name, part in (("re", np.real(values[lag])), ("im", np.imag(values[lag]))):
            if name == "im" and (lag == 0 or not np.iscomplexobj(values)):
                continue
            finite = np.isfinite(part)
            out[(lag, name)] = float((np.abs(part[finite]) > bound[lag][finite]).mean())
    return out


def test_the_expected_values_exceed_the_bound_on_the_device_tests_inputs():
    for label, frames, W, lags in inputs():
        values, bound = ref.autocorrelate(list(frames), W, lags)
        s = shares(values, bound)
        print(f"  {label}: |expected| > bound on {min(s.values()):.3f} of the elements at the least ({len(s)} lag parts)")
        assert min(s.values()) > 0.5, (label, s)
        assert not np.imag(values[0]).any()


def test_the_bound_tells_the_definition_from_the_conjugate_on_the_other_operand_and_from_a_lag_off_by_one():
    for label, frames, W, lags in inputs():
        values, bound = ref.autocorrelate(list(frames), W, lags)
        y, _ = ref.filtered(list(frames), W)
        shape = values.shape
        shifted = ref.lag_products(y, lags, shift=1).reshape(shape) if y.shape[0] > lags else None
        swapped = ref.lag_products(y, lags, conj_second=True).reshape(shape)
        for lag in range(lags):
            if shifted is not None:
                moved = np.maximum(np.abs(np.real(shifted[lag] - values[lag])), np.abs(np.imag(shifted[lag] - values[lag])))
                assert (moved > bound[lag]).mean() > 0.5, (label, lag, "shift")
            if lag and np.iscomplexobj(values):
                moved = np.abs(np.imag(swapped[lag] - values[lag]))
                assert (moved > bound[lag]).mean() > 0.5, (label, lag, "conj")
    print("  every lag moves by more than its bound on more than half of the elements under either mistake")
