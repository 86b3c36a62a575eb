"""The ensemble filter on the CPU (beamformer_hip_gram_last_frames, beamformer_hip_clutter_projector, beamformer_hip_mix_last_frames):
the three symbols are exported and bound; the struct the binding mirrors is the header's, field by field, as gcc lays it out; the
kernels DESIGN 3.7c lists are in the library without spills or scratch; every refusal that needs no device holds, with its error kind,
and leaves the outputs alone; the host-only projector reproduces constructed projectors within the float32 rounding of its entries; and
the numpy reference the device tests judge against (tests/ensemble_ref.py) gives a case small enough to work out by hand."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from ogl_beamforming_amd import lib
from ogl_beamforming_amd import params as P
from tests import ensemble_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = P.LibError
SYMBOLS = ("beamformer_hip_gram_last_frames", "beamformer_hip_clutter_projector", "beamformer_hip_mix_last_frames")
MAX = P.HIP_MAX_ENSEMBLE_FRAMES


def test_the_three_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "ogl_beamformer_hip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", lib.LIBRARY_PATH], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in nm.stdout.splitlines() if " T " in line}
    for name in SYMBOLS:
        assert re.search(r"BEAMFORMER_LIB_EXPORT uint32_t " + name + r"\(", header), name
        assert name in exported and name in lib.exported_symbols(), name
        assert getattr(lib.library(), name).argtypes is not None


def test_the_struct_is_the_headers_field_by_field(tmp_path):
    name, cls = "BeamformerHipEnsembleInfo", P.HipEnsembleInfo
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ogl_beamformer_hip.h"', 'int main(void) {',
             f'printf("{name} %zu\\n", sizeof({name}));']
    for field, _ in cls._fields_:
        lines.append(f'printf("{name}.{field} %zu\\n", offsetof({name}, {field}));')
    lines += ['printf("MAX %u\\n", BEAMFORMER_HIP_MAX_ENSEMBLE_FRAMES);', 'return 0; }']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    printed = dict(line.split(" ", 1) for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert C.sizeof(cls) == int(printed[name]) == sum(C.sizeof(t) for _, t in cls._fields_) == 64          # no padding
    for field, _ in cls._fields_:
        assert getattr(cls, field).offset == int(printed[f"{name}.{field}"]), field
    assert [f for f, _ in cls._fields_] == ["count", "data_kind", "points", "region_first", "region_count", "first_frame_id", "voxels", "non_finite"]
    assert int(printed["MAX"]) == MAX == 256


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="needs the ROCm LLVM binutils")
def test_the_kernels_design_lists_are_in_the_library_without_spills_or_scratch():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    listed = set(re.findall(r"\b(?:gram_[a-z]+_kernel|mix_kernel)\b", open(os.path.join(ROOT, "DESIGN.md")).read()))
    assert listed == {"gram_mask_kernel", "gram_partial_kernel", "gram_fold_kernel", "mix_kernel"}, listed
    kernels = [k for k in kernel_resources.kernels_of(lib.LIBRARY_PATH) if re.search(r"gram_[a-z]+_kernel|mix_kernel", k["demangled"])]    # (mangled where llvm-cxxfilt is missing)
    assert len(kernels) == 5, [k["demangled"] for k in kernels]                # mix_kernel<true> and mix_kernel<false>
    for want in listed:
        assert any(want in k["demangled"] for k in kernels), want
    for k in kernels:
        assert not k["vgpr_spill_count"] and not k["private_segment_fixed_size"], k["demangled"]


def test_every_refusal_of_the_device_calls_that_needs_no_device():
    L = lib.library()
    L.beamformer_hip_shutdown()                       # (no device in use from here on: none of the calls below starts one)
    gram = (C.c_double * 8)(*([-7.0] * 8))
    info = P.HipEnsembleInfo()
    C.memset(C.byref(info), 0x5A, C.sizeof(info))
    untouched = bytes(gram), bytes(info)
    first, ms = C.c_uint32(77), C.c_float(-1.0)

    def gram_refused(kind, count=2, out=gram):
        assert not L.beamformer_hip_gram_last_frames(count, None, out, C.byref(info), C.byref(ms))
        assert lib.last_error()[0] == kind
        assert (bytes(gram), bytes(info)) == untouched and ms.value == -1.0

    # (the count, the outputs and the good call without a device, of both calls: tests/test_frame_ops_contract_host.py)
    gram_refused(E.InvalidAccess, out=None)                    # the matrix alone missing
    region = lib.frame_region((0, 0, 0), (1, 1, 1))
    assert not L.beamformer_hip_gram_last_frames(1, C.byref(region), gram, None, None) and lib.last_error()[0] == E.InvalidAccess
    assert bytes(gram) == untouched[0]

    good = (C.c_float * 8)(1, 0, 0, 0, 0, 0, 1, 0)

    def mix_refused(kind, count=2, weights=good, out_count=2):
        assert not L.beamformer_hip_mix_last_frames(count, weights, out_count, 0, C.byref(first), C.byref(ms))
        assert lib.last_error()[0] == kind
        assert first.value == 77 and ms.value == -1.0

    for n in (0, MAX + 1):
        mix_refused(E.BufferOverflow, out_count=n)
    mix_refused(E.BufferOverflow, count=0, weights=None)       # BufferOverflow on count is decided before the weights are looked at
    mix_refused(E.InvalidAccess, weights=None)
    for bad in (float("nan"), float("inf"), float("-inf")):
        for at in (0, 3, 7):                                   # a real part, an imaginary part, the last float
            w = (C.c_float * 8)(*good)
            w[at] = bad
            mix_refused(E.InvalidAccess, weights=w)


def test_every_refusal_of_the_projector():
    L = lib.library()
    g = (C.c_double * 8)(2, 0, 0.5, 0.25, 0.5, -0.25, 1, 0)
    w = (C.c_float * 8)(*([-7.0] * 8))
    values = (C.c_double * 2)(-7.0, -7.0)
    untouched = bytes(w), bytes(values)

    def refused(kind, gram=g, count=2, hi=1, lo=0, weights=w):
        assert not L.beamformer_hip_clutter_projector(gram, count, hi, lo, weights, values)
        assert lib.last_error()[0] == kind
        assert (bytes(w), bytes(values)) == untouched

    refused(E.InvalidAccess, gram=None)
    refused(E.InvalidAccess, weights=None)
    for count in (0, MAX + 1):
        refused(E.BufferOverflow, count=count)
    refused(E.InvalidAccess, hi=3)
    refused(E.InvalidAccess, hi=2, lo=1)
    refused(E.InvalidAccess, hi=0xFFFFFFFF, lo=2)              # (the sum is not taken in 32 bits)
    for bad in (float("nan"), float("inf")):
        for at in (0, 2, 3, 6):                                # the upper triangle: [0][0].re, [0][1].re, [0][1].im, [1][1].re
            m = (C.c_double * 8)(*g)
            m[at] = bad
            refused(E.InvalidAccess, gram=m)
    # what is not read may be anything: the lower triangle and the diagonal's imaginary parts
    m = (C.c_double * 8)(*g)
    m[1] = m[4] = m[5] = m[7] = float("nan")
    assert L.beamformer_hip_clutter_projector(m, 2, 1, 0, w, values)
    expect, lam = ref.projector(np.array([[2, 0.5 + 0.25j], [0.5 - 0.25j, 1]]), 1)
    assert np.abs(np.frombuffer(w, np.complex64).reshape(2, 2) - expect).max() <= 2.0 ** -23
    assert np.abs(np.frombuffer(values, np.float64) - lam).max() <= 64 * 2 * 2.0 ** -53 * lam.max()
    assert L.beamformer_hip_clutter_projector(g, 2, 1, 0, w, None)            # eigenvalues may be NULL


# ---- the projector against constructed spectra ----

def constructed(K, seed):
    """G = U diag(lambda) U^H, U from a QR of a seeded complex Gaussian: lambda_i = 2^-i (K = 65: eight such values, then a near-flat tail)"""
    rng = np.random.default_rng(seed)
    U, _ = np.linalg.qr(rng.standard_normal((K, K)) + 1j * rng.standard_normal((K, K)))
    lam = 2.0 ** -np.arange(K, dtype=np.float64)
    geometric = K
    if K == 65:
        geometric = 8
        lam[8:] = 2.0 ** -9 * (1.0 + 1e-3 * np.arange(K - 8, dtype=np.float64)[::-1])
    return (U * lam) @ U.conj().T, U, lam, geometric


@pytest.mark.parametrize("K", [3, 8, 17, 65])
def test_the_projector_reproduces_constructed_projectors(K):
    G, U, lam, geometric = constructed(K, 100 + K)
    cuts = [(1, 0), (2, 0), (5, 0), (2, 3), (0, 0), (K, 0)]
    ran = 0
    for hi, lo in cuts:
        # a cut lies inside the geometric part of the spectrum (or removes nothing / everything), where the gap is at least 2^-8 ||G||:
        # a low cut drops the near-flat tail whole, and `lo` components of the geometric part with it
        if lo:
            lo += K - geometric
        if hi + lo > K or (0 < hi < K and hi > geometric):
            continue
        ran += 1
        W, values = lib.clutter_projector(G, hi, lo)
        kept = U[:, hi:K - lo]
        truth = kept @ kept.conj().T
        assert W.dtype == np.complex64 and W.shape == (K, K) and values.shape == (K,)
        assert np.abs(W.astype(np.complex128) - truth).max() <= 2.0 ** -23, (K, hi, lo)
        assert np.abs(values - lam).max() <= 64 * K * 2.0 ** -53 * lam.max(), (K, hi, lo)
        assert (np.diff(values) <= 0).all()
        # the reference itself is far inside the bar
        assert np.abs(ref.projector(G, hi, lo)[0] - truth).max() <= 1e-10
        W = W.astype(np.complex128)
        assert np.abs(W - W.conj().T).max() <= 2.0 ** -21 and np.abs(W @ W - W).max() <= 2.0 ** -21
        if (hi, lo) == (0, 0):
            assert np.abs(W - np.eye(K)).max() <= 2.0 ** -23
        if (hi, lo) == (K, 0):
            assert not W.any()
    assert ran == (4 if K == 3 else 6), ran


def test_a_real_symmetric_matrix_gives_imaginary_parts_of_exactly_zero():
    rng = np.random.default_rng(7)
    Q, _ = np.linalg.qr(rng.standard_normal((17, 17)))
    lam = 2.0 ** -np.arange(17, dtype=np.float64)
    G = (Q * lam) @ Q.T
    G = (G + G.T) / 2
    for hi, lo in ((1, 0), (2, 3), (0, 0)):
        W, values = lib.clutter_projector(G, hi, lo)
        assert not W.imag.any()
        assert np.abs(W.real - Q[:, hi:17 - lo] @ Q[:, hi:17 - lo].T).max() <= 2.0 ** -23
        assert np.abs(values - lam).max() <= 64 * 17 * 2.0 ** -53


# ---- the reference by hand ----

def test_the_reference_on_two_frames_of_three_voxels_with_one_nan():
    f0 = np.array([[[1 + 2j, 3 - 1j, np.nan + 0j]]], np.complex64)            # (z, y, x) = (1, 1, 3)
    f1 = np.array([[[2 - 1j, 0 + 1j, 5 + 5j]]], np.complex64)
    G, voxels, non_finite, bound = ref.gram([f0, f1])
    assert (voxels, non_finite) == (2, 1)
    # conj(1+2j)(2-1j) + conj(3-1j)(1j) = (1-2j)(2-1j) + (3+1j)(1j) = (0-5j) + (-1+3j) = -1-2j
    assert np.array_equal(G, np.array([[5 + 10, -1 - 2j], [-1 + 2j, 5 + 1]], np.complex128))
    assert np.array_equal(bound, 4 * 2.0 ** -53 * np.array([[9 + 16, 3 * 3 + 4 * 1], [3 * 3 + 4 * 1, 9 + 1]]))
    # the box that leaves the NaN voxel out, and the one that holds nothing else
    assert ref.gram([f0, f1], ((0, 0, 0), (2, 1, 1)))[1:3] == (2, 0)
    G2, voxels, non_finite, _ = ref.gram([f0, f1], ((2, 0, 0), (1, 1, 1)))
    assert (voxels, non_finite) == (0, 1) and not G2.any()
    W = np.array([[0, 1], [2, 1j], [0, 0]], np.complex64)
    out, bound = ref.mix([f0, f1], W)
    assert out.shape == (3, 1, 1, 3)
    assert np.array_equal(out[0, 0, 0, :2], f1[0, 0, :2]) and np.isnan(out[0, 0, 0, 2].real)       # 0 * NaN is NaN: no weight is skipped
    assert np.array_equal(out[1, 0, 0, :2], np.array([2 * (1 + 2j) + 1j * (2 - 1j), 2 * (3 - 1j) + 1j * 1j]))
    assert not out[2, 0, 0, :2].any() and np.isnan(out[2, 0, 0, 2].real) and np.isnan(out[2, 0, 0, 2].imag)
    assert bound[1, 0, 0, 0] == 6 * 2.0 ** -24 * (2 * 3 + 1 * 3)
    r0, r1 = np.array([[[1.0, np.inf]]], np.float32), np.array([[[2.0, 1.0]]], np.float32)
    G, voxels, non_finite, _ = ref.gram([r0, r1])
    assert (voxels, non_finite) == (1, 1) and np.array_equal(G, np.array([[1, 2], [2, 4]], np.complex128))
    out, _ = ref.mix([r0, r1], np.array([[0.5, -1.0]]))
    assert out.dtype == np.float64 and out[0, 0, 0, 0] == -1.5 and np.isinf(out[0, 0, 0, 1])
    P1, lam = ref.projector(np.diag([1.0, 4.0, 2.0]), 1)
    assert np.allclose(lam, [4, 2, 1]) and np.allclose(P1, np.diag([1.0, 0.0, 1.0]))
