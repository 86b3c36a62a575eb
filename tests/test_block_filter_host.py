"""The block-wise ensemble filter on the CPU (beamformer_hip_gram_boxes_last_frames, beamformer_hip_lattice_boxes,
beamformer_hip_mix_field_last_frames): the three symbols are declared, exported and bound; the constants of the binding are the
header's; the kernels DESIGN lists are in the library without spills or scratch; the exact float32 fmaf of the reference
(tests/block_filter_ref.py) agrees with rational arithmetic, constructed ties included; the host-only lattice_boxes gives the
reference's boxes and every one of its refusals; every refusal of the two device calls that needs no device holds, with its error kind,
and leaves the outputs alone; the segments of an axis small enough to work out by hand; and the two-clutter ensemble the device test
filters does separate a block-wise filter from a global one -- a condition on the inputs, checked here on the reference alone."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from ogl_beamforming_amd import lib
from ogl_beamforming_amd import params as P
from tests import block_filter_ref as ref
from tests import ensemble_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = P.LibError
SYMBOLS = ("beamformer_hip_gram_boxes_last_frames", "beamformer_hip_lattice_boxes", "beamformer_hip_mix_field_last_frames")
MAX = P.HIP_MAX_ENSEMBLE_FRAMES
F32 = np.float32
U3 = C.c_uint32 * 3


def test_the_three_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "ogl_beamformer_hip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", lib.LIBRARY_PATH], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in nm.stdout.splitlines() if " T " in line}
    for name in SYMBOLS:
        assert re.search(r"BEAMFORMER_LIB_EXPORT uint32_t " + name + r"\(", header), name
        assert name in exported and name in lib.exported_symbols(), name
        assert getattr(lib.library(), name).argtypes is not None
    for name in ("gram_boxes_last_frames", "lattice_boxes", "mix_field_last_frames"):
        assert callable(getattr(lib, name))


def test_the_constants_are_the_headers(tmp_path):
    names = {"BEAMFORMER_HIP_MAX_GRAM_BOXES": P.HIP_MAX_GRAM_BOXES, "BEAMFORMER_HIP_MAX_GRAM_BOX_ENTRIES": P.HIP_MAX_GRAM_BOX_ENTRIES,
             "BEAMFORMER_HIP_MAX_MIX_NODES": P.HIP_MAX_MIX_NODES, "BEAMFORMER_HIP_MAX_MIX_FIELD_ENTRIES": P.HIP_MAX_MIX_FIELD_ENTRIES}
    lines = ['#include <stdio.h>', '#include "ogl_beamformer_hip.h"', 'int main(void) {']
    lines += [f'printf("{name} %llu\\n", (unsigned long long){name});' for name in names]
    lines += ['return 0; }']
    src, exe = tmp_path / "constants.c", tmp_path / "constants"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    printed = dict(line.split(" ", 1) for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    for name, value in names.items():
        assert int(printed[name]) == value, name
    assert (P.HIP_MAX_GRAM_BOXES, P.HIP_MAX_GRAM_BOX_ENTRIES, P.HIP_MAX_MIX_NODES, P.HIP_MAX_MIX_FIELD_ENTRIES) == (1024, 1 << 22, 1024, 1 << 22)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="needs the ROCm LLVM binutils")
def test_the_kernels_design_lists_are_in_the_library_without_spills_or_scratch():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    pattern = r"blocks_[a-z]+_kernel|blend_(?:once_)?kernel"
    listed = set(re.findall(r"\b(?:" + pattern + r")\b", open(os.path.join(ROOT, "DESIGN.md")).read()))
    assert listed == {"blocks_mask_kernel", "blocks_partial_kernel", "blocks_fold_kernel", "blend_kernel", "blend_once_kernel"}, listed
    kernels = [k for k in kernel_resources.kernels_of(lib.LIBRARY_PATH) if re.search(pattern, k["demangled"])]
    assert len(kernels) == 7, [k["demangled"] for k in kernels]                # blend_kernel and blend_once_kernel: <true> and <false>
    for want in listed:
        assert any(want in k["demangled"] for k in kernels), want
    for k in kernels:
        assert not k["vgpr_spill_count"] and not k["private_segment_fixed_size"], k["demangled"]


# ---- the exact fmaf ----

def nearest_float32(exact):
    """the float32 nearest to a Fraction, ties to the even significand; infinity past the overflow threshold"""
    if exact == 0:
        return F32(0)
    if abs(exact) >= Fraction(ref.OVERFLOW_TIE):
        return F32(np.inf) if exact > 0 else F32(-np.inf)
    start = F32(float(exact))                                    # (within an ulp: the candidates are it and its two neighbours)
    if not np.isfinite(start):
        start = F32(np.finfo(F32).max) if exact > 0 else F32(-np.finfo(F32).max)
    with np.errstate(over="ignore"):
        candidates = {float(start), float(np.nextafter(start, F32(np.inf))), float(np.nextafter(start, F32(-np.inf)))}
    candidates = [c for c in candidates if np.isfinite(c)]
    best = min(abs(Fraction(c) - exact) for c in candidates)
    nearest = [c for c in candidates if abs(Fraction(c) - exact) == best]
    if len(nearest) == 2:
        nearest = [c for c in nearest if (int(np.array(c, F32).view(np.uint32)) & 1) == 0]
    assert len(nearest) == 1
    return F32(nearest[0])


def constructed_ties(rng, n):
    """triples whose product p = a * b is EXACTLY a float32 midpoint (two odd integers whose product has 25 bits, scaled by powers of
    two) and whose c is far below the last bit of a double at p: the float64 sum is p, the residual is c, on either side"""
    out = []
    while len(out) < n:
        a, b = int(rng.integers(1 << 12, 1 << 13)) | 1, int(rng.integers(1 << 11, 1 << 13)) | 1
        if not (1 << 24) <= a * b < (1 << 25):
            continue
        ea, eb = (int(v) for v in rng.integers(-20, 20, 2))
        sign = 1.0 if rng.random() < 0.5 else -1.0
        c = float(rng.choice([-1.0, 1.0])) * float(rng.uniform(1.0, 2.0)) * 2.0 ** (ea + eb - 70)
        out.append((F32(sign * a * 2.0 ** ea), F32(b * 2.0 ** eb), F32(c)))
    return out


def test_the_exact_fmaf_agrees_with_rational_arithmetic():
    rng = np.random.default_rng(4100)
    triples = []
    for scale in (1.0, 1e-3, 1e20, 1e-30):                       # ordinary numbers, cancellation, near overflow, near the subnormals
        a, b = rng.standard_normal(600).astype(F32), (scale * rng.standard_normal(600)).astype(F32)
        c = np.where(rng.random(600) < 0.5, -(a.astype(np.float64) * b).astype(F32) * F32(1 + 2.0 ** -20), (scale * rng.standard_normal(600)).astype(F32))
        triples += list(zip(a, b, c.astype(F32)))
    ties = constructed_ties(rng, 600)
    triples += ties
    triples += [(F32(np.finfo(F32).max), F32(1), F32(2.0 ** 103)), (F32(np.finfo(F32).max), F32(1), np.nextafter(F32(2.0 ** 103), F32(0))),
                (F32(2.0 ** -100), F32(2.0 ** -49), F32(0)), (F32(2.0 ** -100), F32(2.0 ** -50), F32(2.0 ** -149)), (F32(3), F32(2.0 ** -150), F32(2.0 ** -149))]
    a, b, c = (np.array(v, F32) for v in zip(*triples))
    got = ref.fmaf(a, b, c)
    with np.errstate(over="ignore"):
        double_rounded = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)
    differ = 0
    for n, (x, y, z) in enumerate(triples):
        want = nearest_float32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z)))
        assert got[n].view(np.uint32) == want.view(np.uint32) or (got[n] == 0 and want == 0), (n, x, y, z, got[n], want)
        differ += int(double_rounded[n] != want)
    # the constructed ties are ties: the sum rounded twice goes wrong on about half of them, on either side
    tie_errors = int((double_rounded[2400:3000] != got[2400:3000]).sum())
    print(f"  {len(triples)} triples, {differ} of them rounded wrongly by the float64 sum rounded again ({tie_errors} of the 600 constructed ties)")
    assert len(triples) >= 3000 and 200 <= tie_errors <= 400
    up = sum(1 for n in range(2400, 3000) if double_rounded[n] != got[n] and abs(got[n]) > abs(double_rounded[n]))
    assert 0 < up < tie_errors
    # plain IEEE for what is not finite
    odd = ref.fmaf(np.array([np.inf, np.nan, 0.0, 1.0], F32), np.array([1.0, 1.0, np.inf, 1.0], F32), np.array([1.0, 1.0, 1.0, -np.inf], F32))
    assert np.isposinf(odd[0]) and np.isnan(odd[1]) and np.isnan(odd[2]) and np.isneginf(odd[3])


# ---- lattice_boxes ----

def boxes_of(regions):
    return [(tuple(r.first), tuple(r.count)) for r in regions]


LATTICES = [((64, 1, 64), (3, 1, 4), (5, 0, 3), (23, 1, 17), (8, 0, 8)),        # clipped at x = 0 (5 - 8) and at z = 64 (54 + 8 + 1)
            ((33, 1, 7), (2, 1, 1), (0, 0, 0), (40, 1, 1), (10, 0, 3)),         # the last node beyond the frame, its box still reaches it
            ((9, 5, 6), (2, 2, 3), (2, 1, 0), (5, 3, 2), (1, 1, 1)),
            ((9, 5, 6), (1, 1, 1), (4, 2, 3), (0, 0, 0), (100, 100, 100)),      # one node: the step is not read, the box is the frame
            ((7, 1, 1), (2, 3, 1), (2, 0, 0), (3, 5, 1), (1, 0, 0)),            # N > 1 on an axis of 1 point: half 10 would reach, 0 does not
            ((0xFFFFFFFF, 1, 2), (2, 1, 1), (0xFFFFFFF0, 0, 0), (0xFFFFFFFF, 1, 1), (0xFFFFFFFF, 0, 0))]   # 64-bit positions


def test_lattice_boxes_against_the_reference():
    for points, nodes, first, step, half in LATTICES:
        try:
            want = ref.lattice_boxes(points, nodes, first, step, half)
        except ValueError as error:
            want = str(error)
        if isinstance(want, str):
            with pytest.raises(lib.BeamformerError):
                lib.lattice_boxes(points, nodes, first, step, half)
            assert lib.last_error()[0] == getattr(E, want)
            continue
        got = boxes_of(lib.lattice_boxes(points, nodes, first, step, half))
        print(f"  {points} nodes {nodes} first {first} step {step} half {half}: {got[:4]}{' ...' if len(got) > 4 else ''}")
        assert got == want
    # by hand: 64 points, nodes at 5, 28, 51, half 8 -> [0, 14), [20, 37), [43, 60)
    got = boxes_of(lib.lattice_boxes((64, 1, 64), (3, 1, 1), (5, 0, 3), (23, 1, 17), (8, 0, 8)))
    assert got == [((0, 0, 0), (14, 1, 12)), ((20, 0, 0), (17, 1, 12)), ((43, 0, 0), (17, 1, 12))]
    # the case above whose middle row of nodes misses the frame is a refusal; with a reach of 10 it is none
    assert isinstance(ref.lattice_boxes((7, 1, 1), (2, 3, 1), (2, 0, 0), (3, 5, 1), (1, 10, 0)), list)


def test_every_refusal_of_lattice_boxes():
    L = lib.library()
    regions = (P.HipFrameRegion * 4)()
    C.memset(regions, 0x5A, C.sizeof(regions))
    untouched = bytes(regions)
    good = dict(points=U3(9, 5, 6), nodes=U3(2, 2, 1), first=U3(1, 1, 0), step=U3(4, 2, 0), half=U3(1, 1, 1))

    def refused(kind, out=regions, **change):
        a = dict(good, **change)
        assert not L.beamformer_hip_lattice_boxes(a["points"], a["nodes"], a["first"], a["step"], a["half"], out)
        assert lib.last_error()[0] == kind and bytes(regions) == untouched

    assert L.beamformer_hip_lattice_boxes(good["points"], good["nodes"], good["first"], good["step"], good["half"], regions)
    assert boxes_of(regions) == ref.lattice_boxes((9, 5, 6), (2, 2, 1), (1, 1, 0), (4, 2, 0), (1, 1, 1))
    C.memset(regions, 0x5A, C.sizeof(regions))
    for name in good:
        refused(E.InvalidAccess, **{name: None})
    refused(E.InvalidAccess, out=None)
    for at in range(3):
        for name in ("points", "nodes"):
            values = list(good[name])
            values[at] = 0
            refused(E.InvalidAccess, **{name: U3(*values)})
    refused(E.InvalidAccess, step=U3(0, 2, 0))                  # a step of 0 on an axis of two nodes (on the axis of one node it is not read)
    refused(E.InvalidAccess, step=U3(4, 0, 0))
    refused(E.InvalidAccess, first=U3(11, 1, 0))                # the box of node 0 along x, [10, 13), misses the 9 points
    refused(E.InvalidAccess, step=U3(4, 6, 0))                  # the box of node 1 along y, [6, 9), misses the 5 points
    refused(E.BufferOverflow, nodes=U3(1025, 1, 1))
    refused(E.BufferOverflow, nodes=U3(33, 32, 1))
    refused(E.BufferOverflow, nodes=U3(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF))


# ---- the device calls without a device ----

def test_every_refusal_of_the_device_calls_that_needs_no_device():
    L = lib.library()
    L.beamformer_hip_shutdown()                       # (no device in use from here on: none of the calls below starts one)
    grams = (C.c_double * 16)(*([-7.0] * 16))
    infos = (P.HipEnsembleInfo * 2)()
    C.memset(infos, 0x5A, C.sizeof(infos))
    untouched = bytes(grams), bytes(infos)
    boxes = (P.HipFrameRegion * 2)(lib.frame_region((0, 0, 0), (1, 1, 1)), lib.frame_region((1, 0, 0), (2, 1, 1)))
    first, ms = C.c_uint32(77), C.c_float(-1.0)

    def gram_refused(kind, count=2, regions=boxes, region_count=2, out=grams):
        assert not L.beamformer_hip_gram_boxes_last_frames(count, regions, region_count, out, infos, C.byref(ms))
        assert lib.last_error()[0] == kind
        assert (bytes(grams), bytes(infos)) == untouched and ms.value == -1.0

    # (the count, the number of boxes, the outputs and the good call without a device, of both calls: tests/test_frame_ops_contract_host.py)
    gram_refused(E.BufferOverflow, count=65, region_count=1024)          # 1024 x 65 x 65 entries: more than 2^22 (64 x 64 is exactly the cap)
    gram_refused(E.BufferOverflow, region_count=0, regions=None)
    gram_refused(E.InvalidAccess, out=None)
    gram_refused(E.InvalidAccess, regions=None)
    gram_refused(E.InvalidAccess, count=64, region_count=1024, regions=(P.HipFrameRegion * 1024)())     # at the cap: past the limits, no device
    assert not L.beamformer_hip_gram_boxes_last_frames(2, boxes, 2, grams, None, None) and lib.last_error()[0] == E.InvalidAccess
    assert bytes(grams) == untouched[0]

    good = (C.c_float * 16)(1, 0, 0, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0)           # two nodes, M = K = 2
    lattice = dict(nodes=U3(2, 1, 1), node_first=U3(1, 0, 0), node_step=U3(3, 0, 0))

    def mix_refused(kind, count=2, weights=good, out_count=2, **change):
        a = dict(lattice, **change)
        assert not L.beamformer_hip_mix_field_last_frames(count, weights, a["nodes"], a["node_first"], a["node_step"], out_count, 0, C.byref(first), C.byref(ms))
        assert lib.last_error()[0] == kind
        assert first.value == 77 and ms.value == -1.0

    for n in (0, MAX + 1):
        mix_refused(E.BufferOverflow, out_count=n)
    mix_refused(E.BufferOverflow, count=0, weights=None)
    mix_refused(E.BufferOverflow, out_count=0, nodes=None)
    mix_refused(E.InvalidAccess, weights=None)
    for name in lattice:
        mix_refused(E.InvalidAccess, **{name: None})
    for at in range(3):
        values = [2, 1, 1]
        values[at] = 0
        mix_refused(E.BufferOverflow, nodes=U3(*values))
    mix_refused(E.BufferOverflow, nodes=U3(1025, 1, 1))
    mix_refused(E.BufferOverflow, nodes=U3(33, 32, 1), node_step=U3(1, 1, 1))
    mix_refused(E.BufferOverflow, nodes=U3(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), node_step=U3(1, 1, 1))
    mix_refused(E.BufferOverflow, count=65, out_count=64, nodes=U3(32, 1, 32), node_step=U3(1, 1, 1))    # 1024 x 64 x 65 entries: over the cap
    mix_refused(E.BufferOverflow, nodes=U3(0, 1, 1), node_step=U3(0, 0, 0))      # the lattice's size is judged before its steps
    mix_refused(E.InvalidAccess, node_step=U3(0, 0, 0))                          # a step of 0 on the axis of two nodes
    mix_refused(E.InvalidAccess, nodes=U3(1, 2, 1), node_step=U3(3, 0, 0))
    for bad in (float("nan"), float("inf"), float("-inf")):
        for at in (0, 3, 15):                                   # a real part, an imaginary part, the last float of the second node
            w = (C.c_float * 16)(*good)
            w[at] = bad
            mix_refused(E.InvalidAccess, weights=w)
    mix_refused(E.InvalidAccess, nodes=U3(1, 1, 1), node_step=U3(0, 0, 0), weights=(C.c_float * 8)(*good[:8]))   # one node: the step is not read
    with pytest.raises(ValueError):
        lib.mix_field_last_frames(2, np.eye(2), (0, 0, 0), (1, 1, 1))
    # the two hooks of these calls are the library's, through the one entry point
    assert L.beamformer_hip_set_hook(b"GRAM_BOXES_BUDGET", b"32768") and L.beamformer_hip_set_hook(b"GRAM_BOXES_BUDGET", None)
    assert L.beamformer_hip_set_hook(b"BLEND_SHAPE", b"1") and L.beamformer_hip_set_hook(b"BLEND_SHAPE", None)


# ---- the reference by hand ----

def test_the_segments_of_seven_voxels_with_nodes_at_two_and_five():
    lower, upper, t, blended = ref.segments(7, 2, 2, 3)
    third = F32(1.0) / F32(3.0)
    assert lower.tolist() == [0, 0, 0, 0, 0, 1, 1] and upper.tolist() == [0, 0, 1, 1, 1, 1, 1]
    assert blended.tolist() == [False, False, True, True, True, False, False]
    assert t.dtype == F32 and t[2] == 0 and t[3] == third and t[4] == F32(2.0) * third and not t[[0, 1, 5, 6]].any()
    # the blend of two constant corner frames 10 and 40 along that axis: 10, 10, 10, 20, 30, 40, 40 up to the rounding of 1/3
    corners = np.empty((1, 1, 2, 1, 1, 1, 7), F32)
    corners[0, 0, 0], corners[0, 0, 1] = 10.0, 40.0
    out = ref.blend(corners, (2, 0, 0), (3, 1, 1))[0, 0, 0]
    print(f"  {out.tolist()}")
    assert out[[0, 1, 2]].tolist() == [10.0] * 3 and out[[5, 6]].tolist() == [40.0] * 2
    assert out[3] == ref.fmaf(third, F32(30), F32(10)) and out[4] == ref.fmaf(F32(2) * third, F32(30), F32(10))
    assert abs(float(out[3]) - 20.0) <= 2e-6 and abs(float(out[4]) - 30.0) <= 4e-6
    # one node: no axis is read, nothing is blended; a node beyond the frame: the voxels in front of it still blend toward it
    assert not ref.segments(5, 1, 99, 0)[3].any()
    lower, upper, t, blended = ref.segments(4, 2, 0, 8)
    assert blended.all() and upper.tolist() == [1] * 4 and t.tolist() == [0.0, 0.125, 0.25, 0.375]
    # NaN and infinity pass through a lerp by plain IEEE
    corners[0, 0, 0, 0, 0, 0, 3], corners[0, 0, 1, 0, 0, 0, 4] = np.nan, np.inf
    out = ref.blend(corners, (2, 0, 0), (3, 1, 1))[0, 0, 0]
    assert np.isnan(out[3]) and np.isposinf(out[4]) and out[2] == 10.0
    # the float64 form agrees with the float32 one within its own bound, and a lattice of one node is the plain mix
    rng = np.random.default_rng(4200)
    frames = [(rng.standard_normal((3, 2, 7)) + 1j * rng.standard_normal((3, 2, 7))).astype(np.complex64) for _ in range(3)]
    W = (rng.standard_normal((2, 1, 2, 2, 3)) + 1j * rng.standard_normal((2, 1, 2, 2, 3))).astype(np.complex64)
    out, bound = ref.mix_field(frames, W, (2, 0, 0), (3, 1, 2))
    corners = np.array([[[ensemble_ref.mix(frames, W[jz, 0, jx])[0].astype(np.complex64) for jx in range(2)]] for jz in range(2)])
    exact = ref.blend(corners, (2, 0, 0), (3, 1, 2))
    assert exact.shape == out.shape == (2, 3, 2, 7)
    assert (np.maximum(np.abs(exact.real - out.real), np.abs(exact.imag - out.imag)) <= bound).all()
    plain, plain_bound = ensemble_ref.mix(frames, W[0, 0, 0])
    one, one_bound = ref.mix_field(frames, W[:1, :, :1], (9, 9, 9), (0, 0, 0))
    assert np.array_equal(one, plain) and np.allclose(one_bound, plain_bound * (2 * 3 + 11) / (2 * 3 + 2))


def test_the_two_clutter_ensemble_separates_the_block_wise_filter_from_the_global_one():
    """a condition on the inputs of tests/test_gpu_block_filter.py's loop: on the reference alone, the two-node block-wise rank-1 filter
    leaves less than 1e-3 of the clutter energy the global rank-1 filter leaves"""
    frames, parts = ref.two_clutter_ensemble()
    K = frames.shape[0]
    points = (frames.shape[3], frames.shape[2], frames.shape[1])
    nodes, first, step, half = ref.two_clutter_lattice(points)
    boxes = ref.lattice_boxes(points, nodes, first, step, half)
    assert boxes == [((15, 0, 0), (1, 1, 48)), ((16, 0, 0), (1, 1, 48))]
    G, voxels, _, _ = ensemble_ref.gram(list(frames))
    W_global, values = ensemble_ref.projector(G, 1)
    global_out, _ = ensemble_ref.mix(list(frames), W_global)
    W = np.empty((1, 1, 2, K, K), np.complex128)
    for n, (Gb, Vb, _, _) in enumerate(ref.gram_boxes(list(frames), boxes)):
        assert Vb == 48
        W[0, 0, n], _ = ensemble_ref.projector(Gb, 1)
    block_out, _ = ref.mix_field(list(frames), W.astype(np.complex64), first, step)
    before = ref.clutter_left(frames, parts)
    left_global, left_block = ref.clutter_left(global_out, parts), ref.clutter_left(block_out, parts)
    signal = float((np.abs(parts["signal"]) ** 2).sum())
    kept = float((np.abs(np.tensordot(parts["s"].conj(), block_out, axes=(0, 0))) ** 2).sum())
    print(f"  clutter energy {before:.4e}; left by the global rank-1 filter {left_global:.4e}, by the two-node block-wise one {left_block:.4e} "
          f"(ratio {left_block / left_global:.3e}); signal {signal:.4e}, kept by the block-wise filter {kept:.4e}")
    assert left_global > 0.2 * before                          # one cut cannot take two directions out
    assert left_block < 1e-3 * left_global
    assert 0.9 * signal < kept < 1.1 * signal                  # and the weak signal comes through
