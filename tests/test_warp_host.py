"""The warp on the CPU (beamformer_hip_warp_last_frames): the symbol is declared, exported and bound, its limits and enums agree between
the header and params.py; the kernel DESIGN 3.7g names is in the library, eight instantiations without spills or scratch, inside the
register and LDS budgets stated there; every refusal that needs no device holds, with its error kind, and leaves the outputs alone;
and the numpy reference the device tests judge against (tests/warp_ref.py) gives cases small enough to work out by hand, holds its
float32 restatement inside its own bound, and tells the definition from the five mistakes nearest to it."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from ogl_beamforming_amd import lib
from ogl_beamforming_amd import params as P
from tests import warp_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = P.LibError
NAME = "beamformer_hip_warp_last_frames"
MAX = P.HIP_MAX_ENSEMBLE_FRAMES
LINEAR, CUBIC, ZERO, CLAMP = ref.LINEAR, ref.CUBIC, ref.ZERO, ref.CLAMP


def test_the_symbol_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "ogl_beamformer_hip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", lib.LIBRARY_PATH], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in nm.stdout.splitlines() if " T " in line}
    assert re.search(r"BEAMFORMER_LIB_EXPORT uint32_t " + NAME + r"\(", header)
    assert NAME in exported and NAME in lib.exported_symbols()
    assert len(getattr(lib.library(), NAME).argtypes) == 11
    assert re.search(r"#define BEAMFORMER_HIP_MAX_WARP_NODES\s+(\d+)u", header).group(1) == str(P.HIP_MAX_WARP_NODES) == "4096"
    assert re.search(r"#define BEAMFORMER_HIP_MAX_WARP_ENTRIES\s+(\d+)u", header).group(1) == str(P.HIP_MAX_WARP_ENTRIES) == "32768"
    assert float(re.search(r"#define BEAMFORMER_HIP_MAX_WARP_DISPLACEMENT\s+([0-9.]+)f", header).group(1)) == P.HIP_MAX_WARP_DISPLACEMENT == 65536.0
    assert [(m.name, int(m)) for m in P.HipWarpInterpolation] == [("Linear", 0), ("Cubic", 1)]
    assert [(m.name, int(m)) for m in P.HipWarpEdge] == [("Zero", 0), ("Clamp", 1)]
    assert re.search(r"BeamformerHipWarpInterpolation_Linear = 0,\s*BeamformerHipWarpInterpolation_Cubic  = 1,\s*BeamformerHipWarpInterpolation_Count", header)
    assert re.search(r"BeamformerHipWarpEdge_Zero  = 0,\s*BeamformerHipWarpEdge_Clamp = 1,\s*BeamformerHipWarpEdge_Count", header)
    assert "BeamformerHipDasPath_WarpDirect       = 0x10000" in header and P.HIP_DAS_PATH_WARP_DIRECT == 0x10000
    # the call's table fits the table of a mix: rotations and field against 2 K^2 floats
    assert 2 * MAX + 3 * P.HIP_MAX_WARP_ENTRIES <= 2 * MAX * MAX


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="needs the ROCm LLVM binutils")
def test_the_kernel_design_names_is_in_the_library_within_its_budgets():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "warp_kernel" in design and "eight instantiations" in design
    kernels = [k for k in kernel_resources.kernels_of(lib.LIBRARY_PATH) if "warp_kernel" in k["demangled"]]
    assert len(kernels) == 8, [k["demangled"] for k in kernels]          # complex / real x Linear / Cubic x Zero / Clamp
    sizes = set()
    for k in kernels:
        print(f"  {k['demangled'].split('(')[0]}: {k['vgpr_count']} VGPRs, {k['group_segment_fixed_size']} bytes of LDS")
        assert not k["vgpr_spill_count"] and not k["private_segment_fixed_size"], k["demangled"]
        assert k["vgpr_count"] <= 128, k["demangled"]
        # the stated budget: 4096 voxels and 96 bytes of ends -- at least two blocks (four, in fact) in a CU's 160 KiB
        assert 0 < k["group_segment_fixed_size"] <= 4096 * 8 + 96, k["demangled"]
        sizes.add(k["group_segment_fixed_size"])
    assert sizes == {4096 * 8 + 96, 4096 * 4 + 96}


def floats(values):
    return (C.c_float * len(values))(*values)


def call(L, count, field, nodes, node_first, node_step, rotations, interpolation, edge, first, ms):
    triple = lambda kind, v: None if v is None else (kind * 3)(*v)      # noqa: E731
    return getattr(L, NAME)(count, field, triple(C.c_uint32, nodes), triple(C.c_float, node_first), triple(C.c_float, node_step), rotations,
                            interpolation, edge, 0, None if first is None else C.byref(first), None if ms is None else C.byref(ms))


def test_every_refusal_that_needs_no_device():
    L = lib.library()
    L.beamformer_hip_shutdown()                       # (no device in use from here on: none of the calls below starts one)
    first, ms = C.c_uint32(77), C.c_float(-1.0)
    good = floats([0.5] * (3 * 2 * 8))
    nan, inf = float("nan"), float("inf")

    def refused(kind, count=2, field=good, nodes=(2, 2, 2), node_first=(0, 0, 0), node_step=(1, 1, 1), rotations=None, interpolation=0, edge=0):
        assert not call(L, count, field, nodes, node_first, node_step, rotations, interpolation, edge, first, ms)
        assert lib.last_error()[0] == kind
        assert first.value == 77 and ms.value == -1.0

    # (the count, the outputs and the good call without a device: tests/test_frame_ops_contract_host.py)
    refused(E.BufferOverflow, count=0, field=None, nodes=None)           # BufferOverflow on count is decided before the field is looked at
    for at in range(3):
        refused(E.BufferOverflow, nodes=[0 if a == at else 2 for a in range(3)])
    big = floats([0.0] * (3 * 4097))
    refused(E.BufferOverflow, count=1, field=big, nodes=(4097, 1, 1))
    refused(E.BufferOverflow, count=1, field=big, nodes=(64, 64, 2))
    refused(E.BufferOverflow, count=1, field=big, nodes=(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF))
    refused(E.BufferOverflow, count=9, field=big, nodes=(16, 16, 16))   # 9 x 4096 entries
    refused(E.BufferOverflow, count=MAX, field=big, nodes=(129, 1, 1))  # 256 x 129 entries
    refused(E.InvalidAccess, field=None)
    refused(E.InvalidAccess, nodes=None)
    refused(E.InvalidAccess, node_first=None)
    refused(E.InvalidAccess, node_step=None)
    for bad in (nan, inf, -inf, 65537.0, -65536.5):
        for at in (0, 1, 3 * 2 * 8 - 1):
            refused(E.InvalidAccess, field=floats([bad if n == at else 0.5 for n in range(3 * 2 * 8)]))
        refused(E.InvalidAccess, count=1, field=floats([0.0, bad, 0.0]), nodes=(1, 1, 1))
    for bad in (nan, inf, -inf):
        refused(E.InvalidAccess, node_first=(0, bad, 0))
        refused(E.InvalidAccess, rotations=floats([1.0, 0.0, bad, 0.0]))
        refused(E.InvalidAccess, rotations=floats([1.0, 0.0, 0.0, bad]))
    for bad in (nan, inf, 0.0, -1.0):
        refused(E.InvalidAccess, node_step=(1, 1, bad))
    refused(E.InvalidAccess, interpolation=2)
    refused(E.InvalidAccess, edge=2)
    refused(E.InvalidAccess, interpolation=0xFFFFFFFF)
    # every argument good, the limits themselves among them: no device yet, so there is no frame
    refused(E.InvalidAccess, interpolation=1, edge=1, rotations=floats([0.0, 1.0, 1.0, 0.0]))
    refused(E.InvalidAccess, field=floats([65536.0, -65536.0, 0.0] * 16))                        # the limit itself is legal
    refused(E.InvalidAccess, count=1, field=floats([1.0, 2.0, 3.0]), nodes=(1, 1, 1), node_step=(0, nan, -1))   # with one node the step is not read
    refused(E.InvalidAccess, count=8, field=big, nodes=(16, 16, 16))    # 8 x 4096 entries: the limit itself
    with pytest.raises(lib.BeamformerError):
        lib.warp_last_frames(1, np.zeros((2, 1, 2, 3)), nodes=(2, 1, 2), interpolation=P.HipWarpInterpolation.Cubic, edge=P.HipWarpEdge.Clamp, rotations=[1j])
    with pytest.raises(ValueError):
        lib.warp_last_frames(2, np.zeros((2, 3)), nodes=(2, 1, 1))
    with pytest.raises(ValueError):
        lib.warp_last_frames(2, np.zeros((2, 3)), rotations=[1.0])


# ---- the reference by hand ----

def test_the_reference_by_hand():
    f = np.array([[[1.0, 2.0, 4.0, 8.0]]], np.float32)                  # 4 x 1 x 1 (x, y, z)
    # the sign: output at v is the source at v + d -- d = +1 brings the right-hand neighbour; y and z components change nothing here
    for interpolation in (LINEAR, CUBIC):
        out, bound = ref.warp(f, [1.0, 7.0, -3.0], interpolation=interpolation)
        assert out.dtype == np.float64 and np.array_equal(out[0, 0], [2, 4, 8, 0]) and (bound >= 0).all()
        assert np.array_equal(ref.warp(f, [-2.0, 0, 0], interpolation=interpolation)[0][0, 0], [0, 0, 1, 2])
        assert np.array_equal(ref.warp(f, [1.0, 0, 0], interpolation=interpolation, edge=CLAMP)[0][0, 0], [2, 4, 8, 8])
        assert np.array_equal(ref.warp(f, [-2.0, 0, 0], interpolation=interpolation, edge=CLAMP)[0][0, 0], [1, 1, 1, 2])
        assert np.array_equal(ref.warp_float32(f, [1.0, 0, 0], interpolation=interpolation)[0, 0], [2, 4, 8, 0])
    # half a voxel, linear: the mean of two neighbours; the last voxel's right-hand tap is outside
    assert np.array_equal(ref.warp(f, [0.5, 0, 0])[0][0, 0], [1.5, 3, 6, 4])
    assert np.array_equal(ref.warp(f, [0.5, 0, 0], edge=CLAMP)[0][0, 0], [1.5, 3, 6, 8])
    assert np.array_equal(ref.warp(f, [-0.5, 0, 0])[0][0, 0], [0.5, 1.5, 3, 6])
    assert np.array_equal(ref.warp(f, [-0.5, 0, 0], edge=CLAMP)[0][0, 0], [1, 1.5, 3, 6])
    # Catmull-Rom at t = 0.5: weights -1/16, 9/16, 9/16, -1/16, in both restatements
    assert np.array_equal(ref.weights_of(np.float64(0.5), CUBIC, np.float64), [-0.0625, 0.5625, 0.5625, -0.0625])
    assert np.array_equal(ref.weights_of(np.float32(0.5), CUBIC, np.float32), np.array([-0.0625, 0.5625, 0.5625, -0.0625], np.float32))
    for t in (0.0, 0.125, 0.75, 1.0):
        assert abs(sum(ref.weights_of(np.float64(t), CUBIC, np.float64)) - 1.0) < 1e-15
    out = ref.warp(f, [0.5, 0, 0], interpolation=CUBIC)[0][0, 0]
    assert np.array_equal(out, [(9 * 1 + 9 * 2 - 4) / 16, (-1 + 9 * 2 + 9 * 4 - 8) / 16, (-2 + 9 * 4 + 9 * 8) / 16, (-4 + 9 * 8) / 16])
    out = ref.warp(f, [0.5, 0, 0], interpolation=CUBIC, edge=CLAMP)[0][0, 0]
    assert np.array_equal(out, [(-1 + 9 * 1 + 9 * 2 - 4) / 16, (-1 + 9 * 2 + 9 * 4 - 8) / 16, (-2 + 9 * 4 + 9 * 8 - 8) / 16, (-4 + 9 * 8 + 9 * 8 - 8) / 16])
    # a two-node field: d = 0 at x = 1, d = 1 at x = 3, constant outside the lattice: d = (0, 0, 0.5, 1)
    field = np.array([[0, 0, 0], [1, 0, 0]], np.float32)
    out, _ = ref.warp(f, field, nodes=(2, 1, 1), node_first=(1, 0, 0), node_step=(2, 1, 1))
    assert np.array_equal(out[0, 0], [1, 2, 6, 0])
    assert np.array_equal(ref.warp_float32(f, field, nodes=(2, 1, 1), node_first=(1, 0, 0), node_step=(2, 1, 1))[0, 0], [1, 2, 6, 0])
    # 2 x 2 x 1: a shift along y, then along both axes by half a voxel: the mean of four
    g = np.array([[[1.0, 2.0], [3.0, 5.0]]], np.float32)
    assert np.array_equal(ref.warp(g, [0, 1.0, 9.0])[0][0], [[3, 5], [0, 0]])
    assert np.array_equal(ref.warp(g, [0.5, 0.5, 0])[0][0], [[2.75, 1.75], [2, 1.25]])
    assert np.array_equal(ref.warp(g, [0.5, 0.5, 0], edge=CLAMP)[0][0], [[2.75, 3.5], [4, 5]])
    # NaN under the support poisons, a zero weight's tap included (d = 0: taps v and v + 1, the second of weight 0); parts apart
    c = np.array([[[1 + 1j, np.nan + 2j, 3 + 3j, 4 + 4j]]], np.complex64)
    out, _ = ref.warp(c, [0.0, 0, 0])
    assert np.array_equal(np.isnan(out.real[0, 0]), [True, True, False, False]) and not np.isnan(out.imag).any()
    assert np.array_equal(out.imag[0, 0], [1, 2, 3, 4])
    # a rotation by i: (x, y) -> (-y, x); real frames take the real part
    out, bound = ref.warp(c[:, :, 2:], [0.0, 0, 0], rotation=1j)
    assert np.array_equal(out[0, 0], [-3 + 3j, -4 + 4j]) and (bound.real >= 0).all() and (bound.imag >= 0).all()
    assert np.array_equal(ref.warp_float32(c[:, :, 2:], [0.0, 0, 0], rotation=1j)[0, 0], [-3 + 3j, -4 + 4j])
    assert np.array_equal(ref.warp(f, [0.0, 0, 0], rotation=-2.0)[0][0, 0], [-2, -4, -8, -16])
    # an integer shift is exact: the bound of an exact case is rounding-sized
    out, bound = ref.warp(f, [1.0, 0, 0])
    assert bound.max() < 64 * ref.U * 8


def test_the_path_rule_by_hand():
    """tests/warp_ref.py restates which path a tile takes: the tile of a grid, and the voxels of a tile's source box"""
    assert [ref.tile_of(e) for e in ((512, 1, 1024), (256, 256, 256), (33, 1, 7), (9, 5, 6), (1, 1, 1), (2, 1, 1000), (1, 300, 1))] == \
        [(16, 1, 16), (8, 8, 4), (32, 1, 8), (8, 8, 4), (1, 1, 1), (2, 1, 128), (1, 256, 1)]
    # a line of 40 voxels, one tile: a shift of 2.5 reads 2 .. 41, cut to 2 .. 39; the cubic's taps 1 .. 42, cut to 1 .. 39
    assert ref.tile_boxes((1, 1, 40), [2.5, 0, 0]).tolist() == [[[38]]]
    assert ref.tile_boxes((1, 1, 40), [2.5, 0, 0], interpolation=CUBIC).tolist() == [[[39]]]
    assert ref.tile_boxes((1, 1, 40), [-100.0, 0, 0]).tolist() == [[[1]]]                 # every tap at the clamped edge
    # 20 x 1 x 20 under tiles of 16 x 16: four tiles, the ragged ones smaller; a field from -8 at x = 0 to +8 at x = 16 widens the first
    assert ref.tile_boxes((20, 1, 20), [0.0, 0, 0]).tolist() == [[[17 * 17, 4 * 17]], [[17 * 4, 4 * 4]]]
    boxes = ref.tile_boxes((20, 1, 20), np.array([[-8.0, 0, 0], [8.0, 0, 0]], np.float32), nodes=(2, 1, 1), node_first=(0, 0, 0), node_step=(16, 1, 1))
    # x of the first tile: taps from 0 - 8, cut to 0, to 15 + 7.5 + 1, cut to 19; the ragged tile reads 16 + 8 .. 19 + 8 + 1: all at the edge, x = 19
    assert boxes.tolist() == [[[20 * 17, 1 * 17]], [[20 * 4, 1 * 4]]]
    assert ref.BOX_VOXELS == 4096


# ---- the reference on the device tests' kinds of input ----

def inputs():
    """(label, frame, keywords of ref.warp): frames of the device tests' shapes (z, y, x) and fields of their kinds"""
    rng = np.random.default_rng(9500)

    def frame(shape, cplx=True):
        f = rng.standard_normal(shape) + 0.5
        if cplx:
            f = f + 1j * (rng.standard_normal(shape) - 0.5)
        return f.astype(np.complex64 if cplx else np.float32)

    for interpolation in (LINEAR, CUBIC):
        for edge in (ZERO, CLAMP):
            k = dict(interpolation=interpolation, edge=edge)
            yield "plane rigid", frame((7, 1, 33)), dict(k, field=[2.375, 0.5, -1.625])
            yield "volume lattice", frame((6, 5, 9)), dict(k, field=rng.uniform(-2, 2, (2, 2, 2, 3)), nodes=(2, 2, 2), node_first=(2, 1, 1.5), node_step=(4, 2, 2.5))
            yield "real lattice", frame((7, 1, 33), cplx=False), dict(k, field=rng.uniform(-2, 2, (2, 1, 2, 3)), nodes=(2, 1, 2), node_first=(5, 0, 1), node_step=(20, 1, 4), rotation=-1.5)
            yield "square wild", frame((64, 1, 64)), dict(k, field=rng.uniform(-40, 40, (3, 1, 3, 3)), nodes=(3, 1, 3), node_first=(0, 0, 0), node_step=(31.5, 1, 31.5), rotation=0.6 - 0.8j)


def test_a_float32_restatement_stays_inside_the_bound():
    for label, frame, k in inputs():
        values, bound = ref.warp(frame, **k)
        got = ref.warp_float32(frame, **k)
        worst, inside = ref.share_of_bound(got, values, bound)
        finite = np.isfinite(values.real) & np.isfinite(values.imag)
        print(f"  {label}, interpolation {k['interpolation']}, edge {k['edge']}: float32 numpy at {worst:.3f} of the bound at the worst")
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


def test_the_bound_tells_the_definition_from_five_mistakes():
    for label, frame, k in inputs():
        values, bound = ref.warp(frame, **k)
        mistakes = {"the opposite sign": ref.warp(frame, sign=-1, **k)[0]}
        if k["interpolation"] == CUBIC:
            mistakes["cubic B-spline weights"] = ref.warp(frame, bspline=True, **k)[0]
            mistakes["linear for cubic"] = ref.warp(frame, **dict(k, interpolation=LINEAR))[0]
        if "nodes" in k:
            mistakes["nodes off by half a step"] = ref.warp(frame, node_shift=0.5, **k)[0]
        for name, wrong in mistakes.items():
            share = moved_share(wrong, values, bound)
            print(f"  {label}, interpolation {k['interpolation']}, edge {k['edge']}, {name}: {share:.3f} of the floats leave the bound")
            assert share > 0.5, (label, name)
    # Clamp for Zero, on inputs whose displaced reads leave the frame for most voxels
    rng = np.random.default_rng(9501)
    frame = (rng.standard_normal((7, 1, 33)) + 1j * rng.standard_normal((7, 1, 33)) + 1).astype(np.complex64)
    for interpolation in (LINEAR, CUBIC):
        k = dict(field=[20.5, 0, -4.25], interpolation=interpolation)
        values, bound = ref.warp(frame, edge=ZERO, **k)
        share = moved_share(ref.warp(frame, edge=CLAMP, **k)[0], values, bound)
        print(f"  Clamp for Zero, interpolation {interpolation}: {share:.3f} of the floats leave the bound")
        assert share > 0.5
