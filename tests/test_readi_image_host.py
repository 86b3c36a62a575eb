"""READI image pushes (beamformer_hip_push_data_readi_image_with_compute), everything that needs no device: what
beamformer_hip_describe_readi_image reports against beamformer_hip_describe_das of the derived FORCES block, the refusals -- which
the push makes before it touches a device and before it takes an id, so they are asked of the push itself as well -- and the
identity the push rests on, checked on the CPU oracle alone: the sum of the oracle's READI frames is the oracle's FORCES frame of the
host-decoded RF (tests/readi_image_cases.py)."""
import ctypes as C

import numpy as np
import pytest

from ogl_beamforming_amd import params as P
from tests import cases
from tests import readi_image_cases as R
from tests.das_push import noise_frames

E = P.LibError
I = P.InterpolationMode

# (geometry, interpolation, kind, acquisition kind, sparse elements, group list -- None: a permutation of 0 .. G - 1)
DESCRIBED = [("g4a4", I.Linear, "real", R.K.FORCES, None, None), ("g2a8", I.Cubic, "iq", R.K.FORCES, None, None),
             ("g8a2", I.Linear, "iq", R.K.FORCES, None, None), ("g12a1", I.Cubic, "real", R.K.FORCES, None, R.PARTIAL12),
             ("g4a4", I.Nearest, "real", R.K.FORCES, None, None),
             ("g4a4", I.Linear, "i16", R.K.FORCES, None, None), ("g8a2", I.Cubic, "i16", R.K.UFORCES, [5], None),
             ("g12a1", I.Linear, "i16", R.K.FORCES, None, None)]
DESCRIBED_IDS = [f"{g}-{i.name.lower()}-{k}{'-uforces' if a == R.K.UFORCES else ''}{'-partial' if l else ''}" for g, i, k, a, s, l in DESCRIBED]
# the f32 cases of the identity: every geometry, both kinds, linear and cubic
IDENTITY = [(g, interp, kind) for n, g in enumerate(R.GEOMETRIES) for m, interp in enumerate((I.Linear, I.Cubic)) for kind in (("real", "iq")[(n + m) % 2],)]
IDENTITY += [("g12a1", I.Linear, "real-partial"), ("g4a4", I.Nearest, "iq")]


@pytest.fixture()
def L(bflib):
    lib = bflib.library()
    lib.beamformer_reserve_parameter_blocks(2)
    lib.beamformer_hip_set_das_path(0)
    yield lib
    lib.beamformer_hip_set_das_path(0)
    lib.beamformer_reserve_parameter_blocks(1)


def refused(bflib, kind, call):
    with pytest.raises(bflib.BeamformerError) as e:
        call()
    assert e.value.kind == kind, e.value
    return e.value


def push(bflib, acq, n, groups=None):
    """the host push of n copies of the case's RF: reaches the device only when nothing refuses it first"""
    lib = bflib.library()
    for slot, fp in enumerate(acq.filters):
        assert lib.beamformer_create_filter(C.byref(fp), slot, 0), bflib.last_error()
    assert lib.beamformer_push_simple_parameters(C.byref(acq.bp)), bflib.last_error()
    rf = np.ascontiguousarray(np.broadcast_to(acq.rf, (max(n, 1),) + acq.rf.shape))
    array = None if groups is None else (C.c_uint32 * len(groups))(*groups)
    bflib._check(lib.beamformer_hip_push_data_readi_image_with_compute(rf.ctypes.data_as(C.c_void_p), acq.rf.nbytes, n, array, 0, 0))


@pytest.mark.parametrize("geometry,interp,kind,acquisition_kind,sparse,groups", DESCRIBED, ids=DESCRIBED_IDS)
def test_the_description_is_the_derived_blocks_own_decision(geometry, interp, kind, acquisition_kind, sparse, groups, L, bflib):
    acq = R.image_case(geometry, interp, kind, acquisition_kind=acquisition_kind, sparse=sparse)
    G, A, _ = R.GEOMETRIES[geometry]
    groups = R.PERMUTATIONS[geometry] if groups is None else groups
    for mode in (1, 0):
        L.beamformer_hip_set_das_path(mode)
        d = bflib.describe_readi_image(acq.bp, len(groups), groups, acq.filters)
        derived = bflib.describe_das(R.derived_case(acq).bp, acq.filters, slot=1)[4]
        assert d.transmit_count == G * A and d.decode_launches == 1 and d.stage_launches == 1
        assert d.das_path == derived.path and d.das_launches == 1, (mode, d.reason, derived.name)
        assert b"READI image" in d.reason and derived.name in d.reason, d.reason
    # the route does not depend on the list or on the count: one frame, three frames and no list
    a, b = bflib.describe_readi_image(acq.bp, 1, [0], acq.filters), bflib.describe_readi_image(acq.bp, 3, None, acq.filters)
    assert a.das_path == b.das_path == d.das_path


def test_the_automatic_path_of_the_derived_block_is_not_the_general_kernel(L, bflib):
    """what the image is for: G x A >= 3 FORCES transmits run the factored kernel, not the general one a READI frame needs"""
    for geometry in R.GEOMETRIES:
        acq = R.image_case(geometry, I.Linear, "real")
        assert bflib.describe_das(acq.bp, acq.filters)[4].path == 0
        assert bflib.describe_readi_image(acq.bp, 2, [0, 1], acq.filters).das_path == 3, geometry


def frames_taken(bflib):
    """the id the next push would take, as far as the host knows it: a refused push must leave it where it was.  Without a device
    there is no frame to ask for: the frame info call fails both before and after."""
    info = P.HipFrameInfo()
    ok = bflib.library().beamformer_hip_get_last_frame_info(C.byref(info))
    return (ok, int(info.frame_id) if ok else None)


@pytest.mark.parametrize("name", ["config1_small", "forces", "readi_one_group"])
def test_blocks_that_are_not_readi_are_refused(name, L, bflib, capfd):
    if name == "readi_one_group":
        acq = cases.make("readi")
        acq.bp.readi_group_count, acq.bp.readi_group = 1, 0
    else:
        acq = cases.make(name)                    # a Flash block; a FORCES block with readi_group_count 0
    before = frames_taken(bflib)
    capfd.readouterr()
    refused(bflib, E.InvalidAccess, lambda: bflib.describe_readi_image(acq.bp, 4, None, acq.filters))
    assert "FORCES / UFORCES block with readi_group_count > 1" in capfd.readouterr().err
    refused(bflib, E.InvalidAccess, lambda: push(bflib, acq, 4))
    assert "FORCES / UFORCES block with readi_group_count > 1" in capfd.readouterr().err
    assert frames_taken(bflib) == before


def test_a_group_out_of_range(L, bflib):
    acq = cases.make("readi")                     # G = 4
    before = frames_taken(bflib)
    for groups in ([0, 1, 2, 3, 4], [4], [0, 0, 0xFFFFFFFF]):
        refused(bflib, E.InvalidComputeStage, lambda: bflib.describe_readi_image(acq.bp, len(groups), groups))
        refused(bflib, E.InvalidComputeStage, lambda: push(bflib, acq, len(groups), groups))
    assert frames_taken(bflib) == before


@pytest.mark.parametrize("n", [0, 1025])
def test_frame_counts_out_of_range(n, L, bflib):
    acq = cases.make("readi")
    before = frames_taken(bflib)
    refused(bflib, E.BufferOverflow, lambda: bflib.describe_readi_image(acq.bp, n))
    refused(bflib, E.BufferOverflow, lambda: push(bflib, acq, n))
    assert frames_taken(bflib) == before


def test_more_transmits_than_the_emission_limit(L, bflib, capfd):
    """G = 32, A = 16: 512 transmit elements, twice BeamformerMaxEmissionsCount"""
    acq = R._forces("readi_image_g32a16", 32, 16, (16, 1, 16), "real", I.Linear, False, 3999)
    before = frames_taken(bflib)
    assert bflib.describe_readi_sweep(acq.bp, 4).single_path == 0        # a valid READI block: the sweep takes it
    capfd.readouterr()
    refused(bflib, E.InvalidAccess, lambda: bflib.describe_readi_image(acq.bp, 4))
    assert "32 x 16" in capfd.readouterr().err
    refused(bflib, E.InvalidAccess, lambda: push(bflib, acq, 4))
    assert "32 x 16" in capfd.readouterr().err
    assert frames_taken(bflib) == before
    # at the limit it is taken: G = 16, A = 16
    ok = R._forces("readi_image_g16a16", 16, 16, (16, 1, 16), "real", I.Linear, False, 3998)
    assert bflib.describe_readi_image(ok.bp, 4).transmit_count == 256


# ---- the identity, on the oracle alone

def test_the_order_12_matrix_is_not_symmetric(bflib):
    H = R.hadamard(bflib, 12)
    assert not np.array_equal(H, H.T)
    for G in (2, 4, 8):
        assert np.array_equal(R.hadamard(bflib, G) @ R.hadamard(bflib, G).T, G * np.eye(G))


@pytest.mark.parametrize("geometry,interp,kind", IDENTITY, ids=[f"{g}-{i.name.lower()}-{k}" for g, i, k in IDENTITY])
def test_the_sum_of_the_oracles_readi_frames_is_its_forces_frame_of_the_decoded_rf(geometry, interp, kind, bflib, oracle):
    """float64 sum of the oracle's READI frames against the oracle's FORCES frame of the host-decoded RF: within 1e-5 of the frame maximum
    (measured 4.5e-7 .. 8.0e-7: both sides are float32 sums of the same C x G x A terms a voxel in different orders).  With the matrix
    indexed transposed the order-12 case is off by more than the maximum itself: that is asserted too."""
    partial = kind.endswith("-partial")
    acq = R.image_case(geometry, interp, kind.split("-")[0])
    groups = R.PARTIAL12 if partial else R.PERMUTATIONS[geometry]
    rf = noise_frames(acq, len(groups), 6100 + len(groups))
    total = None
    for k, g in enumerate(groups):
        frame, _ = oracle.beamform(R.with_group(acq, g).bp, rf[k], acq.filters)
        total = frame.astype(np.complex128 if np.iscomplexobj(frame) else np.float64) + (0 if total is None else total)
    derived = R.derived_case(acq, R.decoded_rf(bflib, acq, rf, groups))
    image, _ = oracle.beamform(derived.bp, derived.rf, acq.filters)
    scale = np.abs(total).max()
    assert scale > 0
    worst = np.abs(image - total).max() / scale
    print(f"{acq.name}: sum of {len(groups)} oracle READI frames against the oracle FORCES frame of the decoded RF: {worst:.2e} of the maximum")
    assert worst <= 1e-5, worst
    if geometry == "g12a1":
        G, A, Sn = 12, 1, 512
        frames = (rf.view(np.complex64) if kind.startswith("iq") else rf).reshape(len(groups), 16, A, Sn)
        wrong = R.decode(R.hadamard(bflib, G).T.copy(), groups, frames)
        wrong = np.ascontiguousarray(wrong)
        transposed, _ = oracle.beamform(derived.bp, (wrong.view(np.float32) if kind.startswith("iq") else wrong).reshape(16, -1), acq.filters)
        assert np.abs(transposed - total).max() / scale > 0.5
