"""READI image pushes through the C ABI (beamformer_hip_push_data_readi_image_with_compute) on the device: N group acquisitions
compounded into ONE frame -- the derived FORCES block's single push of the DAS input decoded across the acquisitions
(tests/readi_image_cases.py states the identity; tests/test_readi_image_host.py checks it on the CPU oracle alone).

The frame is judged exactly as a single frame is: tests/parity.py compare() against the CPU oracle's frame of the derived FORCES
acquisition on host-decoded RF, with cases.tolerance -- nothing is loosened.  The decoded buffer is checked bit for bit against the
sequential float32 sum, and the image against the single push of that buffer, bit for bit as well.  All cases are the `readi`
case's size class (16 channels, 512 samples, 16 x 1 x 16 to 32 x 1 x 32 voxels)."""
import ctypes as C

import numpy as np
import pytest

from ogl_beamforming_amd import params as P
from tests import cases
from tests import readi_image_cases as R
from tests.das_push import compare, last_timings, noise_frames, same_bits
from tests.parity import reference
from tests.push_kinds import group_list, image, last_frame_id
from tests.scaffold import automatic_path  # noqa: F401

pytestmark = pytest.mark.gpu
I = P.InterpolationMode
S = P.ShaderKind

# every interpolation x kind x coherency weighting once, the geometries dealt round; then the group lists that are no permutation
VARIANTS = [(list(R.GEOMETRIES)[i % 4], interp, kind, cw, "permutation")
            for i, (interp, kind, cw) in enumerate((interp, kind, cw) for interp in (I.Linear, I.Cubic, I.Nearest) for kind in ("real", "iq") for cw in (False, True))]
VARIANTS += [("g12a1", I.Linear, "real", False, "partial"), ("g12a1", I.Cubic, "iq", True, "partial"),
             ("g4a4", I.Cubic, "real", False, "no-list"), ("g8a2", I.Linear, "iq", True, "no-list"),
             ("g4a4", I.Linear, "iq", False, "one"), ("g2a8", I.Cubic, "real", True, "one")]
VARIANT_IDS = [f"{g}-{interp.name.lower()}-{kind}{'-cw' if cw else ''}-{listed}" for g, interp, kind, cw, listed in VARIANTS]


@pytest.fixture(autouse=True)
def two_parameter_blocks(automatic_path, bflib):
    L = bflib.library()
    L.beamformer_reserve_parameter_blocks(2)
    yield
    L.beamformer_reserve_parameter_blocks(1)


@pytest.mark.parametrize("geometry,interp,kind,cw,listed", VARIANTS, ids=VARIANT_IDS)
def test_image_parity(geometry, interp, kind, cw, listed, bflib, oracle):
    acq = R.image_case(geometry, interp, kind, cw)
    groups, n = group_list(geometry, listed)
    rf = noise_frames(acq, n, 6200 + n)
    frame, info = image(bflib, acq, rf, groups)
    derived = R.derived_case(acq, R.decoded_rf(bflib, acq, rf, groups))
    ref, _, flags = reference(oracle, derived)
    v = compare(frame, ref, derived, flags, label=f"{acq.name}/{listed}")
    print(f"{acq.name}/{listed}: image of {n} acquisitions on das path {info.route.das_path}: max_rel_err {v.max_rel_err:.3e} (tolerance {cases.tolerance(derived):.0e})")


@pytest.mark.parametrize("geometry,kind,listed", [("g12a1", "real", "partial"), ("g8a2", "iq", "permutation")], ids=["g12a1-real-partial", "g8a2-iq"])
def test_the_decoded_input_bit_for_bit_then_the_image_is_the_derived_single_push(geometry, kind, listed, bflib, hooks):
    """first: beamformer_hip_copy_das_input is the sequential float32 sum, in k order, of +- the per-frame DAS inputs, signs from
    beamformer_hip_host_hadamard -- as words; then: that buffer pushed as the RF of the derived FORCES block, a single push in
    another slot, gives the image's bits, on the same das path.  Under SCRATCH_POISON: an element the decode did not write is a NaN."""
    hooks.set("SCRATCH_POISON")
    L = bflib.library()
    acq = R.image_case(geometry, I.Cubic, kind)
    G, A = int(acq.bp.readi_group_count), int(acq.bp.acquisition_count)
    groups, n = group_list(geometry, listed)
    rf = noise_frames(acq, n, 6300 + n)
    frame, info = image(bflib, acq, rf, groups)
    decoded = bflib.das_input(acq.bp, transmits=G * A).copy()
    inputs = np.stack([bflib.das_input(acq.bp, frame=k) for k in range(n)])
    assert not np.isnan(inputs.view(np.float32)).any()
    expected = R.decode(R.hadamard(bflib, G), groups, inputs)
    assert decoded.shape == expected.shape == (16, G * A, 512) and decoded.dtype == expected.dtype
    assert np.array_equal(decoded.view(np.uint32), expected.view(np.uint32)), "the decoded DAS input is not the sequential float32 sum"
    # (and the per-frame inputs are the RF frames themselves: no stage precedes DAS)
    assert np.array_equal(inputs.view(np.uint32).reshape(n, -1), rf.view(np.uint32).reshape(n, -1))
    with pytest.raises(bflib.BeamformerError):
        bflib.das_input(acq.bp, frame=n)
    # ---- the image IS the derived single push
    derived = R.derived_case(acq, np.ascontiguousarray(decoded).view(np.float32).reshape(16, -1))
    assert L.beamformer_push_simple_parameters_at(C.byref(derived.bp), 1), bflib.last_error()
    data = np.ascontiguousarray(derived.rf)
    assert L.beamformer_push_data_with_compute(data.ctypes.data_as(C.c_void_p), data.nbytes, 0, 1), bflib.last_error()
    single = bflib.get_last_frame(derived.bp).copy()
    assert int(last_timings(bflib).das_path) == info.route.das_path
    assert not np.isnan(single.view(np.float32)).any()
    assert same_bits(single, frame), "the image is not the single push of its decoded input under the derived block"


INT16_CASES = [("g4a4", R.K.FORCES, None), ("g8a2", R.K.UFORCES, [5]), ("g12a1", R.K.FORCES, None)]


@pytest.mark.parametrize("interp", [I.Linear, I.Cubic], ids=["linear", "cubic"])
@pytest.mark.parametrize("geometry,acquisition_kind,sparse", INT16_CASES, ids=["forces-g4a4", "uforces-g8a2-sparse", "forces-g12a1"])
def test_against_the_sum_of_the_oracles_readi_frames(geometry, acquisition_kind, sparse, interp, bflib, oracle):
    """Int16 through (Demodulate, DAS): max|image - sum over k of the oracle's READI frame k| <= cases.tolerance x max|sum| -- the
    pipeline's 2e-3 (the decode before and after the binary16-staged stage: the two CPU references differ by at most 4.7e-4)."""
    acq = R.image_case(geometry, interp, "i16", acquisition_kind=acquisition_kind, sparse=sparse)
    assert cases.tolerance(acq) == 2e-3
    groups = R.PERMUTATIONS[geometry]
    rf = noise_frames(acq, len(groups), 6400 + len(groups))
    frame, info = image(bflib, acq, rf, groups)
    total = np.zeros(frame.shape, np.complex128)
    for k, g in enumerate(groups):
        total += oracle.beamform(R.with_group(acq, g).bp, rf[k], acq.filters)[0]
    scale = np.abs(total).max()
    worst = np.abs(frame - total).max() / scale
    print(f"{acq.name}: image against the sum of {len(groups)} oracle READI frames: {worst:.3e} of the maximum (das path {info.route.das_path})")
    assert scale > 0 and worst <= cases.tolerance(acq), worst
    stages = [int(info.stage_kind[i]) for i in range(info.stage_count)]
    assert stages[:2] == [0xFFFF, int(S.Demodulate)] and stages.count(int(S.Decode)) == 1 and stages[-2:] == [int(S.Decode), int(S.DAS)], stages


def test_against_the_librarys_own_sweep(bflib):
    """a consistency check, not the parity bar: the sweep's frames of the same RF summed in float64, at 1e-4 of the maximum"""
    acq = R.image_case("g8a2", I.Linear, "real")
    groups = R.PERMUTATIONS["g8a2"]
    rf = noise_frames(acq, len(groups), 6500)
    swept = bflib.beamform_readi_sweep(acq.bp, rf, groups, acq.filters).astype(np.float64).sum(axis=0)
    frame, _ = image(bflib, acq, rf, groups)
    worst = np.abs(frame - swept).max() / np.abs(swept).max()
    print(f"{acq.name}: image against the summed sweep: {worst:.3e} of the maximum")
    assert worst <= 1e-4, worst


def test_one_id_one_frame_and_the_stage_list(bflib):
    L = bflib.library()
    acq = R.image_case("g4a4", I.Linear, "real")
    groups = R.PERMUTATIONS["g4a4"]
    rf = noise_frames(acq, 4, 6600)
    first = bflib.beamform(R.with_group(acq, 0).bp, rf[0], acq.filters).copy()
    before = last_frame_id(bflib)
    frame, info = image(bflib, acq, rf, groups)
    assert info.frame_id == before + 1 and last_frame_id(bflib) == before + 1         # ONE id
    frame_info = P.HipFrameInfo()
    assert L.beamformer_hip_get_last_frame_info(C.byref(frame_info))
    assert list(frame_info.points) == [16, 1, 16] and frame_info.data_kind == int(P.DataKind.Float32) and frame_info.parameter_block == 0
    two = bflib.get_last_frames(acq.bp, 2)                                            # the single push before it, then the image
    assert same_bits(two[0], first) and same_bits(two[1], frame)
    stages = [int(info.stage_kind[i]) for i in range(info.stage_count)]
    assert stages == [0xFFFF, int(S.Decode), int(S.DAS)], stages                      # exactly one Decode entry, directly before DAS
    assert all(info.stage_ms[i] > 0 for i in range(info.stage_count)) and info.image_ms > 0
    t = last_timings(bflib)
    assert [int(t.stage_kind[i]) for i in range(t.stage_count)] == stages and t.das_voxels == acq.voxels
    assert abs(t.frame_ms - info.image_ms) <= 1e-5 * info.image_ms                    # one frame: the whole push's time
    # the same RF again: the same bits, the next id
    again, info2 = image(bflib, acq, rf, groups)
    assert same_bits(again, frame) and info2.frame_id == before + 2


def test_pair_counting_counts_on_the_derived_block(bflib):
    L = bflib.library()
    acq = R.image_case("g4a4", I.Linear, "real")
    groups = R.PERMUTATIONS["g4a4"]
    rf = noise_frames(acq, 4, 7000)
    plain, _ = image(bflib, acq, rf, groups)
    derived = R.derived_case(acq, R.decoded_rf(bflib, acq, rf, groups))
    try:
        L.beamformer_hip_enable_pair_counting(1)
        bflib.beamform(derived.bp, derived.rf, acq.filters)
        single_pairs = int(last_timings(bflib).das_pairs)
        assert single_pairs > 0
        counted, info = image(bflib, acq, rf, groups)
        assert int(last_timings(bflib).das_pairs) == single_pairs
        stages = [int(info.stage_kind[i]) for i in range(info.stage_count)]
        assert stages == [0xFFFF, int(S.Decode), int(S.DAS), 0xFFFE], stages
    finally:
        L.beamformer_hip_enable_pair_counting(0)
    assert same_bits(plain, counted)
