"""HIP path vs CPU oracle through the C ABI (include/ogl_beamformer_lib.h) -- the parity
tests proper.  Every case pushes parameters and RF exactly as a client of the reference
would (tests/throughput.c:422-491) and compares the pulled image with the oracle's
restatement of the reference shaders on the same seeded input."""
import numpy as np
import pytest

from ogl_beamforming_amd import params as P
from tests import cases
from tests.das_kernel_cases import FACTORED, HERCULES, SEPARABLE, STAGED, TILE
from tests.das_push import compare, last_das_path, last_timings
from tests.parity import reference

pytestmark = pytest.mark.gpu

EXPECTED_AUTOMATIC = cases.EXPECTED_AUTOMATIC


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_frame_parity(name, bflib, oracle):
    """default (automatic) DAS path"""
    acq = cases.make(name)
    ref, pairs, flags = reference(oracle, acq)
    bflib.library().beamformer_hip_set_das_path(0)
    gpu = bflib.beamform(acq.bp, acq.rf, acq.filters)
    path, kernel, _, reasons, _ = bflib.describe_das(acq.bp, acq.filters)
    assert last_das_path(bflib) == path, (kernel, reasons)
    if name in EXPECTED_AUTOMATIC:
        assert path == EXPECTED_AUTOMATIC[name], (name, kernel, reasons)
    assert all(reasons[k] for k in (1, 2, 3, 4) if k != path), reasons          # every kernel not taken says why
    compare(gpu, ref, acq, flags)


@pytest.mark.parametrize("name", sorted(SEPARABLE))
def test_general_kernel_on_separable_geometry(name, bflib, oracle):
    """the general kernel on the cases the fast path would otherwise take"""
    acq = cases.make(name)
    ref, pairs, flags = reference(oracle, acq)
    lib = bflib.library()
    lib.beamformer_hip_set_das_path(1)
    try:
        gpu = bflib.beamform(acq.bp, acq.rf, acq.filters)
        assert last_das_path(bflib) == 0
    finally:
        lib.beamformer_hip_set_das_path(0)
    compare(gpu, ref, acq, flags)


@pytest.mark.parametrize("name", sorted(STAGED))
def test_gather_kernel_where_the_staged_kernel_applies(name, bflib, oracle):
    """path 2: automatic, but never staged -- the separable-delay gather kernel for linear interpolation, the factored
    kernel for cubic (as before the staged kernels existed)"""
    acq = cases.make(name)
    ref, pairs, flags = reference(oracle, acq)
    lib = bflib.library()
    lib.beamformer_hip_set_das_path(2)
    try:
        gpu = bflib.beamform(acq.bp, acq.rf, acq.filters)
        path = bflib.describe_das(acq.bp, acq.filters)[0]
        assert path in (1, 3) and last_das_path(bflib) == path
        if acq.bp.interpolation_mode == int(P.InterpolationMode.Linear):
            assert path == 1
    finally:
        lib.beamformer_hip_set_das_path(0)
    compare(gpu, ref, acq, flags)


@pytest.mark.parametrize("name", sorted(SEPARABLE))
def test_lds_staged_kernel(name, bflib, oracle):
    """the LDS-staged kernel on request (these acquisitions have fewer transmits than its automatic
    threshold); geometries outside its window bound fall back to the gather kernel"""
    acq = cases.make(name)
    ref, pairs, flags = reference(oracle, acq)
    lib = bflib.library()
    lib.beamformer_hip_set_das_path(3)
    try:
        gpu = bflib.beamform(acq.bp, acq.rf, acq.filters)
        assert last_das_path(bflib) == (2 if name in STAGED and name not in cases.ROW_END_EVERY_PLANE else 1)
    finally:
        lib.beamformer_hip_set_das_path(0)
    compare(gpu, ref, acq, flags)


@pytest.mark.parametrize("shape", ["5,4,5", "4,5,5", "6,4,5", "5,5,5", "4,6,5", "5,4,6", "4,5,6", "6,4,6", "5,5,6", "4,6,6"])
@pytest.mark.parametrize("name", ["rca_staged_auto", "rca_staged_ragged", "rca_staged_cubic_short_rows", "rca_staged_real_narrow_cw"])
def test_lds_staged_kernel_every_tile_and_window_shape(name, shape, bflib, oracle, hooks):
    """BEAMFORMER_HIP_STAGED_SHAPE = "log2 U, log2 V, log2 W": each instantiation of the staged kernel (tile extents along
    the receive / transmit axes, 32- or 64-sample windows, 512- and 1024-thread blocks) instead of the shape the host would
    pick; a shape whose window cannot hold the tile's delay spread is declined and the gather kernel runs"""
    acq = cases.make(name)
    ref, pairs, flags = reference(oracle, acq)
    lib = bflib.library()
    hooks.set("STAGED_SHAPE", shape)
    hooks.set("STAGED_CHECKED")                  # every term range-checked: window violations are counted
    lib.beamformer_hip_set_das_path(3)
    try:
        gpu = bflib.beamform(acq.bp, acq.rf, acq.filters)
        path = last_das_path(bflib)
        assert path in (1, 2)
        assert last_timings(bflib).staged_window_violations == 0
        if shape in ("5,4,6", "4,5,6", "5,5,6", "4,6,6") and name == "rca_staged_auto":
            assert path == 2                     # a 64-sample window holds this case's spread for tiles up to 32 voxels along the receive axis
    finally:
        lib.beamformer_hip_set_das_path(0)
    compare(gpu, ref, acq, flags)


@pytest.mark.parametrize("shape", ["6,4,5", "6,4,6"])
@pytest.mark.parametrize("name", ["rca_staged_fine", "rca_staged_fine_vls_short_rows", "rca_staged_auto"])
def test_lds_staged_kernel_uniform_tables(name, shape, bflib, oracle, hooks, capfd):
    """64 x 16 tiles with x along the receive axis: the transmit delays and phasors of a wave are uniform and come from a global
    table (written per frame by a pre-pass) through scalar loads instead of from LDS.  Same arithmetic: the frame is
    BIT-IDENTICAL to the one the same tile shape gives with the tables in LDS (BEAMFORMER_HIP_STAGED_NOUNIFORM), and both
    are the oracle's."""
    acq = cases.make(name)
    ref, pairs, flags = reference(oracle, acq)
    lib = bflib.library()
    hooks.set("STAGED_SHAPE", shape)
    hooks.set("DEBUG")
    lib.beamformer_hip_set_das_path(3)
    try:
        capfd.readouterr()
        uniform = bflib.beamform(acq.bp, acq.rf, acq.filters)
        path_uniform = last_das_path(bflib)
        log = capfd.readouterr().err
        hooks.set("STAGED_NOUNIFORM")
        tables_in_lds = bflib.beamform(acq.bp, acq.rf, acq.filters)
        path_lds = last_das_path(bflib)
        log_lds = capfd.readouterr().err
    finally:
        lib.beamformer_hip_set_das_path(0)
    assert path_uniform == path_lds
    if path_uniform == 2:
        assert "uniform 1" in log and "uniform 1" not in log_lds, (log, log_lds)
        if path_lds == 2:
            assert np.array_equal(np.asarray(uniform).view(np.uint32), np.asarray(tables_in_lds).view(np.uint32))
    if name == "rca_staged_fine":
        assert path_uniform == 2                 # (rca_staged_auto's coarse grid fits no window 64 voxels wide, the focused transmits'
                                                 #  spread not every window: declined either way, the gather kernel runs)
    compare(uniform, ref, acq, flags)
    if path_lds == 1 and path_uniform == 2:
        compare(tables_in_lds, ref, acq, flags)


@pytest.mark.parametrize("name", sorted(STAGED))
def test_lds_staged_kernel_checked_loop_everywhere(name, bflib, oracle, hooks):
    """BEAMFORMER_HIP_STAGED_CHECKED: every wave of the staged kernel runs the range-checked loop (normally only the
    waves that can leave the RF row do): the oracle's frame either way"""
    acq = cases.make(name)
    ref, pairs, flags = reference(oracle, acq)
    lib = bflib.library()
    hooks.set("STAGED_CHECKED")
    lib.beamformer_hip_set_das_path(3)
    try:
        gpu = bflib.beamform(acq.bp, acq.rf, acq.filters)
        assert last_das_path(bflib) == (1 if name in cases.ROW_END_EVERY_PLANE else 2)
        assert last_timings(bflib).staged_window_violations == 0, "a term left its staged window: plan_staged's bound is wrong"
    finally:
        lib.beamformer_hip_set_das_path(0)
    compare(gpu, ref, acq, flags)


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_general_kernel_without_channel_split(name, bflib, oracle):
    """These acquisitions are small, so the default launch splits the channel loop over waves;
    0x11 forces the one-thread-per-voxel form of the same kernel that full-size frames use."""
    acq = cases.make(name)
    ref, pairs, flags = reference(oracle, acq)
    lib = bflib.library()
    lib.beamformer_hip_set_das_path(0x11)
    try:
        gpu = bflib.beamform(acq.bp, acq.rf, acq.filters)
        assert last_das_path(bflib) == 0
    finally:
        lib.beamformer_hip_set_das_path(0)
    compare(gpu, ref, acq, flags)


@pytest.mark.parametrize("name", HERCULES)
def test_hercules_aligned_kernel(name, bflib, oracle):
    """das_hercules.hip on every HERCULES-family case (mode 6 also takes the grids too narrow for the
    automatic rule): both loop orders, sparse transmits, every interpolation, real and IQ data, with and
    without coherency weighting, checked and unchecked inner loops"""
    acq = cases.make(name)
    ref, pairs, flags = reference(oracle, acq)
    lib = bflib.library()
    lib.beamformer_hip_set_das_path(6)
    try:
        gpu = bflib.beamform(acq.bp, acq.rf, acq.filters)
        assert last_das_path(bflib) == 4
    finally:
        lib.beamformer_hip_set_das_path(0)
    compare(gpu, ref, acq, flags)


def test_hercules_coherent_peak_at_long_delays(bflib, oracle):
    """A point scatterer seen by a 64 x 64 HERCULES aperture at sample indices around 1400 (Float32Complex RF
    straight into DAS): at a coherent peak a systematic error of the delay scale shows undiluted -- 1.9e-8
    relative (the rounding of 1/c) is 1.2e-4 rad of phase, the whole 1e-4 budget.  Both HERCULES kernels
    against the oracle at 1e-4 of the peak."""
    from ogl_beamforming_amd import configs as cfg
    C_, A, S, fs, fd, pitch = 64, 64, 2048, 12.5e6, 6.25e6, 0.2e-3
    half = (C_ - 1) / 2 * pitch
    point = np.array([0.7e-3, -0.4e-3, 80e-3])
    acq = cfg.hercules("hercules_peak", C_, A, S, (64, 6, 5), (point[0] - 1.6e-3, point[1] - 0.3e-3, point[2] - 0.3e-3),
                       (point[0] + 1.6e-3, point[1] + 0.3e-3, point[2] + 0.3e-3), seed=61, data_kind=P.DataKind.Float32Complex,
                       decode=0, pitch=pitch, fs=fs, fd=fd, f_number=0.5, cw=False, noise_sigma=0.05)
    # echo of the scatterer: plane-wave transmit (distance z), receive element (c, t) at (c pitch, t pitch) in
    # transducer space = world + half (cfg.hercules' xdc transform); baseband: envelope x e^{-j 2 pi fd t0}
    xs = np.arange(C_) * pitch - half
    ys = np.arange(A) * pitch - half
    dist = point[2] + np.sqrt(point[2] ** 2 + (point[0] - xs[:, None]) ** 2 + (point[1] - ys[None, :]) ** 2)
    n0 = (dist / cfg.SPEED_OF_SOUND * fs).reshape(-1)
    iq = acq.rf.reshape(C_ * A, S, 2)
    offsets = np.arange(-24, 25)
    idx = np.floor(n0).astype(np.int64)[:, None] + offsets[None, :]
    env = 4.0 * np.exp(-((idx - n0[:, None]) / 10.0) ** 2)
    phase = -2.0 * np.pi * fd * (n0 / fs)
    rows = np.broadcast_to(np.arange(C_ * A)[:, None], idx.shape)
    np.add.at(iq[:, :, 0], (rows, idx), (env * np.cos(phase)[:, None]).astype(np.float32))
    np.add.at(iq[:, :, 1], (rows, idx), (env * np.sin(phase)[:, None]).astype(np.float32))
    assert 1200 < n0.min() and n0.max() < 1700
    ref, pairs, _ = reference(oracle, acq)
    peak = np.abs(ref).max()
    assert peak > 0.5 * 4.0 * C_ * A * 0.5                      # coherent: most of the 4096 taps add up
    lib = bflib.library()
    for mode, want_path in ((6, 4), (0x11, 0)):
        lib.beamformer_hip_set_das_path(mode)
        try:
            gpu = bflib.beamform(acq.bp, acq.rf, acq.filters)
            assert last_das_path(bflib) == want_path
        finally:
            lib.beamformer_hip_set_das_path(0)
        err = np.abs(gpu - ref).max() / peak
        assert err <= 1e-4, (mode, err)


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("name", FACTORED)
def test_factored_kernel(name, split, bflib, oracle):
    """das_factored.hip wherever the index factorises -- also on the geometries the gather
    kernel would take and with fewer transmits than the automatic rule asks for -- with the
    channel split these small frames get by default and without it"""
    acq = cases.make(name)
    ref, pairs, flags = reference(oracle, acq)
    lib = bflib.library()
    lib.beamformer_hip_set_das_path(0x04 if split else 0x14)
    try:
        gpu = bflib.beamform(acq.bp, acq.rf, acq.filters)
        assert last_das_path(bflib) == 3
    finally:
        lib.beamformer_hip_set_das_path(0)
    compare(gpu, ref, acq, flags)


_I = P.InterpolationMode
# (case, interpolation mode, coherency weighting, das path mode, the DAS path the frame must report): the instantiations of the general,
# HERCULES, separable-gather and factored kernels that no case of cases.CASES dispatches as it stands -- real samples with coherency
# weighting, or another interpolation mode of the FORCES cases -- on the smallest case of the family, with the two fields set in its
# parameter block.  Reference and bars are every other test's here: the oracle on the same block, compare().
DISPATCH = [("hercules_real", _I.Nearest, 1, 6, 4), ("hercules_real", _I.Cubic, 1, 6, 4),            # das_hercules.hip
            ("hercules_real", _I.Nearest, 1, 0x11, 0), ("hercules_real", _I.Cubic, 1, 0x11, 0),      # das.hip, HERCULES
            ("forces", _I.Nearest, 0, 0x11, 0), ("forces", _I.Cubic, 0, 0x11, 0),                    # das.hip, FORCES
            ("rca_sep_real_nearest", _I.Nearest, 1, 3, 1), ("rca_sep_real_nearest", _I.Cubic, 1, 3, 1),   # das_separable.hip
            ("rca_cubic_real", _I.Cubic, 1, 0x04, 3), ("rca_staged_real", _I.Cubic, 1, 0x04, 3),     # das_factored.hip, RCA: rows that end, and not
            ("forces", _I.Linear, 1, 0x04, 3), ("forces", _I.Cubic, 0, 0x04, 3)]                     # das_factored.hip, FORCES


@pytest.mark.parametrize("name,interp,cw,mode,want", DISPATCH,
                         ids=[f"{n}-{i.name.lower()}-{'cw' if c else 'plain'}-{m:#x}" for n, i, c, m, _ in DISPATCH])
def test_kernel_instances_no_case_dispatches_as_it_stands(name, interp, cw, mode, want, bflib, oracle):
    acq = cases.make(name)
    acq.bp.interpolation_mode = int(interp)
    acq.bp.coherency_weighting = cw
    ref, pairs, flags = reference(oracle, acq)
    lib = bflib.library()
    lib.beamformer_hip_set_das_path(mode)
    try:
        gpu = bflib.beamform(acq.bp, acq.rf, acq.filters)
        assert last_das_path(bflib) == want
    finally:
        lib.beamformer_hip_set_das_path(0)
    compare(gpu, ref, acq, flags)


DECODING = sorted(n for n in cases.CASES
                  if cases.make(n).bp.decode_mode and int(P.ShaderKind.Decode) in list(cases.make(n).bp.compute_stages[:cases.make(n).bp.compute_stages_count]))


@pytest.mark.parametrize("name", DECODING)
def test_decode_dense_kernel_and_fwht_agree(name, bflib, oracle):
    """Decode runs as a fast Walsh-Hadamard transform wherever the matrix is Sylvester (x) base
    (orders 2^k, 12*2^k, 20*2^k); 0x20 keeps the O(T^2) kernel.  Both match the oracle; on Int16
    RF decoded first every partial sum is an exact integer, so the two frames are bit-identical."""
    acq = cases.make(name)
    ref, pairs, flags = reference(oracle, acq)
    lib = bflib.library()
    fast = bflib.beamform(acq.bp, acq.rf, acq.filters)
    compare(fast, ref, acq, flags)
    lib.beamformer_hip_set_das_path(0x20)
    try:
        dense = bflib.beamform(acq.bp, acq.rf, acq.filters)
    finally:
        lib.beamformer_hip_set_das_path(0)
    compare(dense, ref, acq, flags)
    stages = list(acq.bp.compute_stages[: acq.bp.compute_stages_count])
    if acq.bp.data_kind == int(P.DataKind.Int16) and stages[0] == int(P.ShaderKind.Decode):
        assert np.array_equal(fast, dense, equal_nan=True)


def test_pair_count_matches_oracle(bflib, oracle):
    """G of the roofline model: the geometry-only count kernel agrees with the oracle's tally
    of taken apodization branches (exactly, up to aperture-edge rounding)."""
    import ctypes as C
    lib = bflib.library()
    for name in ("config4_small", "rca_vls_cw", "hercules_real", "forces"):
        acq = cases.make(name)
        _, pairs = oracle.beamform(acq.bp, acq.rf, acq.filters)
        lib.beamformer_hip_enable_pair_counting(1)
        try:
            bflib.beamform(acq.bp, acq.rf, acq.filters)
            t = P.HipFrameTimings()
            assert lib.beamformer_hip_get_last_frame_timings(C.byref(t))
        finally:
            lib.beamformer_hip_enable_pair_counting(0)
        assert abs(int(t.das_pairs) - pairs) <= max(4, 2e-4 * pairs), (name, int(t.das_pairs), pairs)


# what the block does with its (block, chunk of four channels) pairs -- staged windows, or the kernel's own gather loop where the
# spread of the chunk does not fit the window (BeamformerHipFrameTimings::tile_staged_chunks / tile_gather_chunks)
TILE_STAGED_ONLY = {"tile_tpw", "tile_tpw_w64", "tile_w32", "tile_forces", "tile_uforces_cw", "tile_thin_volume"}
TILE_BOTH        = {"tile_near_field"}
TILE_WINDOW      = {"tile_w32": 32, "tile_tpw": 32, "tile_tpw_w64": 64, "tile_near_field": 64}
# fine-grid cases whose RF rows END inside the image: the row-end rule (csrc/das_exact.h, das_select.h decide_das_parts) hands their plane to
# the factored kernel, which evaluates the terms at the row ends with the shader's own index
TILE_ROW_END     = {"tile_tpw_cw_short", "tile_vls"}


def test_block_staging_candidates():
    assert TILE_STAGED_ONLY | TILE_BOTH <= set(TILE), TILE
    assert not (TILE_ROW_END & set(TILE)), TILE
    assert len(TILE) >= 10, TILE


@pytest.mark.parametrize("name", sorted(TILE_ROW_END))
def test_block_staging_declined_where_rows_end_inside_the_image(name, bflib, oracle):
    acq = cases.make(name)
    ref, pairs, flags = reference(oracle, acq)
    lib = bflib.library()
    try:
        lib.beamformer_hip_set_das_path(0x14 | 0x100)
        gpu = np.asarray(bflib.beamform(acq.bp, acq.rf, acq.filters)).copy()
        t = last_timings(bflib)
        assert int(t.das_path) == 3 and int(t.das_row_end_planes) == max(1, acq.bp.output_points[2])
    finally:
        lib.beamformer_hip_set_das_path(0)
    compare(gpu, ref, acq, flags)


@pytest.mark.parametrize("name", TILE)
def test_factored_kernel_block_staging(name, bflib, oracle):
    """das_tile.hip (flag 0x100: a 1024-thread block stages the RF windows of its 64 x 16 voxels as cubic polynomials in LDS;
    automatic on fine grids with tx and rx on one axis -- BASELINE config 2) against the oracle, and that das_factored.hip's
    gather loop runs instead under flag 0x200 (the polynomial re-expansion rounds differently: parity tolerance, not bit for bit).
    Fine-grid cases must really be served from the staged windows, the near-field case by both kinds of chunk; the coarse harness
    frames exercise the kernel's own fallback."""
    acq = cases.make(name)
    ref, pairs, flags = reference(oracle, acq)
    lib = bflib.library()
    try:
        lib.beamformer_hip_set_das_path(0x14 | 0x100)
        if name in TILE_WINDOW:
            assert int(bflib.describe_das(acq.bp, acq.filters)[4].tile_window_samples) == TILE_WINDOW[name]
        lib.beamformer_hip_enable_pair_counting(1)         # (the count runs with the general kernel's tiles, not the block's)
        tile = np.asarray(bflib.beamform(acq.bp, acq.rf, acq.filters)).copy()
        t = last_timings(bflib)
        assert int(t.das_path) == 5
        assert abs(int(t.das_pairs) - pairs) <= max(4, 2e-4 * pairs), (int(t.das_pairs), pairs)
        staged, gathered = int(t.tile_staged_chunks), int(t.tile_gather_chunks)
        assert staged + gathered > 0
        if name in TILE_STAGED_ONLY:
            assert staged > 0 and gathered == 0, (staged, gathered)
        if name in TILE_BOTH:
            assert staged > 0 and gathered > 0, (staged, gathered)
        lib.beamformer_hip_enable_pair_counting(0)
        lib.beamformer_hip_set_das_path(0x14 | 0x200)
        np.asarray(bflib.beamform(acq.bp, acq.rf, acq.filters))
        assert last_das_path(bflib) != 5
    finally:
        lib.beamformer_hip_enable_pair_counting(0)
        lib.beamformer_hip_set_das_path(0)
    compare(tile, ref, acq, flags)


@pytest.mark.parametrize("name", ["tile_near_field", "tile_tpw_w64", "tile_thin_volume"])
def test_block_staged_kernel_is_deterministic(name, bflib):
    """das_tile.hip hands LDS windows from 1024 staging threads to 1024 consumers across two buffers and four kinds of barrier: a missing
    one shows as a frame that differs from run to run.  Forty frames of the same push, bit for bit (staged and gathered chunks, both
    window lengths, a tile over two planes)."""
    acq = cases.make(name)
    lib = bflib.library()
    try:
        lib.beamformer_hip_set_das_path(0x14 | 0x100)
        first = np.asarray(bflib.beamform(acq.bp, acq.rf, acq.filters)).copy()
        assert last_das_path(bflib) == 5
        for k in range(39):
            again = np.asarray(bflib.beamform(acq.bp, acq.rf, acq.filters))
            assert np.array_equal(first.view(np.uint32), again.view(np.uint32)), f"frame {k + 2} differs from the first"
    finally:
        lib.beamformer_hip_set_das_path(0)
