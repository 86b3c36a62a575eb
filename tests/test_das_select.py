"""The DAS kernel selection (csrc/das_select.cpp) on the CPU: beamformer_hip_describe_das needs no device.
(1) the named cases get the kernel written down for them (tests/cases.py EXPECTED_AUTOMATIC) and every kernel not taken says why;
(2) PROPERTY: whenever the LDS-staged kernel is chosen, the delay spread of EVERY tile fits the window the host chose -- brute force
    in float64 over random row-column geometries (plane and focused transmits, ragged grids), restating only the index formula of
    das.glsl:126-130, :187-231 and the kernel's window construction (das_staged.hip: element floor(min R) + floor(min T) + j)."""
import pytest

from ogl_beamforming_amd import configs as cfg
from ogl_beamforming_amd import lib
from ogl_beamforming_amd import params as P
from tests import cases, staged_window


@pytest.mark.parametrize("name", sorted(cases.EXPECTED_AUTOMATIC))
def test_automatic_selection_of_the_named_cases(name):
    acq = cases.make(name)
    lib.library().beamformer_hip_set_das_path(0)
    path, kernel, label, reasons, d = lib.describe_das(acq.bp, acq.filters)
    assert path == cases.EXPECTED_AUTOMATIC[name], (kernel, reasons)
    assert int(d.row_end_planes) == cases.EXPECTED_ROW_END_PLANES.get(name, 0)
    assert kernel.startswith("das_") and label
    assert not reasons[path]
    assert all(reasons[k] for k in (1, 2, 3, 4) if k != path), reasons


def test_forced_paths_and_reasons():
    L = lib.library()
    acq = cases.make("rca_staged_auto")
    try:
        L.beamformer_hip_set_das_path(1)
        path, _, _, reasons, _ = lib.describe_das(acq.bp, acq.filters)
        assert path == 0 and "general kernel was asked for" in reasons[2]
        L.beamformer_hip_set_das_path(2)
        path, _, _, reasons, _ = lib.describe_das(acq.bp, acq.filters)
        assert path == 1 and "no LDS staging" in reasons[2]
        L.beamformer_hip_set_das_path(4)
        assert lib.describe_das(acq.bp, acq.filters)[0] == 3
        L.beamformer_hip_set_das_path(0)
        # the uniform-table form falls back to the tables in LDS when the global table may not be allocated
        fine = cases.make("rca_staged_fine")
        _, _, _, _, d = lib.describe_das(fine.bp, fine.filters)
        assert d.uniform_tables == 1 and d.u_shift == 6 and d.v_shift == 4
        lib.set_hook("STAGED_TABLE_CAP", "1")
        path, _, _, _, d = lib.describe_das(fine.bp, fine.filters)
        assert path == 2 and d.uniform_tables == 0
    finally:
        lib.set_hook("STAGED_TABLE_CAP", None)
        L.beamformer_hip_set_das_path(0)


@pytest.mark.parametrize("name", sorted(cases.STAGED_SHAPES_TAKEN))
def test_staged_shapes_of_the_real_and_cubic_kernels_are_taken(name):
    """das path 3 under BEAMFORMER_HIP_STAGED_SHAPE: the planner takes the staged kernel at every shape listed for the case -- each
    (V, W) instantiation of the real-sample and of the cubic kernel -- so the GPU test over these shapes runs the kernel it names"""
    acq = cases.make(name)
    L = lib.library()
    L.beamformer_hip_set_das_path(3)
    try:
        for shape in cases.STAGED_SHAPES_TAKEN[name]:
            lib.set_hook("STAGED_SHAPE", shape)
            path, kernel, _, reasons, d = lib.describe_das(acq.bp, acq.filters)
            u, v, w = (int(x) for x in shape.split(","))
            assert path == int(P.DasPath.Staged), (shape, kernel, reasons[2])
            assert (int(d.u_shift), int(d.v_shift), int(d.window_samples)) == (u, v, 1 << w), shape
        assert {(s.split(",")[1], s.split(",")[2]) for s in cases.STAGED_SHAPES_TAKEN[name]} == {(v, w) for v in "456" for w in "56"}
    finally:
        lib.set_hook("STAGED_SHAPE", None)
        L.beamformer_hip_set_das_path(0)


def test_block_staged_kernel_selection():
    """das_tile.hip (path 5): automatic for BASELINE config 2 at full size (fine grid, cubic IQ, tx and rx on one axis: 64 x 16 tiles,
    32-sample windows -- the derivative bound says 27.9 samples, the spread sampled on the image's extreme tiles 26 --, the banded plane walk), declined with its reason on small frames (channel split), under flag 0x200, for other
    sample kinds; flag 0x100 asks for it wherever the kernel is able to run, with the 32-sample window on very fine grids."""
    L = lib.library()
    try:
        L.beamformer_hip_set_das_path(0)
        full = cfg.config(2)
        path, kernel, _, reasons, d = lib.describe_das(full.bp, full.filters)
        assert (path, kernel) == (5, "das_tile_kernel") and "block-staged" in reasons[3]
        assert list(d.tile_shift) == [6, 4, 0] and list(d.blocks) == [16, 64, 1] and d.tile_window_samples == 32 and d.tile_walk == 3
        assert 20.0 <= d.tile_spread_estimate <= 26.0 and list(d.tile_estimate_shift) == [6, 4, 0]
        L.beamformer_hip_set_das_path(0x200)
        path, _, _, reasons, d = lib.describe_das(full.bp, full.filters)
        assert path == 3 and "0x200" in reasons[5] and d.tile_window_samples == 0
        # frames under the channel-split size: from 192 blocks the block-staged kernel runs instead of the split one (480^2: 8 x 30)
        L.beamformer_hip_set_das_path(0)
        for points, want in ((480, 5), (384, 3)):
            full.bp.output_points[0] = full.bp.output_points[1] = points
            path, _, _, _, d = lib.describe_das(full.bp, full.filters)
            assert path == want and (d.split_shift == 0) == (want == 5), (points, path, d.split_shift)
        L.beamformer_hip_set_das_path(0)
        small = cases.make("config2_small")
        path, _, _, reasons, _ = lib.describe_das(small.bp, small.filters)
        assert path == 3 and "channel split" in reasons[5]
        real = cases.make("forces")
        assert "cubic interpolation of IQ samples only" in lib.describe_das(real.bp, real.filters)[3][5]
        coarse = cfg.harness("tpw")
        L.beamformer_hip_set_das_path(0x10)
        path, _, _, reasons, _ = lib.describe_das(coarse.bp, coarse.filters)
        assert path == 3 and "coarse grid" in reasons[5]
        # asked for on the harness plane, the block-staged kernel is taken away again by the ROW-END rule: at F# 0.5 the outermost channels of
        # the deepest pixels echo from beyond the 2048 samples a row holds, and das_tile.hip carries no exact evaluation of such terms
        # (csrc/das_exact.h; the factored kernel behind it does)
        L.beamformer_hip_set_das_path(0x14 | 0x100)
        path, _, _, _, d = lib.describe_das(coarse.bp, coarse.filters)
        assert path == 3 and d.row_end_planes == 1
        fine = cases.make("tile_w32")
        path, _, _, _, d = lib.describe_das(fine.bp, fine.filters)
        assert path == 5 and d.tile_window_samples == 32
    finally:
        L.beamformer_hip_set_das_path(0)


@pytest.mark.parametrize("seed", range(40))
def test_staged_window_holds_every_tile_brute_force(seed):
    """random separable row-column acquisitions: the window plan_staged chose holds (max R - floor min R) + (max T - floor min T)
    of every tile, with the taps and the rounding of the position (linear: round(p) <= W - 2, p = R' + T'' and T'' carries - 1/2;
    cubic: segment n <= W - 3).  Generator, brute force and bound live in tests/staged_window.py (tests/test_poses_host.py runs them
    on posed geometry)"""
    acq, cubic = staged_window.property_draw(seed)
    held, reason = staged_window.window_holds(acq, cubic)
    if held is None:
        pytest.skip("declined by plan_staged: " + reason)


def test_full_size_configurations_stay_clear_of_row_ends_and_the_harness_planes_do_not():
    """the host bound per plane (das_select.cpp plane_index_bounds): BASELINE configs 2-5 at full size have no in-aperture term within
    reach of an end of its RF row -- their kernels run the instantiation without any row-end code, as in round 3 --, while on the
    reference harness's own F# 0.5 view plane the outermost channels of the deepest pixels echo from beyond the row's 2048 samples"""
    lib.library().beamformer_hip_set_das_path(0)
    for n in (2, 3, 4, 5):
        acq = cfg.config(n)
        d = lib.describe_das(acq.bp, acq.filters)[4]
        assert int(d.row_ends) == 0 and int(d.row_end_planes) == 0, n
    for kind in ("tpw", "forces", "hercules"):
        acq = cfg.harness(kind)
        d = lib.describe_das(acq.bp, acq.filters)[4]
        assert int(d.row_ends) == 1 and int(d.row_end_planes) == 0, kind


def test_random_view_planes_select_the_plane_kernels():
    """the view-plane generator of tests/draws.py (the reference harness's shape at test size) is aimed at the HERCULES aligned-grid
    kernel and at the factored kernel: the selection rules say so without a device (small frames: with the channel split switched off,
    flag 0x10, as the GPU test and the fuzz ask for them)"""
    from tests import draws as R
    L = lib.library()
    taken = {}
    L.beamformer_hip_set_das_path(0x10)
    try:
        for seed in range(24):
            acq = R.draw_plane(seed)
            path, kernel, _, _, d = lib.describe_das(acq.bp, acq.filters)
            hercules = int(acq.bp.acquisition_kind) in (int(P.AcquisitionKind.HERCULES), int(P.AcquisitionKind.UHERCULES))
            taken.setdefault(hercules, set()).add(path)
    finally:
        L.beamformer_hip_set_das_path(0)
    assert taken[True] == {int(P.DasPath.Hercules)}, taken
    assert int(P.DasPath.Factored) in taken[False] and int(P.DasPath.Hercules) not in taken[False], taken


def test_random_paired_draws_are_planned_in_the_channel_paired_form():
    """tests/draws.py draw_paired, asked for the LDS-staged kernel in 32 x 32 tiles with 32-sample windows (path 3, STAGED_SHAPE 5,5,5, as
    tests/test_gpu_staged_paired.py runs them): the channel-paired form (uniform_tables 2) is planned for nearly every draw, across one and
    two transmit groups, padded transmit counts and odd channel counts; never for more than two groups; and the short-row draws hand
    their deepest plane to the kernel behind the staged one"""
    from tests import draws
    L = lib.library()
    paired, other, short = [], [], []
    lib.set_hook("STAGED_SHAPE", "5,5,5")
    L.beamformer_hip_set_das_path(3)
    try:
        for seed in range(24):
            acq = draws.draw_paired(seed)
            path, kernel, _, reasons, d = lib.describe_das(acq.bp, acq.filters)
            C, A = int(acq.bp.channel_count), int(acq.bp.acquisition_count)
            if d.uniform_tables == 2:
                assert path == 2 and d.u_shift == 5 and d.v_shift == 5 and d.window_samples == 32 and d.threads == 1024, (seed, kernel)
                paired.append((seed, C, A))
            else:
                other.append((seed, C, A, path, int(d.uniform_tables)))
            if A > 120:
                # the padded transmit table (A rounded up to 4) splits into groups of at most 60 transmits whose two channel windows fit the
                # LDS (das_select.cpp plan_staged, BF_STAGED_PAIRED_GROUP_MAX); the paired form takes at most two such groups
                assert d.uniform_tables != 2, f"seed {seed}: {A} transmits need {-(-((A + 3) // 4 * 4) // 60)} groups of 60, the paired form was planned"
            if acq.notes == "short rows":
                assert d.row_end_planes > 0 and d.row_end_path == 1, (seed, int(d.row_end_planes), int(d.row_end_path))
                short.append(seed)
            else:
                assert d.row_end_planes == 0 and d.row_end_path == -1, seed
    finally:
        lib.set_hook("STAGED_SHAPE", None)
        L.beamformer_hip_set_das_path(0)
    assert len(paired) >= 20, (paired, other)
    assert any(A <= 60 for _, _, A in paired) and any(A > 60 for _, _, A in paired), paired           # one group and two groups
    assert any(A % 4 for _, _, A in paired) and any(C % 2 for _, C, _ in paired), paired               # padded tables, a zero partner
    assert any(A > 120 for _, _, A, _, _ in other) and short, (other, short)


@pytest.mark.parametrize("seed", [120, 160, 385, 439])
def test_planes_rerouted_from_the_block_staged_kernel_keep_the_factored_kernel_asked_for(seed):
    """mode 0x114 asks for the factored kernel with block staging (das_tile.hip) and no channel split; on these short-row volumes of the
    separable generator (tests/test_gpu_random.py ROW_END_SEPARABLE) the row-end rule takes planes away from the block-staged kernel, and
    those run the factored kernel asked for (nibble 4 with block staging off), not "automatic, never staged".  Mode 3 on a linear draw
    of the same generator (107) sends its re-routed plane to the gather kernel"""
    from tests import draws
    L = lib.library()
    acq = draws.draw_separable(seed)
    try:
        L.beamformer_hip_set_das_path(0x114)
        path, _, _, _, d = lib.describe_das(acq.bp, acq.filters)
        assert d.row_end_planes > 0 and d.row_end_path == int(P.DasPath.Factored), (path, int(d.row_end_planes), int(d.row_end_path))
        linear = draws.draw_separable(107)
        assert linear.bp.interpolation_mode == int(P.InterpolationMode.Linear)
        L.beamformer_hip_set_das_path(3)
        path, _, _, _, d = lib.describe_das(linear.bp, linear.filters)
        assert path == int(P.DasPath.Staged) and d.row_end_planes == 1 and d.row_end_path == int(P.DasPath.Gather)
    finally:
        L.beamformer_hip_set_das_path(0)
