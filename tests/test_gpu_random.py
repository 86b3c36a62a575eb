"""Randomised parity: 48 seeded small acquisitions drawn over family x geometry x interpolation
x element kind x stages x f-number x coherency weighting x per-transmit orientations / focal
depths, each beamformed through the C ABI on the automatic DAS path and compared with the
oracle (same tolerances as tests/test_gpu_parity.py).  Complements the named cases: the
combinations here are not hand-picked."""
import numpy as np
import pytest

from ogl_beamforming_amd import params as P
from tests.das_push import compare, last_das_path, last_timings
from tests.draws import K, draw, draw_plane, draw_separable, draw_tile  # noqa: F401  (the generators live in tests/draws.py)
from tests.parity import reference

pytestmark = pytest.mark.gpu


STAGED_DRAWS = []          # (seed, form: uniform_tables 0 / 1 / 2) of the draws whose staged pass ran the LDS-staged kernel (reported below)


# 1001: round 4's out-of-sample fuzz draw whose median error on the gather kernel (1.4e-5: the phase of 96 turns rounded once more than the
# shader rounds it) is the size of the float oracle's own distance from its double twin -- the draw behind compare()'s median rule
@pytest.mark.parametrize("seed", list(range(72)) + [1001])
def test_random_acquisition(seed, bflib, oracle, hooks):
    acq = draw(seed)
    ref, pairs, flags = reference(oracle, acq)
    ok = ~np.isnan(ref)
    if not ok.any() or np.max(np.abs(ref[ok])) == 0:
        pytest.skip("the draw produced an empty image (aperture closed everywhere)")
    bflib.library().beamformer_hip_set_das_path(0)
    gpu = bflib.beamform(acq.bp, acq.rf, acq.filters)
    compare(gpu, ref, acq, flags)
    # and the general kernel on the same input, whatever the automatic choice was
    first_path = last_das_path(bflib)
    if first_path != 0:
        bflib.library().beamformer_hip_set_das_path(1)
        try:
            gpu = bflib.beamform(acq.bp, acq.rf, acq.filters)
        finally:
            bflib.library().beamformer_hip_set_das_path(0)
        compare(gpu, ref, acq, flags)
    # row-column draws the gather kernel took also go through the LDS-staged kernel (path 3; it declines -- and the gather
    # kernel runs again -- when the interpolation is not linear, the data real or the delay spread too wide for a window)
    if first_path in (1, 2):
        bflib.library().beamformer_hip_set_das_path(3)
        hooks.set("STAGED_CHECKED")          # every term range-checked: a position outside its staged window is counted
        try:
            form = int(bflib.describe_das(acq.bp, acq.filters)[4].uniform_tables)
            gpu = bflib.beamform(acq.bp, acq.rf, acq.filters)
            t = last_timings(bflib)
            assert int(t.das_path) in (1, 2)
            assert int(t.staged_window_violations) == 0, "a term left its staged window: plan_staged's bound is wrong"
            if int(t.das_path) == 2:
                STAGED_DRAWS.append((seed, form))
        finally:
            hooks.clear("STAGED_CHECKED")
            bflib.library().beamformer_hip_set_das_path(0)
        compare(gpu, ref, acq, flags)
    # HERCULES-family draws also go through the aligned-grid kernel (forced: these grids are narrower than
    # the automatic rule asks for), whichever loop order and sparsity the draw produced
    if P.AcquisitionKind(acq.bp.acquisition_kind) in (P.AcquisitionKind.HERCULES, P.AcquisitionKind.UHERCULES, P.AcquisitionKind.HERO_PA):
        bflib.library().beamformer_hip_set_das_path(6)
        try:
            gpu = bflib.beamform(acq.bp, acq.rf, acq.filters)
            assert last_das_path(bflib) == 4
        finally:
            bflib.library().beamformer_hip_set_das_path(0)
        compare(gpu, ref, acq, flags)


@pytest.mark.parametrize("seed", range(32))
def test_random_separable_acquisition_on_the_staged_kernels(seed, bflib, oracle, hooks):
    """32 draws aimed at the LDS-staged kernels (the 72 general draws above reach them once): automatic path, every term
    range-checked with the window-violation count on, against the oracle"""
    acq = draw_separable(seed)
    ref, pairs, flags = reference(oracle, acq)
    ok = ~np.isnan(ref)
    if not ok.any() or np.max(np.abs(ref[ok])) == 0:
        pytest.skip("empty image")
    bflib.library().beamformer_hip_set_das_path(0)
    path, _, _, _, d = bflib.describe_das(acq.bp, acq.filters)
    gpu = bflib.beamform(acq.bp, acq.rf, acq.filters)
    assert last_das_path(bflib) == path
    compare(gpu, ref, acq, flags)
    if path == 2:
        hooks.set("STAGED_CHECKED")
        checked = bflib.beamform(acq.bp, acq.rf, acq.filters)
        t = last_timings(bflib)
        assert int(t.das_path) == 2 and int(t.staged_window_violations) == 0, "a term left its staged window: plan_staged's bound is wrong"
        compare(checked, ref, acq, flags)
        STAGED_DRAWS.append((100 + seed, int(d.uniform_tables)))


def test_random_draws_reach_the_staged_kernel():
    """how many draws exercised the LDS-staged kernels with the window-violation count on (none may be zero by luck), and in which form:
    transmit tables in LDS (0), global wave-uniform tables (1), channel-paired (2; aimed at by tests/test_gpu_staged_paired.py's draws)"""
    forms = {f: sum(1 for _, g in STAGED_DRAWS if g == f) for f in (0, 1, 2)}
    print(f"staged draws: {len(STAGED_DRAWS)}, by form (uniform_tables) {forms}: {STAGED_DRAWS}")
    assert len(STAGED_DRAWS) >= 12, STAGED_DRAWS


TILE_DRAWS = []            # (seed, staged chunks, gathered chunks) of the draws below that ran das_tile.hip


@pytest.mark.parametrize("seed", range(32))
def test_random_acquisition_on_the_block_staged_kernel(seed, bflib, oracle):
    """32 draws aimed at das_tile.hip, asked for with flag 0x100 (no channel split): against the oracle, with the counts of chunks
    served from staged windows and of chunks sent through the kernel's gather loop"""
    acq = draw_tile(seed)
    ref, pairs, flags = reference(oracle, acq)
    ok = ~np.isnan(ref)
    if not ok.any() or np.max(np.abs(ref[ok])) == 0:
        pytest.skip("empty image")
    lib = bflib.library()
    try:
        lib.beamformer_hip_set_das_path(0x10 | 0x100)
        path = bflib.describe_das(acq.bp, acq.filters)[0]
        gpu = bflib.beamform(acq.bp, acq.rf, acq.filters)
        t = last_timings(bflib)
        assert int(t.das_path) == path
    finally:
        lib.beamformer_hip_set_das_path(0)
    compare(gpu, ref, acq, flags)            # against the oracle, nothing else (round 3 accepted voxels on which another kernel agreed)
    if int(t.das_path) == 5:
        TILE_DRAWS.append((seed, int(t.tile_staged_chunks), int(t.tile_gather_chunks)))


def test_random_draws_reach_the_block_staged_kernel():
    """most draws must have run das_tile.hip, and between them both kinds of chunk in quantity"""
    print(f"block-staged draws: {len(TILE_DRAWS)}: {TILE_DRAWS}")
    assert len(TILE_DRAWS) >= 20, TILE_DRAWS
    # (draws whose rows end inside the image -- most of the coarse ones -- go to the factored kernel by the row-end rule)
    assert sum(1 for _, s, g in TILE_DRAWS if s > 0) >= 12 and sum(1 for _, s, g in TILE_DRAWS if g > 0) >= 1, TILE_DRAWS


PLANE_DRAWS = []           # (seed, das path, row-end planes) of the draws below


@pytest.mark.parametrize("seed", range(40))
def test_random_view_plane(seed, bflib, oracle):
    """40 random view planes against the oracle: on the automatic path, on the kernel a full-size plane of the kind gets (no channel split;
    HERCULES: the aligned-grid kernel asked for), and on the general kernel"""
    acq = draw_plane(seed)
    ref, pairs, flags = reference(oracle, acq)
    ok = ~np.isnan(ref)
    if not ok.any() or np.max(np.abs(ref[ok])) == 0:
        pytest.skip("the draw produced an empty image")
    lib = bflib.library()
    # automatic; without the channel split of small frames (0x10: the kernel a full-size plane gets); HERCULES: the aligned-grid kernel asked for
    # (6: small frames go to the general kernel's channel split by themselves); the general kernel
    modes = [0, 0x10] + ([6] if int(acq.bp.acquisition_kind) in (int(K.HERCULES), int(K.UHERCULES)) else []) + [1]
    seen = set()
    for mode in modes:
        lib.beamformer_hip_set_das_path(mode)
        try:
            gpu = bflib.beamform(acq.bp, acq.rf, acq.filters)
        finally:
            lib.beamformer_hip_set_das_path(0)
        t = last_timings(bflib)
        if (int(t.das_path), mode & 0x10) in seen and mode != 6:
            continue
        seen.add((int(t.das_path), mode & 0x10))
        PLANE_DRAWS.append((seed, int(t.das_path), int(t.das_row_end_planes)))
        compare(gpu, ref, acq, flags)


def test_random_view_planes_reach_the_plane_kernels():
    """the draws above are worth their name only if they run the kernels they aim at"""
    if len(PLANE_DRAWS) < 30:
        pytest.skip("needs the draws of this module in the same session")
    paths = {p for _, p, _ in PLANE_DRAWS}
    assert int(P.DasPath.Hercules) in paths and int(P.DasPath.Factored) in paths, sorted(PLANE_DRAWS)


# ---- row ends (csrc/das_exact.h).  sample_rf's range test is a step: round 3's fast kernels formed the index as a rounded receive term plus
# a rounded transmit term and kept or dropped a term within an ulp of the end of an RF row differently from the oracle -- one whole tap of
# difference at a voxel.  These are the draws of round 3's out-of-sample fuzz (tools/auto_fuzz.py 72 600, tools/tile_fuzz.py) that failed
# for it, fixed here as cases: every kernel that can take the draw, against the oracle.
ROW_END_SEPARABLE = [96, 107, 112, 114, 120, 125, 130, 142, 160, 194, 201, 237, 241, 254, 259, 261, 268, 305, 318, 319, 343, 346, 361, 367, 385,
                     398, 434, 439, 480, 495, 547, 584, 593]


@pytest.mark.parametrize("seed", ROW_END_SEPARABLE)
def test_row_end_draws_of_the_separable_generator(seed, bflib, oracle, hooks):
    """automatic path, the general kernel, the gather kernel (never staged), the LDS-staged kernel wherever its window holds (every term
    range-checked) and the factored kernel (block staging on request): the oracle's frame from each"""
    acq = draw_separable(seed)
    ref, pairs, flags = reference(oracle, acq)
    lib = bflib.library()
    ran = {}
    for mode in (0, 1, 2, 3, 0x14, 0x114):
        if mode == 3:
            hooks.set("STAGED_CHECKED")
        lib.beamformer_hip_set_das_path(mode)
        try:
            gpu = bflib.beamform(acq.bp, acq.rf, acq.filters)
            t = last_timings(bflib)
            ran[mode] = (int(t.das_path), int(t.das_row_end_planes))
            assert int(t.staged_window_violations) == 0
            if mode in (0x14, 0x114) and int(t.das_row_end_planes):
                # the planes the row-end rule takes from the block-staged kernel run the factored kernel asked for
                d = bflib.describe_das(acq.bp, acq.filters)[4]
                assert int(d.row_end_planes) == int(t.das_row_end_planes) and int(d.row_end_path) == int(P.DasPath.Factored), (mode, int(d.row_end_path))
        finally:
            lib.beamformer_hip_set_das_path(0)
            if mode == 3:
                hooks.clear("STAGED_CHECKED")
        compare(gpu, ref, acq, flags)
    assert ran[1][0] == 0, ran


@pytest.mark.parametrize("seed", [540, 11, 63, 131, 207])
def test_row_end_draws_of_the_tile_generator(seed, bflib, oracle):
    """540: the draw on which das_tile.hip's window-relative position arithmetic flipped ALONE in round 3; block staging asked for, the
    factored kernel and the general kernel: the oracle's frame from each"""
    acq = draw_tile(seed)
    ref, pairs, flags = reference(oracle, acq)
    ok = ~np.isnan(ref)
    if not ok.any() or np.max(np.abs(ref[ok])) == 0:
        pytest.skip("empty image")
    lib = bflib.library()
    for mode in (0x110, 0x210, 0x11):
        lib.beamformer_hip_set_das_path(mode)
        try:
            gpu = bflib.beamform(acq.bp, acq.rf, acq.filters)
        finally:
            lib.beamformer_hip_set_das_path(0)
        compare(gpu, ref, acq, flags)
