"""Views pushes (beamformer_hip_push_data_views_with_compute) on the CPU: beamformer_hip_describe_views (no device needed) names the
route the rules of csrc/das_select.cpp give.  What a views push shares with every other multi-frame push -- its symbols, its kernel's
instantiations, its refusals -- is asked of all kinds in tests/test_push_contract_host.py."""
from ogl_beamforming_amd import lib
from ogl_beamforming_amd import params as P
from tests import cases
from tests.das_push import mixed_views, patches
from tests.scaffold import automatic_path_on_the_host  # noqa: F401

PREFER, NO_KERNEL = P.HIP_DAS_PATH_PREFER_VIEWS_KERNEL, P.HIP_DAS_PATH_NO_VIEWS_KERNEL


def test_small_patches_take_the_views_kernel_in_one_launch():
    acq = cases.make("config1_small")
    L = lib.library()
    views = patches(16)
    L.beamformer_hip_set_das_path(PREFER)
    d = lib.describe_views(acq.bp, views, acq.filters)
    assert d.kernel_views == 16 and d.das_launches == 1, d.reason
    assert list(d.path[:16]) == [int(P.DasPath.General)] * 16 and d.min_tiles >= 1 and d.reason
    # the flag: every view on its own launch, and the reason names it; it changes nothing about single frames
    L.beamformer_hip_set_das_path(NO_KERNEL)
    d = lib.describe_views(acq.bp, views, acq.filters)
    assert d.kernel_views == 0 and d.das_launches == 16 and "0x800" in d.reason.decode()
    assert list(d.path[:16]) == [int(P.DasPath.General)] * 16
    assert lib.describe_das(acq.bp, acq.filters)[0] == int(P.DasPath.General)


def test_fewer_tiles_than_the_threshold_run_per_view():
    acq = cases.make("config1_small")
    d = lib.describe_views(acq.bp, patches(1), acq.filters)
    tiles = d.min_tiles                                                  # a 16 x 1 x 16 patch is one 256-voxel tile
    # (a threshold of one tile would leave no push below it: this branch of decide_views and its wording would then need another test)
    assert tiles >= 2, "kViewsMinTiles == 1: no views push is below the threshold any more"
    below = lib.describe_views(acq.bp, patches(tiles - 1), acq.filters)
    assert below.kernel_views == 0 and below.das_launches == tiles - 1 and "fewer than" in below.reason.decode()
    at = lib.describe_views(acq.bp, patches(tiles), acq.filters)
    assert at.kernel_views == tiles and at.das_launches == 1, at.reason
    lib.library().beamformer_hip_set_das_path(PREFER)
    assert lib.describe_views(acq.bp, patches(1), acq.filters).kernel_views == 1


def test_other_families_and_faster_kernels_run_per_view_and_say_why():
    acq = cases.make("forces")
    views = [lib.view_of(acq.bp), lib.view((7, 1, 9), (-1e-3, 0, 8e-3), (1e-3, 0, 10e-3))]
    lib.library().beamformer_hip_set_das_path(PREFER)
    d = lib.describe_views(acq.bp, views, acq.filters)
    assert d.kernel_views == 0 and d.das_launches == 2 and "family" in d.reason.decode()
    assert d.path[0] == lib.describe_das(acq.bp, acq.filters)[0]
    # a view of rca_staged_auto's own grid: that case's own decision (the LDS-staged kernel, cut in two by the row-end rule)
    staged = cases.make("rca_staged_auto")
    single = lib.describe_das(staged.bp, staged.filters)
    d = lib.describe_views(staged.bp, [lib.view_of(staged.bp)], staged.filters)
    assert d.kernel_views == 0 and d.path[0] == single[0] == int(P.DasPath.Staged) and d.das_launches == 2, d.reason


def test_a_mixed_list_is_one_launch_plus_the_others():
    acq = cases.make("rca_flash_none_tx")
    lib.library().beamformer_hip_set_das_path(PREFER)
    d = lib.describe_views(acq.bp, mixed_views(acq), acq.filters)
    assert list(d.path[:4]) == [int(P.DasPath.General), int(P.DasPath.Gather), int(P.DasPath.General), int(P.DasPath.Gather)]
    assert d.kernel_views == 2 and d.das_launches == 1 + 2, d.reason
