"""Burst views pushes (beamformer_hip_push_data_burst_views_with_compute) on the CPU: beamformer_hip_describe_burst_views (no device
needed) names the rung of the ladder the rules of csrc/das_select.cpp (decide_burst_views) give.  What a burst views push shares with
every other multi-frame push -- its symbols, its kernel's instantiations, its refusals -- is asked of all kinds in
tests/test_push_contract_host.py."""
import pytest

from ogl_beamforming_amd import lib
from ogl_beamforming_amd import params as P
from tests import cases
from tests.das_push import mixed_views, patches
from tests.scaffold import automatic_path_on_the_host  # noqa: F401

NO_BURST, NO_VIEWS = P.HIP_DAS_PATH_NO_BURST_KERNEL, P.HIP_DAS_PATH_NO_VIEWS_KERNEL
GENERAL = int(P.DasPath.General)


def test_the_ladder_on_four_patches_of_config_1():
    acq = cases.make("config1_small")
    L = lib.library()
    views = patches(4)
    # rung 1: all four in ONE launch, whatever their tile count (four tiles here; PreferViewsKernel is not needed)
    d = lib.describe_burst_views(acq.bp, 5, views, acq.filters)
    assert d.min_frames == 5
    assert (d.rung, d.kernel_views, d.frame_kernel_views, d.das_launches, d.frames_per_thread) == (1, 4, 0, 1, 4), d.reason
    assert list(d.path[:4]) == [GENERAL] * 4 and d.stage_launches == 1 and d.reason
    one = lib.describe_burst_views(acq.bp, 5, views[:1], acq.filters)          # one tile: below kViewsMinTiles, still taken
    assert (one.rung, one.kernel_views, one.das_launches) == (1, 1, 1), one.reason
    # rung 2: below the threshold, and under 0x400 -- the views kernel once per RF frame
    d = lib.describe_burst_views(acq.bp, 4, views, acq.filters)
    assert (d.rung, d.kernel_views, d.frame_kernel_views, d.das_launches, d.frames_per_thread) == (2, 0, 4, 4, 1), d.reason
    assert "fewer than 5 frames" in d.reason.decode()
    L.beamformer_hip_set_das_path(NO_BURST)
    d = lib.describe_burst_views(acq.bp, 5, views, acq.filters)
    assert (d.rung, d.kernel_views, d.frame_kernel_views, d.das_launches) == (2, 0, 4, 5) and "0x400" in d.reason.decode()
    # ... under decide_views' unchanged rules: one patch is fewer tiles than kViewsMinTiles and runs per view
    d = lib.describe_burst_views(acq.bp, 5, views[:1], acq.filters)
    assert (d.rung, d.frame_kernel_views, d.das_launches) == (3, 0, 5) and "fewer than" in d.reason.decode()
    # rung 3: under 0x800 every (view, RF frame) its own launch
    for mode in (NO_VIEWS, NO_VIEWS | NO_BURST):
        L.beamformer_hip_set_das_path(mode)
        d = lib.describe_burst_views(acq.bp, 5, views, acq.filters)
        assert (d.rung, d.kernel_views, d.frame_kernel_views, d.das_launches) == (3, 0, 0, 20) and "0x800" in d.reason.decode()
        assert list(d.path[:4]) == [GENERAL] * 4
    # one RF frame goes through the same code
    L.beamformer_hip_set_das_path(0)
    d = lib.describe_burst_views(acq.bp, 1, views, acq.filters)
    assert (d.rung, d.frame_kernel_views, d.das_launches) == (2, 4, 1), d.reason


def test_a_mixed_list_is_one_fused_launch_plus_n_times_the_others():
    acq = cases.make("rca_flash_none_tx")
    d = lib.describe_burst_views(acq.bp, 5, mixed_views(acq), acq.filters)
    assert list(d.path[:4]) == [GENERAL, int(P.DasPath.Gather), GENERAL, int(P.DasPath.Gather)]
    assert (d.rung, d.kernel_views, d.das_launches) == (1, 2, 1 + 5 * 2), d.reason
    reason = d.reason.decode()
    assert "2 of 4 views" in reason and "once per RF frame" in reason and "10" in reason


@pytest.mark.parametrize("name,word", [("forces", "family"), ("hercules_wide_cw", "family"), ("rca_staged_auto", "row-end rule")])
def test_other_families_and_faster_kernels_run_on_rung_3_and_say_why(name, word):
    """(rca_staged_auto's own grid: the LDS-staged kernel, cut in two by the row-end rule -- tests/test_views_host.py)"""
    acq = cases.make(name)
    single = lib.describe_das(acq.bp, acq.filters)
    own = lib.describe_views(acq.bp, [lib.view_of(acq.bp)], acq.filters)
    d = lib.describe_burst_views(acq.bp, 5, [lib.view_of(acq.bp)] * 2, acq.filters)
    assert (d.rung, d.kernel_views, d.frame_kernel_views) == (3, 0, 0), d.reason
    assert d.das_launches == 5 * 2 * own.das_launches and d.path[0] == d.path[1] == single[0]
    assert word in d.reason.decode() and "per RF frame" in d.reason.decode(), d.reason
