"""Views pushes (beamformer_hip_push_data_views_with_compute) on the CPU: the four entry points exist and are bound, the views kernel
is in the library with its twelve instantiations, beamformer_hip_describe_views (no device needed) names the route the rules of
csrc/das_select.cpp give, and a malformed push is refused before any device is touched."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from ogl_beamforming_amd import lib
from ogl_beamforming_amd import params as P
from tests import cases
from tests.das_push import mixed_views, patches, push_parameters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = P.LibError
VIEWS_SYMBOLS = ("beamformer_hip_push_data_views_with_compute", "beamformer_hip_push_device_data_views_with_compute",
                 "beamformer_hip_describe_views", "beamformer_hip_get_last_views_info")
PREFER, NO_KERNEL = P.HIP_DAS_PATH_PREFER_VIEWS_KERNEL, P.HIP_DAS_PATH_NO_VIEWS_KERNEL


@pytest.fixture(autouse=True)
def automatic_path():
    lib.library().beamformer_hip_set_das_path(0)
    yield
    lib.library().beamformer_hip_set_das_path(0)


def test_the_four_views_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "ogl_beamformer_hip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", lib.LIBRARY_PATH], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in nm.stdout.splitlines() if " T " in line}
    for name in VIEWS_SYMBOLS:
        assert f"{name}(" in header, name
        assert name in exported, name
        assert name in lib.exported_symbols(), name
    assert "#define BEAMFORMER_HIP_MAX_VIEWS" in header and P.HIP_MAX_VIEWS == 1024
    assert "BeamformerHipDasPath_NoViewsKernel    = 0x800" in header and "BeamformerHipDasPath_PreferViewsKernel = 0x1000" in header
    assert "BeamformerHipDasPath_FailViewsDas     = 0x2000" in header and P.HIP_DAS_PATH_FAIL_VIEWS_DAS == 0x2000
    # the structs the binding mirrors: 16 floats + 3 extents + the tag; 3 words + 1024 paths + the reason; the description + 3 words
    # + 24 kinds + 24 times + the total + the host time
    assert C.sizeof(P.HipView) == 64 + 12 + 4
    assert C.sizeof(P.HipViewsDescription) == 12 + 1024 + 160
    assert C.sizeof(P.HipViewsInfo) == 1196 + 12 + 4 * 24 + 4 * 24 + 4 + 4


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="needs the ROCm LLVM binutils")
def test_the_views_kernel_has_twelve_instantiations_without_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    kernels = [k for k in kernel_resources.kernels_of(lib.LIBRARY_PATH) if "das_views_kernel" in k["demangled"]]
    assert len({k["demangled"] for k in kernels}) == 12, sorted(k["demangled"] for k in kernels)
    for k in kernels:
        assert not k["vgpr_spill_count"] and not k["private_segment_fixed_size"], k["demangled"]
        assert k["vgpr_count"] <= 128, (k["demangled"], k["vgpr_count"])
        assert not k["group_segment_fixed_size"], k["demangled"]                 # no LDS


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


def test_malformed_pushes_are_refused_before_a_device_is_touched():
    acq = cases.make("config1_small")
    L = push_parameters(acq)
    rf = np.ascontiguousarray(acq.rf)
    ptr, size = rf.ctypes.data_as(C.c_void_p), rf.nbytes
    views = (P.HipView * 3)(*patches(3))
    push = L.beamformer_hip_push_data_views_with_compute
    assert not push(ptr, size, views, 0, 0) and lib.last_error()[0] == E.BufferOverflow
    many = (P.HipView * (P.HIP_MAX_VIEWS + 1))(*([patches(1)[0]] * (P.HIP_MAX_VIEWS + 1)))
    assert not push(ptr, size, many, P.HIP_MAX_VIEWS + 1, 0) and lib.last_error()[0] == E.BufferOverflow
    assert not push(ptr, size, None, 3, 0) and lib.last_error()[0] == E.InvalidAccess
    # the single push's checks, with its error kinds (lib/ogl_beamformer_lib.c:503-511)
    assert not push(ptr, size - 2, views, 3, 0) and lib.last_error()[0] == E.DataSizeMismatch
    assert not push(ptr, size + 2, views, 3, 0) and lib.last_error()[0] == E.DataSizeMismatch
    assert not push(ptr, size, views, 3, 5) and lib.last_error()[0] == E.ParameterBlockUnallocated
    assert not push(None, size, views, 3, 0) and lib.last_error()[0] == E.BufferOverflow
    assert not L.beamformer_hip_push_device_data_views_with_compute(ptr, size - 2, views, 3, 0) and lib.last_error()[0] == E.DataSizeMismatch
    # per view: the tag and the extents
    bad = (P.HipView * 3)(*patches(3))
    bad[2].image_plane_tag = 7
    assert not push(ptr, size, bad, 3, 0) and lib.last_error()[0] == E.InvalidImagePlane
    bad[2].image_plane_tag = 0
    bad[1].output_points[1] = 0
    assert not push(ptr, size, bad, 3, 0) and lib.last_error()[0] == E.InvalidAccess
    assert not L.beamformer_hip_describe_views(0, bad, 3, C.byref(P.HipViewsDescription())) and lib.last_error()[0] == E.InvalidAccess
    # an output shard on the block
    try:
        assert L.beamformer_hip_set_output_shard(0, 0, 1)
        assert not push(ptr, size, views, 3, 0) and lib.last_error()[0] == E.InvalidAccess
    finally:
        assert L.beamformer_hip_set_output_shard(0, 0, 0)


def test_views_larger_than_the_frame_ring_are_refused_whole():
    """1024 x 1024 complex voxels are 8 MiB a view: 1024 of them are twice the default 4 GiB ring (one of them fits); and extents
    whose product wraps 64 bits"""
    acq = cases.make("config1_small")
    L = push_parameters(acq)
    rf = np.ascontiguousarray(acq.rf)
    big = lib.view((1024, 1024, 1), (-10e-3, 0, 5e-3), (10e-3, 0, 40e-3))
    views = (P.HipView * 1024)(*([big] * 1024))
    assert not L.beamformer_hip_push_data_views_with_compute(rf.ctypes.data_as(C.c_void_p), rf.nbytes, views, 1024, 0)
    assert lib.last_error()[0] == E.FrameSizeOverflow
    wrap = (P.HipView * 1)(big)
    wrap[0].output_points[:] = [0x80000000, 0x80000000, 4]
    assert not L.beamformer_hip_push_data_views_with_compute(rf.ctypes.data_as(C.c_void_p), rf.nbytes, wrap, 1, 0)
    assert lib.last_error()[0] == E.FrameSizeOverflow
