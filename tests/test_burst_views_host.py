"""Burst views pushes (beamformer_hip_push_data_burst_views_with_compute) on the CPU: the four entry points exist and are bound, the
fused kernel is in the library with its twelve instantiations, beamformer_hip_describe_burst_views (no device needed) names the rung of
the ladder the rules of csrc/das_select.cpp (decide_burst_views) give, and a malformed push is refused before any device is touched."""
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
SYMBOLS = ("beamformer_hip_push_data_burst_views_with_compute", "beamformer_hip_push_device_data_burst_views_with_compute",
           "beamformer_hip_describe_burst_views", "beamformer_hip_get_last_burst_views_info")
NO_BURST, NO_VIEWS = P.HIP_DAS_PATH_NO_BURST_KERNEL, P.HIP_DAS_PATH_NO_VIEWS_KERNEL
GENERAL = int(P.DasPath.General)


@pytest.fixture(autouse=True)
def automatic_path():
    lib.library().beamformer_hip_set_das_path(0)
    yield
    lib.library().beamformer_hip_set_das_path(0)


def test_the_four_symbols_are_declared_exported_and_bound(tmp_path):
    header = open(os.path.join(ROOT, "include", "ogl_beamformer_hip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", lib.LIBRARY_PATH], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in nm.stdout.splitlines() if " T " in line}
    for name in SYMBOLS:
        assert f"{name}(" in header, name
        assert name in exported, name
        assert name in lib.exported_symbols(), name
    # 7 words + 1024 paths + the reason; the description + 4 words + 24 kinds + 24 times + the total + the host time
    assert C.sizeof(P.HipBurstViewsDescription) == 28 + 1024 + 160
    assert C.sizeof(P.HipBurstViewsInfo) == 1212 + 16 + 4 * 24 + 4 * 24 + 4 + 4
    # ... and the header's own sizes and offsets, by the C compiler
    source = tmp_path / "sizes.c"
    d, i = P.HipBurstViewsDescription, P.HipBurstViewsInfo
    source.write_text(
        '#include <stddef.h>\n#include "ogl_beamformer_hip.h"\n'
        f"_Static_assert(sizeof(BeamformerHipBurstViewsDescription) == {C.sizeof(d)}, \"description\");\n"
        f"_Static_assert(offsetof(BeamformerHipBurstViewsDescription, path) == {d.path.offset}, \"path\");\n"
        f"_Static_assert(offsetof(BeamformerHipBurstViewsDescription, reason) == {d.reason.offset}, \"reason\");\n"
        f"_Static_assert(sizeof(BeamformerHipBurstViewsInfo) == {C.sizeof(i)}, \"info\");\n"
        f"_Static_assert(offsetof(BeamformerHipBurstViewsInfo, view_count) == {i.view_count.offset}, \"view_count\");\n"
        f"_Static_assert(offsetof(BeamformerHipBurstViewsInfo, stage_ms) == {i.stage_ms.offset}, \"stage_ms\");\n"
        f"_Static_assert(offsetof(BeamformerHipBurstViewsInfo, decide_us) == {i.decide_us.offset}, \"decide_us\");\n")
    run = subprocess.run(["cc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(source)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="needs the ROCm LLVM binutils")
def test_the_fused_kernel_has_twelve_instantiations_without_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    kernels = [k for k in kernel_resources.kernels_of(lib.LIBRARY_PATH) if "das_burst_views_kernel" in k["demangled"]]
    assert len({k["demangled"] for k in kernels}) == 12, sorted(k["demangled"] for k in kernels)
    for k in kernels:
        assert not k["vgpr_spill_count"] and not k["sgpr_spill_count"] and not k["private_segment_fixed_size"], k["demangled"]
        assert k["vgpr_count"] <= 128, (k["demangled"], k["vgpr_count"])
        assert not k["group_segment_fixed_size"], k["demangled"]                 # no LDS


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


def test_malformed_pushes_are_refused_before_a_device_is_touched():
    acq = cases.make("config1_small")
    L = push_parameters(acq)
    n = 3
    rf = np.ascontiguousarray(np.stack([acq.rf] * n))
    ptr, size = rf.ctypes.data_as(C.c_void_p), rf[0].nbytes
    views = (P.HipView * 3)(*patches(3))
    push = L.beamformer_hip_push_data_burst_views_with_compute
    describe = L.beamformer_hip_describe_burst_views
    out = P.HipBurstViewsDescription()
    # the counts and their product
    assert not push(ptr, size, 0, views, 3, 0) and lib.last_error()[0] == E.BufferOverflow
    assert not push(ptr, size, P.HIP_MAX_BURST_FRAMES + 1, views, 3, 0) and lib.last_error()[0] == E.BufferOverflow
    assert not push(ptr, size, n, views, 0, 0) and lib.last_error()[0] == E.BufferOverflow
    many = (P.HipView * (P.HIP_MAX_VIEWS + 1))(*([patches(1)[0]] * (P.HIP_MAX_VIEWS + 1)))
    assert not push(ptr, size, n, many, P.HIP_MAX_VIEWS + 1, 0) and lib.last_error()[0] == E.BufferOverflow
    assert not push(ptr, size, 17, many, 241, 0) and lib.last_error()[0] == E.BufferOverflow            # 17 x 241 = 4097 frames
    assert not describe(0, 17, many, 241, C.byref(out)) and lib.last_error()[0] == E.BufferOverflow
    assert not describe(0, 0, views, 3, C.byref(out)) and lib.last_error()[0] == E.BufferOverflow
    # the list
    assert not push(ptr, size, n, None, 3, 0) and lib.last_error()[0] == E.InvalidAccess
    bad = (P.HipView * 3)(*patches(3))
    bad[2].image_plane_tag = 7
    assert not push(ptr, size, n, bad, 3, 0) and lib.last_error()[0] == E.InvalidImagePlane
    bad[2].image_plane_tag = 0
    bad[1].output_points[2] = 0
    assert not push(ptr, size, n, bad, 3, 0) and lib.last_error()[0] == E.InvalidAccess
    assert not describe(0, n, bad, 3, C.byref(out)) and lib.last_error()[0] == E.InvalidAccess
    assert not describe(0, n, views, 3, None) and lib.last_error()[0] == E.InvalidAccess
    # the single push's checks, per frame, with its error kinds
    assert not push(ptr, size - 2, n, views, 3, 0) and lib.last_error()[0] == E.DataSizeMismatch
    assert not push(ptr, size + 2, n, views, 3, 0) and lib.last_error()[0] == E.DataSizeMismatch
    assert not push(ptr, size, n, views, 3, 5) and lib.last_error()[0] == E.ParameterBlockUnallocated
    assert not push(None, size, n, views, 3, 0) and lib.last_error()[0] == E.BufferOverflow
    assert not L.beamformer_hip_push_device_data_burst_views_with_compute(ptr, size - 2, n, views, 3, 0) and lib.last_error()[0] == E.DataSizeMismatch
    # an output shard on the block
    try:
        assert L.beamformer_hip_set_output_shard(0, 0, 1)
        assert not push(ptr, size, n, views, 3, 0) and lib.last_error()[0] == E.InvalidAccess
    finally:
        assert L.beamformer_hip_set_output_shard(0, 0, 0)


def test_several_devices_are_refused(capfd):
    acq = cases.make("config1_small")
    L = push_parameters(acq)
    rf = np.ascontiguousarray(np.stack([acq.rf] * 2))
    views = (P.HipView * 2)(*patches(2))
    try:
        assert L.beamformer_hip_set_devices((C.c_int32 * 2)(0, 0), 2)
        capfd.readouterr()
        assert not L.beamformer_hip_push_data_burst_views_with_compute(rf.ctypes.data_as(C.c_void_p), rf[0].nbytes, 2, views, 2, 0)
        assert lib.last_error()[0] == E.InvalidAccess and "one device" in capfd.readouterr().err
    finally:
        assert L.beamformer_hip_set_devices((C.c_int32 * 1)(0), 1)


def test_a_run_larger_than_the_frame_ring_is_refused_whole_and_4096_small_frames_are_not():
    """1024 x 1024 complex voxels are 8 MiB a frame: 4 RF frames on 256 such views are twice the default 4 GiB ring (4 x 128 fit);
    extents whose product wraps 64 bits; and the most frames a push may queue, 4 x 1024 single voxels, are described"""
    acq = cases.make("config1_small")
    L = push_parameters(acq)
    rf = np.ascontiguousarray(np.stack([acq.rf] * 4))
    ptr, size = rf.ctypes.data_as(C.c_void_p), rf[0].nbytes
    big = lib.view((1024, 1024, 1), (-10e-3, 0, 5e-3), (10e-3, 0, 40e-3))
    views = (P.HipView * 256)(*([big] * 256))
    assert not L.beamformer_hip_push_data_burst_views_with_compute(ptr, size, 4, views, 256, 0)
    assert lib.last_error()[0] == E.FrameSizeOverflow
    # (the small views in front of the large ones do not hide them)
    mixed = (P.HipView * 256)(*(patches(1) * 64 + [big] * 192))
    assert not L.beamformer_hip_push_data_burst_views_with_compute(ptr, size, 4, mixed, 256, 0)
    assert lib.last_error()[0] == E.FrameSizeOverflow
    wrap = (P.HipView * 1)(big)
    wrap[0].output_points[:] = [0x80000000, 0x80000000, 4]
    assert not L.beamformer_hip_push_data_burst_views_with_compute(ptr, size, 4, wrap, 1, 0)
    assert lib.last_error()[0] == E.FrameSizeOverflow
    voxel = lib.view((1, 1, 1), (0, 0, 10e-3), (0, 0, 10e-3))
    d = lib.describe_burst_views(acq.bp, 4, [voxel] * 1024, acq.filters)
    assert d.rung == 2 and d.frame_kernel_views == 1024 and d.das_launches == 4, d.reason
