"""What the DAS push tests share: the comparison that names the newest frame's DAS path, single pushes, bursts, views and
sweeps built the way every test module builds them.  A plain module (its asserts run, without pytest's rewritten messages); it imports
tests/cases.py and tests/parity.py and no test module.  The kernel case lists, which ask the library while they are imported, live in
tests/das_kernel_cases.py so that only their users pay for them."""
import ctypes as C
import dataclasses
import functools

import numpy as np

from ogl_beamforming_amd import configs as cfg
from ogl_beamforming_amd import lib
from ogl_beamforming_amd import lib as bf
from ogl_beamforming_amd import params as P
from tests import cases
from tests import parity
from tests.parity import reference


def compare(gpu, ref, acq, flags=None, *, path=None, label=None):
    """tests/parity.py compare(); the log entry names the DAS path of the library's newest frame unless `path` is given"""
    if path is None:
        from ogl_beamforming_amd import lib
        path = last_das_path(lib)
    return parity.compare(gpu, ref, acq, flags, path=path, label=label)


def last_timings(bflib):
    import ctypes as C
    t = P.HipFrameTimings()
    assert bflib.library().beamformer_hip_get_last_frame_timings(C.byref(t))
    return t


def last_das_path(bflib):
    return int(last_timings(bflib).das_path)


def use_devices(lib, ordinals):
    lib.beamformer_hip_shutdown()
    arr = (C.c_int32 * len(ordinals))(*ordinals)
    assert lib.beamformer_hip_set_devices(arr, len(ordinals))
    assert lib.beamformer_hip_get_device_count() == len(ordinals)


I = P.InterpolationMode


def row_end_case(interp):
    """A two-transmit RCA plane of real f32 samples whose 256-sample rows end inside the image (the deepest voxels ask for sample
    290): it takes the burst kernel, and -- found by a scan of the depth range on the CPU -- the float oracle and its double twin
    keep or drop a row-end term differently at one or two of its voxels (parity.py's flip set)."""
    j = {I.Linear: 29, I.Cubic: 68}[interp]
    return cfg.rca(f"burst_row_ends_{interp.name.lower()}", 24, 2, 256, (96, 1, 96), (-3e-3, 0, 5e-3), (3e-3, 0, 9.0e-3 + j * 37e-6),
                   seed=900 + j, interp=interp, demodulate=False, data_kind=P.DataKind.Float32, f_number=1.0, angles=np.array([-6.0, 6.0]))


def noise_frames(acq, n, seed):
    rng = np.random.default_rng(seed)
    shape = (n,) + acq.rf.shape
    if acq.rf.dtype.kind == "i":
        return np.clip(np.rint(rng.normal(0, 1000.0, shape)), -32000, 32000).astype(acq.rf.dtype)
    return rng.normal(0, 1.0, shape).astype(acq.rf.dtype)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def single_push(bflib, acq, rf):
    rf = np.ascontiguousarray(rf)
    assert bflib.library().beamformer_push_data_with_compute(rf.ctypes.data_as(C.c_void_p), rf.nbytes, 0, 0), bflib.last_error()
    return bflib.get_last_frame(acq.bp).copy()


def close_to_single_push(oracle, acq, rf, one, frame, k):
    """a burst's frame `frame` against the single push `one` of the same RF, where another DAS kernel computed it (the burst kernel):
    within the case's tolerance of the frame maximum"""
    assert np.array_equal(np.isnan(one), np.isnan(frame))
    ok = ~np.isnan(one)
    scale = np.abs(one[ok]).max()
    slack = cases.tolerance(acq) * scale
    if acq.bp.interpolation_mode == int(I.Nearest):
        # a tap within float rounding of k + 1/2 may fall either way in either kernel: the oracle's per-voxel budget, once each
        flags = {}
        oracle.beamform(acq.bp, rf, acq.filters, flags=flags)
        slack = slack + 2.02 * flags["budget"][ok]
    err = np.abs(one[ok] - frame[ok])
    assert (err <= slack).all(), f"frame {k}: burst and single push differ by {err.max() / scale:.3e} of the frame maximum"


def check_burst(bflib, oracle, acq, n, seed, expect_kernel, against_single=True):
    """one burst of n noise frames: parity of every frame, pairwise different frames, frame k belongs to RF k, the route the library
    reports, and every frame against the single push of the same RF.  Returns (frames, RF)."""
    L = bflib.library()
    rf = noise_frames(acq, n, seed)
    described = bflib.describe_burst(acq.bp, n, acq.filters)
    assert bool(described.burst_kernel) == expect_kernel, described.reason
    gpu = bflib.beamform_burst(acq.bp, rf, acq.filters).copy()
    info = bflib.last_burst_info()
    assert info.frame_count == n and bool(info.route.burst_kernel) == expect_kernel, info.route.reason
    assert info.route.das_launches == described.das_launches and info.route.single_path == described.single_path
    if expect_kernel:
        assert info.route.das_launches == 1 and info.route.frames_per_thread == 4
    frame_info = P.HipFrameInfo()
    assert L.beamformer_hip_get_last_frame_info(C.byref(frame_info)) and frame_info.frame_id == info.first_frame_id + n - 1
    assert gpu.shape[0] == n
    worst = 0.0
    for k in range(n):
        acq_k = dataclasses.replace(acq, rf=rf[k])
        ref, pairs, flags = reference(oracle, acq_k)
        v = compare(gpu[k], ref, acq_k, flags, label=f"{acq.name}/burst{n}/{k}")
        worst = max(worst, v.max_rel_err)
    print(f"{acq.name}: burst of {n} on the {'burst kernel' if expect_kernel else 'per-frame route'}: worst max_rel_err {worst:.3e}")
    for a in range(n):
        for b in range(a + 1, n):
            assert not np.array_equal(gpu[a], gpu[b], equal_nan=True), (a, b)
    # the order: the same frames permuted come back permuted, bit for bit (a frame's bits do not depend on its slot in the burst)
    perm = np.random.default_rng(seed + 1).permutation(n)
    again = bflib.beamform_burst(acq.bp, rf[perm], acq.filters)
    for i in range(n):
        assert same_bits(again[i], gpu[perm[i]]), f"frame {i} of the permuted burst is not the frame of RF {perm[i]}"
    if against_single:
        identical = 0
        for k in range(n):
            one = single_push(bflib, acq, rf[k])
            close_to_single_push(oracle, acq, rf[k], one, gpu[k], k)
            identical += same_bits(one, gpu[k])
        if expect_kernel:
            print(f"{acq.name}: {identical} of {n} frames of the burst equal their single push bit for bit")
    return gpu, rf


def patches(n, points=(16, 1, 16)):
    """n small patches inside config 1's image (x -19 .. 19 mm of a 64-element array at 0.3 mm pitch; 5 .. 40 mm deep)"""
    return [lib.view(points, (-4e-3 + 0.4e-3 * k, 0, 10e-3 + 0.5e-3 * k), (-3e-3 + 0.4e-3 * k, 0, 11e-3 + 0.5e-3 * k)) for k in range(n)]


def mixed_views(acq):
    """rca_flash_none_tx's block: its own plane runs the general kernel (the views kernel takes it), volumes the gather kernel"""
    volume = lib.view((12, 10, 3), (-2e-3, -2e-3, 8e-3), (2e-3, 2e-3, 9e-3))
    return [lib.view_of(acq.bp), volume, lib.view((5, 1, 7), (-1e-3, 0, 8e-3), (1e-3, 0, 10e-3)), volume]


def push_parameters(acq):
    L = lib.library()
    for s, fp in enumerate(acq.filters):
        assert L.beamformer_create_filter(C.byref(fp), s, 0)
    assert L.beamformer_push_simple_parameters(C.byref(acq.bp)), lib.last_error()
    return L


KERNEL_CASES = ["config1_small", "rca_cubic_real", "rca_f32_complex_in", "rca_a1s2", "rca_nearest_real"]
GENERAL_PATH_FOR = {"rca_nearest_real"}            # see the module docstring
# The instantiations of the views kernels no case above dispatches (every one with coherency weighting, and nearest x IQ): the file's
# small real and IQ cases with the interpolation mode and the weighting set in the parameter block ("case+mode+cw", case_of()), run
# under das path 1 like rca_nearest_real so that the views kernel takes them whatever their single frames would run.
DISPATCH_CASES = ["rca_nearest_real+cw", "rca_f32_complex_in+nearest", "rca_f32_complex_in+nearest+cw", "rca_cubic_real+linear+cw",
                  "rca_f32_complex_in+linear+cw", "rca_cubic_real+cw", "rca_f32_complex_in+cw"]
# the part of the case's depth range its RF rows reach (256-sample rows end a tenth of the way down the 6 .. 18 mm image): the views are
# laid inside it, so that none of them is an empty image -- and their deepest voxels lie at the ends of the rows
REACHED_DEPTH = {"rca_f32_complex_in": 0.1, "rca_a1s2": 0.1, "rca_cubic_real": 0.8, "rca_nearest_real": 0.8}


def box(bp):
    """(lo, hi) of the case's own grid in world coordinates, read off its voxel transform: a volume's three extents, or a view
    plane's x and depth with the lateral extent repeated along y"""
    m = list(bp.das_voxel_transform)
    if m[10] != 0.0:                       # das_transform_3d
        return (m[12], m[13], m[14]), (m[12] + m[0], m[13] + m[5], m[14] + m[10])
    return (m[12], m[12], m[14]), (m[12] + m[0], m[12] + m[0], m[14] + m[6])      # das_transform_2d_xz


def inner(lo, hi, a, b):
    """the part a .. b (fractions of the extent, per axis) of the box lo .. hi"""
    return (tuple(l + (h - l) * f for l, h, f in zip(lo, hi, a)), tuple(l + (h - l) * f for l, h, f in zip(lo, hi, b)))


def case_of(name):
    """cases.make() of the name before the first '+', then 'nearest' / 'linear' / 'cubic' and 'cw' set in its parameter block"""
    base, *changes = name.split("+")
    acq = cases.make(base)
    for change in changes:
        if change == "cw":
            acq.bp.coherency_weighting = 1
        else:
            acq.bp.interpolation_mode = int({"nearest": I.Nearest, "linear": I.Linear, "cubic": I.Cubic}[change])
    return acq


def kernel_views(acq):
    """the view set of the kernel tests: the max(1, n - 1) division, less than a tile, ragged tiles, a volume, a YZ plane, the case's
    own grid, and the second view once more.  Nearest interpolation keeps the views of at least the case's own voxel count (on
    fewer voxels compare()'s share rule for nearest taps allows no outlier at all) and repeats its own grid."""
    lo, hi = box(acq.bp)
    d = REACHED_DEPTH.get(acq.name, 1.0)
    views = [bf.view((1, 1, 1), *inner(lo, hi, (0.5, 0.5, 0.5 * d), (1, 1, d))),
             bf.view((5, 1, 7), *inner(lo, hi, (0.3, 0.5, 0.2 * d), (0.6, 0.5, 0.7 * d))),
             bf.view((33, 1, 17), *inner(lo, hi, (0.1, 0.5, 0.1 * d), (0.9, 0.5, 0.9 * d))),
             bf.view((9, 6, 5), *inner(lo, hi, (0.2, 0.3, 0.3 * d), (0.8, 0.7, 0.8 * d))),
             bf.view((1, 40, 24), *inner(lo, hi, (0.5, 0.1, 0.2 * d), (0.5, 0.9, 1.1 * d))),
             bf.view_of(acq.bp)]
    views.append(views[1])
    if acq.bp.interpolation_mode == int(I.Nearest):
        views = [v for v in views if int(np.prod(list(v.output_points))) >= acq.voxels]
        views.append(bf.view_of(acq.bp))
    return views


def per_view_views(acq):
    lo, hi = box(acq.bp)
    own = [int(n) for n in acq.bp.output_points[:3]]
    part = tuple(max(1, n // 2 + (n > 2)) for n in own)
    return [bf.view_of(acq.bp), bf.view(part, *inner(lo, hi, (0.2, 0.2, 0.3), (0.7, 0.7, 0.8))), bf.view_of(acq.bp)]


def on_grid(acq, view, rf):
    """the acquisition with the view's grid in its parameter block, and `rf`"""
    bp = type(acq.bp).from_buffer_copy(acq.bp)
    bp.das_voxel_transform[:] = list(view.das_voxel_transform)
    bp.output_points[:3] = [int(n) for n in view.output_points]
    return dataclasses.replace(acq, bp=bp, rf=rf)


@functools.lru_cache(maxsize=None)
def prepared(name, which="kernel"):
    """(acquisition, noise RF, views, per view: its acquisition and the oracle's reference) -- computed once, shared, left unchanged"""
    from oracle import binding
    binding.library()
    acq = row_end_case({"row_ends_linear": I.Linear, "row_ends_cubic": I.Cubic}[name]) if name.startswith("row_ends") else case_of(name)
    rf = noise_frames(acq, 1, 4200 if name.startswith("row_ends") else 5000)[0]
    if name.startswith("row_ends"):
        # the whole plane; the deepest 96 x 1 x 12 strip -- which lies wholly past the ends of the 256-sample rows: an image of zeros,
        # compared exactly --; and the 12 rows around the depth at which the rows end (rows r - 8 .. r + 3 of the plane, r its last
        # row with signal), which compare() judges as it judges the plane
        lo, hi = box(acq.bp)
        whole = reference(binding, on_grid(acq, bf.view_of(acq.bp), rf))[0]
        r = int(np.flatnonzero((whole != 0).any(axis=(1, 2)))[-1])
        assert 8 <= r <= 80
        views = [bf.view_of(acq.bp), bf.view((96, 1, 12), *inner(lo, hi, (0, 0, (r - 8) / 95), (1, 1, (r + 3) / 95))),
                 bf.view((96, 1, 12), *inner(lo, hi, (0, 0, 84 / 95), (1, 1, 1)))]
    else:
        views = kernel_views(acq) if which == "kernel" else per_view_views(acq)
    refs = []
    for v in views:
        acq_v = on_grid(acq, v, rf)
        refs.append((acq_v,) + tuple(reference(binding, acq_v)))
    return acq, rf, views, refs


def mode_for(name, flag):
    return flag | (1 if name in GENERAL_PATH_FOR or name in DISPATCH_CASES else 0)


def four_views(acq):
    """of kernel_views: less than a tile (5 x 1 x 7), ragged tiles (33 x 1 x 17), a small volume (9 x 6 x 5)
    and the case's own grid.  Nearest interpolation keeps that helper's own filter (views of at least the case's voxel count), so that
    compare()'s outlier share is met by the reference alone."""
    views = kernel_views(acq)
    if acq.bp.interpolation_mode == int(I.Nearest):
        return views[:4]
    return [views[1], views[2], views[3], views[5]]


S = P.ShaderKind
LO, HI = (-1e-3, 0, 5e-3), (1e-3, 0, 9e-3)          # the `readi` case's extent (tests/cases.py LO3 / HI3)
# (readi_group_count, acquisition_count, voxels): G x A = 16 transmit elements on 16 channels
GEOMETRIES = {"g4a4": (4, 4, (16, 1, 16)), "g2a8": (2, 8, (24, 1, 20)), "g8a2": (8, 2, (32, 1, 32))}
GROUPS5 = [2, 0, 3, 3, 1]                            # not monotone, with a repeat; taken modulo G


def sweep_case(geometry, interp, iq, cw):
    G, A, points = GEOMETRIES[geometry]
    name = f"readi_sweep_{geometry}_{interp.name.lower()}_{'iq' if iq else 'real'}{'_cw' if cw else ''}"
    seed = 3300 + 16 * list(GEOMETRIES).index(geometry) + 4 * int(interp) + 2 * iq + cw
    if iq:       # Int16 through Demodulate: IQ samples
        return cfg.forces(name, 16, A, 512, points, LO, HI, seed=seed, interp=interp, cw=cw, decode=0, readi_groups=G, readi_group=1,
                          stages=(S.Demodulate, S.DAS))
    return cfg.forces(name, 16, A, 512, points, LO, HI, seed=seed, interp=interp, cw=cw, decode=0, readi_groups=G, readi_group=1,
                      data_kind=P.DataKind.Float32)


def groups_for(acq, groups):
    return [g % int(acq.bp.readi_group_count) for g in groups]


def run(bflib, acq):
    frame = bflib.beamform(acq.bp, acq.rf, acq.filters).copy()
    return frame, last_das_path(bflib), last_timings(bflib).staged_window_violations


def lds_bytes(group, chunk, a4):
    """bf_staged_paired_lds_bytes (bf_kernels.h), restated"""
    return (16 * (group * 64 + 3) + 16 * (((chunk + 1) & ~1) << 5) + 4 * (a4 + 2 * (chunk + 2)) + 128 + 15) & ~15


def plan(acq):
    """the plan of the frame with the paired shape asked for (beamformer_hip_describe_das needs no device)"""
    lib = bf.library()
    bf.set_hook("STAGED_SHAPE", "5,5,5")
    lib.beamformer_hip_set_das_path(3)
    try:
        return bf.describe_das(acq.bp, acq.filters)[4]
    finally:
        lib.beamformer_hip_set_das_path(0)
        bf.set_hook("STAGED_SHAPE", None)
