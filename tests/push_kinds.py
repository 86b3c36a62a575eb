"""The six multi-frame pushes as one table.  csrc/executor.cpp runs a burst, a READI sweep, a READI image, a views push, a burst views
push and a variants push through one function (push_frames / walk_plan), and csrc/lib_api.cpp refuses them through one
(multi_push_ready): what holds for one of them holds for all, and tests/test_gpu_push_contract.py and tests/test_push_contract_host.py
ask it of all, parametrised over KINDS.  A PushKind record says everything those tests need to treat the kinds alike.  A kind is left
out of a rule only by an entry of its `exempt`, which says why and names the line of the library that makes it so.

A plain module: it imports no test module, and nothing while it is imported that needs a device or the oracle."""
import contextlib
import ctypes as C
import dataclasses
import math

import numpy as np

from ogl_beamforming_amd import lib
from ogl_beamforming_amd import params as P
from tests import cases
from tests import readi_image_cases as R
from tests import variants_cases as vc
from tests.das_push import (case_of, four_views, groups_for, kernel_views, last_timings, noise_frames, patches, per_view_views,
                            sweep_case)

E = P.LibError
I = P.InterpolationMode
FAIL_DAS = P.HIP_DAS_PATH_FAIL_VIEWS_DAS
NO_BURST, NO_VIEWS, PREFER_VIEWS = P.HIP_DAS_PATH_NO_BURST_KERNEL, P.HIP_DAS_PATH_NO_VIEWS_KERNEL, P.HIP_DAS_PATH_PREFER_VIEWS_KERNEL


# ---- the helpers of the kinds' own test modules that these records use

def frame_id(L):
    info = P.HipFrameInfo()
    assert L.beamformer_hip_get_last_frame_info(C.byref(info))
    return info


def last_frame_id(bflib):
    info = P.HipFrameInfo()
    assert bflib.library().beamformer_hip_get_last_frame_info(C.byref(info)), bflib.last_error()
    return int(info.frame_id)


def single_push_of(bflib, acq):
    return bflib.beamform(acq.bp, acq.rf, acq.filters).copy()


def sweep(bflib, acq, rf, groups, expect_kernel=True, device_pointer=None):
    """one sweep; the route the library reports is the one described, and -- on the kernel -- one DAS launch of four frames a thread"""
    n = len(rf)
    described = bflib.describe_readi_sweep(acq.bp, n, groups, acq.filters)
    assert bool(described.burst_kernel) == expect_kernel, described.reason
    frames = bflib.beamform_readi_sweep(acq.bp, rf, groups, acq.filters, on_device_pointer=device_pointer).copy()
    info = bflib.last_burst_info()
    assert info.frame_count == n and bool(info.route.burst_kernel) == expect_kernel, info.route.reason
    assert info.route.das_launches == described.das_launches and info.route.single_path == described.single_path
    assert info.route.min_frames == described.min_frames
    if expect_kernel:
        assert info.route.das_launches == 1 and info.route.frames_per_thread == 4
    else:
        assert info.route.das_launches == n and info.route.frames_per_thread == 1
    frame_info = P.HipFrameInfo()
    assert bflib.library().beamformer_hip_get_last_frame_info(C.byref(frame_info)) and frame_info.frame_id == info.first_frame_id + n - 1
    assert frames.shape[0] == n
    return frames


def group_list(geometry, listed):
    """(group list as the push takes it, frame count)"""
    G = R.GEOMETRIES[geometry][0]
    if listed == "partial":
        return R.PARTIAL12, len(R.PARTIAL12)
    if listed == "no-list":
        return None, G                               # (block.readi_group + k) % G, readi_group 1
    if listed == "one":
        return [G - 1], 1
    return R.PERMUTATIONS[geometry], G


def image(bflib, acq, rf, groups, device_pointer=None):
    """one image push; the route the library reports is the one described.  Returns (frame, info)."""
    n = len(rf)
    G, A = int(acq.bp.readi_group_count), int(acq.bp.acquisition_count)
    described = bflib.describe_readi_image(acq.bp, n, groups, acq.filters)
    frame = bflib.beamform_readi_image(acq.bp, rf, groups, acq.filters, on_device_pointer=device_pointer).copy()
    info = bflib.last_readi_image_info()
    assert info.rf_frame_count == n and info.frame_id == last_frame_id(bflib)
    assert bytes(info.route) == bytes(described), (info.route.reason, described.reason)
    assert info.route.transmit_count == G * A and info.route.decode_launches == 1 and info.route.das_launches == 1
    assert int(last_timings(bflib).das_path) == info.route.das_path
    return frame, info


@contextlib.contextmanager
def two_devices_asked_for(L):
    """the devices of beamformer_hip_set_devices are ordinal 0 twice, none of them initialised: what the several-devices refusal is
    asked under; a single device again on every way out"""
    try:
        L.beamformer_hip_shutdown()          # (where a device is in use, the set of devices is fixed until the library lets go of it)
        assert L.beamformer_hip_set_devices((C.c_int32 * 2)(0, 0), 2)
        yield
    finally:
        L.beamformer_hip_shutdown()
        assert L.beamformer_hip_set_devices((C.c_int32 * 1)(0), 1)


# ---- the records

@dataclasses.dataclass
class Case:
    """the prepared input of one push: the acquisition, the RF as the kind's Python helper takes it (N frames stacked, or the one frame
    of a views or variants push), the kind's extra argument (group list, views, variants), the das path flags the push runs under, the
    output shard (first plane, planes) the shard rules set, and -- a sweep -- whether the sweep kernel takes it"""
    acq: object
    rf: np.ndarray
    extra: object = None
    path: int = 0
    shard: tuple = (0, 1)
    expect_kernel: bool = True


@dataclasses.dataclass(frozen=True)
class Kernels:
    """the kind's own DAS kernel: a pattern of its demangled name for tools/kernel_resources.py, the instantiations the library holds, and
    the figures its removed test asserted on top of "no vector spills, no scratch" """
    pattern: str
    count: int = 12
    max_vgprs: int = None
    no_lds: bool = False
    no_sgpr_spills: bool = False


@dataclasses.dataclass(frozen=True)
class Info:
    """the info struct of the kind's pushes, its getter, and how to read the first id and the number of frames from it"""
    struct: type
    getter: str
    first_id: str
    count: object

    def read(self, L):
        """(first id, frames) of the newest push, or the error kind the getter refuses with"""
        info = self.struct()
        if not getattr(L, self.getter)(C.byref(info)):
            return lib.last_error()[0]
        return int(getattr(info, self.first_id)), int(self.count(info))

    def newest(self, L):
        info = self.struct()
        assert getattr(L, self.getter)(C.byref(info)), lib.last_error()
        return info


@dataclasses.dataclass(frozen=True)
class Route:
    """one route of the kind: its pytest id, the das path flag that asks for it, and what the info of a push that took it says"""
    name: str
    flag: int
    reported: object = lambda info, case: True


@dataclasses.dataclass(frozen=True)
class Row:
    """one malformed push: the arguments of raw() that differ from the case's, the error, a word of the line on stderr; `describe`: the
    kind's describe call refuses the same arguments the same way, `push` False: only that call is asked"""
    overrides: dict
    error: object
    word: str = None
    push: bool = True
    describe: bool = False


@dataclasses.dataclass(frozen=True)
class PushKind:
    name: str                      # the pytest id
    symbols: tuple                 # push, device push, describe, [last info], [resolve_readi_groups]
    kernels: tuple
    info: Info
    routes: tuple
    whole_grid: bool               # an output shard on the block is a refusal (executor.cpp:1500, lib_api.cpp:158), else honoured
    fails_on_flag: bool            # das path flag 0x2000 fails the push at its DAS step (executor.cpp:1814, :1867, :1942)
    max_count: int                 # the largest `count` the ABI takes
    pushed: tuple                  # the push's arguments after the data and its size, by name
    described: tuple               # the describe call's arguments, by name
    description: type              # the struct the describe call fills
    exempt: dict                   # rule -> why the kind is left out of it
    case: object                   # (rule, name=None) -> the Case the removed copy of that rule used for this kind
    helper: object                 # (bflib, case, rf, device_pointer) -> frames: the kind's Python helper with its own assertions
    frames: object                 # case -> F, the frames a push queues
    newest: object                 # (bflib, case, shard_planes=None) -> the frames of the newest push, oldest first, as push() returns them
    malformed: object              # case -> the kind's own Rows
    too_large: object              # () -> (case, arguments of raw() that differ, None or what is asked instead of the refusal) per row
    header: tuple = ()             # what include/ogl_beamformer_hip.h says
    constants: tuple = ()          # (binding's value, expected)
    sizes: tuple = ()              # (ctypes struct, bytes)
    layout: tuple = ()             # (C struct name, ctypes struct, fields whose offsets the C compiler checks)
    device_rf_cases: tuple = (None,)                 # the cases of the device-resident rule, by name
    list_type: type = C.c_uint32   # what the push's list holds
    single_rf: bool = False        # one RF frame a push (views, variants): `count` counts the list
    sharded_route: object = lambda bflib: True       # what the removed shard test asserted of the sharded push's route

    def push(self, bflib, case, rf=None, device_pointer=None):
        """the kind's Python helper; the frames flattened in id order"""
        return self.helper(bflib, case, case.rf if rf is None else rf, device_pointer)

    def arguments(self, order, case, values):
        """the arguments named in `order`: the case's own where `values` has none; a list shorter than its count repeats its first item"""
        v = dict(count=len(case.extra) if self.single_rf else len(case.rf), view_count=len(case.extra or ()), extra=case.extra, tag=0)
        v.update(values)
        v.setdefault("out", C.byref(self.description()))
        items = None if v["extra"] is None else list(v["extra"])
        if items is not None:
            items += items[:1] * ((v["view_count"] if "view_count" in order else v["count"] if self.single_rf else 0) - len(items))
        v["list"] = None if items is None else (self.list_type * len(items))(*items)
        return [v[name] for name in order]

    def raw(self, L, case, data, size, device=False, slot=0, **overrides):
        """the bare ABI call: 0 or 1.  block: another block pushed at `slot`, with one frame of its own RF and no list"""
        if "block" in overrides:
            other = cases.make(overrides.pop("block"))
            assert L.beamformer_push_simple_parameters_at(C.byref(other.bp), slot)
            rf = np.ascontiguousarray(other.rf)
            data, size, overrides = rf.ctypes.data_as(C.c_void_p), rf.nbytes, dict(overrides, count=1, extra=None)
        data = None if overrides.pop("null_data", False) else data
        size += overrides.pop("size_delta", 0)
        return int(bool(getattr(L, self.symbols[1 if device else 0])(data, size, *self.arguments(self.pushed, case, dict(overrides, slot=slot)))))

    def describe(self, L, case, slot=0, **overrides):
        """the bare describe call on the same arguments: 0 or 1"""
        return int(bool(getattr(L, self.symbols[2])(*self.arguments(self.described, case, dict(overrides, slot=slot)))))

    def data(self, case):
        """(the RF kept alive, its address, the bytes of one frame)"""
        rf = np.ascontiguousarray(case.rf)
        return rf, rf.ctypes.data_as(C.c_void_p), rf.nbytes // self.rf_frames(case)

    def first_rf(self, case):
        return case.rf if self.single_rf else case.rf[0]

    def rf_frames(self, case):
        return 1 if self.single_rf else len(case.rf)


def _on_block(case, points):
    """the case with its block on a grid of `points`"""
    bp = type(case.acq.bp).from_buffer_copy(case.acq.bp)
    bp.output_points[:len(points)] = list(points)
    return dataclasses.replace(case, acq=dataclasses.replace(case.acq, bp=bp))


BIG_VIEW = lib.view((1024, 1024, 1), (-10e-3, 0, 5e-3), (10e-3, 0, 40e-3))            # 8 MiB of complex voxels


def _wrapping_view():
    """extents whose product wraps 64 bits"""
    v = P.HipView.from_buffer_copy(BIG_VIEW)
    v.output_points[:] = [0x80000000, 0x80000000, 4]
    return v


def _changed(items, ctype, at, **fields):
    """a copy of the list with fields of item `at` set (an indexed field: name_index)"""
    out = [ctype.from_buffer_copy(item) for item in items]
    for field, value in fields.items():
        name, _, index = field.rpartition("_at_")
        if name:
            getattr(out[at], name)[int(index)] = value
        else:
            setattr(out[at], field, value)
    return out


# ---- burst

def _burst_case(which, name=None):
    if which == "device_rf":
        acq = cases.make(name)
        return Case(acq, noise_frames(acq, 5, 4500))
    if which == "shard":
        acq = cases.make("rca_vls_cw")                       # 12 x 10 x 14
        return Case(acq, noise_frames(acq, 3, 4650), shard=(4, 6))
    acq = cases.make("config1_small")
    if which in ("malformed", "devices"):
        return Case(acq, np.ascontiguousarray(np.stack([acq.rf] * 3)))
    return Case(acq, noise_frames(acq, 5, {"refusals": 4700, "graphs": 4700, "newest_info": 5400}[which]))


def _newest_frames(bflib, case, shard_planes=None):
    return list(bflib.get_last_frames(case.acq.bp, len(case.rf), shard_planes=shard_planes))


def _a_thousand_frames_of(case, points):
    """1024 x 1024 complex voxels are 8 MiB a frame: 1024 of them are twice the default 4 GiB ring (one of them fits)"""
    case = _on_block(case, points)
    return [(dataclasses.replace(case, rf=np.zeros((1024,) + case.acq.rf.shape, case.acq.rf.dtype)), {}, None)]


NO_FLAG = ("no software failure flag reaches the DAS step of a burst, a READI sweep or a READI image push -- their Push records leave "
           "fails_on_flag false (executor.cpp:752) and walk_plan asks it before it fails a push (executor.cpp:981) --: a tombstone here "
           "would need a device fault")
NO_LIST_NEEDED = "the push takes no list (a burst) or takes NULL for \"the block's group onwards\" (lib_api.cpp:206): NULL is no refusal"
TAG_7 = [Row(dict(tag=7), E.InvalidImagePlane)]

BURST = PushKind(
    name="burst",
    symbols=("beamformer_hip_push_data_burst_with_compute", "beamformer_hip_push_device_data_burst_with_compute",
             "beamformer_hip_describe_burst", "beamformer_hip_get_last_burst_info"),
    kernels=(Kernels("das_burst_kernel", 12, max_vgprs=128),),          # 256-thread blocks: 4 waves per SIMD at least
    info=Info(P.HipBurstInfo, "beamformer_hip_get_last_burst_info", "first_frame_id", lambda i: i.frame_count),
    routes=(Route("kernel", 0), Route("per-frame", NO_BURST)),
    whole_grid=False, fails_on_flag=False, max_count=P.HIP_MAX_BURST_FRAMES,
    pushed=("count", "tag", "slot"), described=("slot", "count", "out"), description=P.HipBurstDescription,
    header=("#define BEAMFORMER_HIP_MAX_BURST_FRAMES",), constants=((P.HIP_MAX_BURST_FRAMES >= 256, True),),
    # the structs the binding mirrors: 6 words + the reason; the description + 3 words + 24 kinds + 24 times + the total
    sizes=((P.HipBurstDescription, 24 + 160), (P.HipBurstInfo, 184 + 12 + 4 * 24 + 4 * 24 + 4)),
    exempt={"tombstones": NO_FLAG, "null_list": NO_LIST_NEEDED},
    device_rf_cases=("config1_small", "rca_shuffled_padded", "forces"),
    case=_burst_case,
    helper=lambda bflib, case, rf, at: list(bflib.beamform_burst(case.acq.bp, rf, case.acq.filters, on_device_pointer=at).copy()),
    frames=lambda case: len(case.rf), newest=_newest_frames, malformed=lambda case: TAG_7,
    too_large=lambda: _a_thousand_frames_of(_burst_case("malformed"), (1024, 1024, 1, 1)))


# ---- READI sweep

def _sweep_case(which, name=None):
    if which in ("malformed", "devices"):
        acq = cases.make("readi")                     # G = 4
        return Case(acq, np.ascontiguousarray(np.broadcast_to(acq.rf, (5,) + acq.rf.shape)))
    if which == "newest_info":
        # the block of the image's case: the sweep kernel takes its four frames where four reach its threshold
        acq = R.image_case("g4a4", I.Linear, "real")
        return Case(acq, noise_frames(acq, 4, 6700), None, expect_kernel=4 >= int(lib.describe_readi_sweep(acq.bp, 4, None, acq.filters).min_frames))
    geometry, interp, iq, cw, seed, groups, shard = {
        "device_rf": ("g8a2", I.Cubic, True, True, 5500, [5, 0, 7, 7, 2], (0, 1)),
        "shard": ("g8a2", I.Linear, True, False, 5700, [6, 1, 1, 4, 3], (9, 13)),          # 32 x 1 x 32
        "refusals": ("g4a4", I.Cubic, False, False, 5800, [2, 0, 3, 3, 1], (0, 1)),
        "graphs": ("g4a4", I.Cubic, False, False, 5800, [2, 0, 3, 3, 1], (0, 1))}[which]
    acq = sweep_case(geometry, interp, iq, cw)
    return Case(acq, noise_frames(acq, 5, seed), groups_for(acq, groups), shard=shard)


READI_SWEEP = PushKind(
    name="readi_sweep",
    symbols=("beamformer_hip_push_data_readi_sweep_with_compute", "beamformer_hip_push_device_data_readi_sweep_with_compute",
             "beamformer_hip_describe_readi_sweep", "beamformer_hip_get_last_burst_info", "beamformer_hip_resolve_readi_groups"),
    kernels=(Kernels("das_readi_burst_kernel", 12),),
    # a sweep is served by the burst's info call
    info=Info(P.HipBurstInfo, "beamformer_hip_get_last_burst_info", "first_frame_id", lambda i: i.frame_count),
    routes=(Route("kernel", 0), Route("per-frame", NO_BURST)),
    whole_grid=False, fails_on_flag=False, max_count=P.HIP_MAX_BURST_FRAMES,
    pushed=("count", "list", "tag", "slot"), described=("slot", "list", "count", "out"), description=P.HipBurstDescription,
    exempt={"tombstones": NO_FLAG, "null_list": NO_LIST_NEEDED},
    case=_sweep_case,
    helper=lambda bflib, case, rf, at: list(sweep(bflib, case.acq, rf, case.extra, expect_kernel=case.expect_kernel, device_pointer=at)),
    frames=lambda case: len(case.rf), newest=_newest_frames, malformed=lambda case: TAG_7,
    # (2048 x 1024 voxels: at least 8 MiB a frame)
    too_large=lambda: _a_thousand_frames_of(_sweep_case("malformed"), (2048, 1, 1024)),
    sharded_route=lambda bflib: bflib.last_burst_info().route.burst_kernel == 1)


# ---- READI image

def _image_case(which, name=None):
    if which in ("malformed", "devices"):
        acq = R.image_case("g4a4", I.Linear, "real")
        return Case(acq, np.ascontiguousarray(np.broadcast_to(acq.rf, (2,) + acq.rf.shape)))
    if which in ("newest_info", "refusals"):
        acq = R.image_case("g4a4", I.Linear, "real")
        return Case(acq, noise_frames(acq, 4, 6700) if which == "newest_info" else noise_frames(acq, 5, 7200)[:4], None)
    geometry, interp, kind, cw, seed, shard = {
        "device_rf": ("g8a2", I.Cubic, "iq", True, 6900, (0, 1)),
        "shard": ("g8a2", I.Linear, "iq", False, 6800, (9, 13)),              # 32 x 1 x 32
        "graphs": ("g4a4", I.Cubic, "real", False, 7100, (0, 1))}[which]
    acq = R.image_case(geometry, interp, kind, cw)
    groups = R.PERMUTATIONS[geometry]
    return Case(acq, noise_frames(acq, len(groups), seed), groups, shard=shard)


def _image_malformed(case):
    """the refusals of the image's own tests: the counts and a group out of range, a block that is not READI (a Flash block in a second
    slot), a wrong size, no data, a tag out of range"""
    return [Row(dict(count=0), E.BufferOverflow), Row(dict(count=1025), E.BufferOverflow),
            Row(dict(count=5, extra=[0, 1, 2, 3, 4]), E.InvalidComputeStage),
            Row(dict(block="config1_small", slot=1), E.InvalidAccess, "FORCES / UFORCES block with readi_group_count > 1"),
            Row(dict(size_delta=-4), E.DataSizeMismatch), Row(dict(null_data=True), E.BufferOverflow), Row(dict(tag=99), E.InvalidImagePlane)]


READI_IMAGE = PushKind(
    name="readi_image",
    symbols=("beamformer_hip_push_data_readi_image_with_compute", "beamformer_hip_push_device_data_readi_image_with_compute",
             "beamformer_hip_describe_readi_image", "beamformer_hip_get_last_readi_image_info"),
    kernels=(),
    info=Info(P.HipReadiImageInfo, "beamformer_hip_get_last_readi_image_info", "frame_id", lambda i: 1),
    routes=(Route("derived block", 0),),
    whole_grid=False, fails_on_flag=False, max_count=P.HIP_MAX_BURST_FRAMES,
    pushed=("count", "list", "tag", "slot"), described=("slot", "list", "count", "out"), description=P.HipReadiImageDescription,
    sizes=((P.HipReadiImageDescription, 20 + 160), (P.HipReadiImageInfo, 180 + 12 + 4 * 24 + 4 * 24 + 4)),
    exempt={"tombstones": NO_FLAG, "null_list": NO_LIST_NEEDED,
            "too_large": "the run of an image push is ONE frame of the block's grid, and a block whose frame does not fit the ring is "
                         "refused when its parameters are pushed (lib_api.cpp:67): no image push gets as far as lib_api.cpp:139 with one",
            "kernels": "an image push has no DAS kernel of its own: its one frame is the derived FORCES block's single-frame launch "
                       "(executor.cpp:1675 push_readi_image)"},
    case=_image_case, helper=lambda bflib, case, rf, at: [image(bflib, case.acq, rf, case.extra, device_pointer=at)[0]],
    frames=lambda case: 1,
    newest=lambda bflib, case, shard_planes=None: [bflib.get_last_frame(case.acq.bp, shard_planes=shard_planes).copy()],
    malformed=_image_malformed, too_large=lambda: [],
    sharded_route=lambda bflib: bflib.last_readi_image_info().route.das_launches == 1)


# ---- views

def _views_case(which, name=None):
    if which in ("malformed", "devices"):
        acq = cases.make("config1_small")
        return Case(acq, acq.rf, patches(3))
    if which == "newest_info":
        acq = cases.make("config1_small")
        views = kernel_views(acq)[:3]          # 1 x 1 x 1, 5 x 1 x 7, 33 x 1 x 17
        assert all(int(np.prod(list(v.output_points))) <= 33 * 17 for v in views)
        return Case(acq, noise_frames(acq, 5, 5400)[0], views)
    # the inputs of tests/das_push.py prepared(): the case, one noise frame of seed 5000, the kernel tests' views or the per-view ones
    case_name, which_views, path, shard = {"device_rf": (name, "kernel" if name == "config1_small" else "per_view", PREFER_VIEWS, (0, 1)),
                                           "refusals": ("rca_vls_cw", "per_view", 0, (4, 6)), "graphs": ("rca_vls_cw", "per_view", 0, (4, 6)),
                                           "tombstones": ("rca_cubic_real", "kernel", 0, (0, 1))}[which]
    acq = case_of(case_name)
    return Case(acq, noise_frames(acq, 1, 5000)[0], kernel_views(acq) if which_views == "kernel" else per_view_views(acq), path, shard)


def _bad_views(case, axis):
    """per view: the tag, and the extents"""
    return [Row(dict(extra=_changed(case.extra, P.HipView, 2, image_plane_tag=7)), E.InvalidImagePlane),
            Row(dict(extra=_changed(case.extra, P.HipView, 1, **{f"output_points_at_{axis}": 0})), E.InvalidAccess, describe=True)]


def _views_too_large():
    """1024 x 1024 complex voxels are 8 MiB a view: 1024 of them are twice the default 4 GiB ring (one of them fits); and extents
    whose product wraps 64 bits"""
    case = _views_case("malformed")
    return [(dataclasses.replace(case, extra=[BIG_VIEW] * 1024), {}, None), (dataclasses.replace(case, extra=[_wrapping_view()]), {}, None)]


VIEWS = PushKind(
    name="views",
    symbols=("beamformer_hip_push_data_views_with_compute", "beamformer_hip_push_device_data_views_with_compute",
             "beamformer_hip_describe_views", "beamformer_hip_get_last_views_info"),
    kernels=(Kernels("das_views_kernel", 12, max_vgprs=128, no_lds=True),),
    info=Info(P.HipViewsInfo, "beamformer_hip_get_last_views_info", "first_frame_id", lambda i: i.view_count),
    routes=(Route("views kernel", PREFER_VIEWS, lambda info, case: info.route.kernel_views == len(case.extra)),
            Route("per-view route", NO_VIEWS, lambda info, case: info.route.kernel_views == 0)),
    whole_grid=True, fails_on_flag=True, max_count=P.HIP_MAX_VIEWS,
    pushed=("list", "count", "slot"), described=("slot", "list", "count", "out"), description=P.HipViewsDescription,
    header=("#define BEAMFORMER_HIP_MAX_VIEWS", "BeamformerHipDasPath_NoViewsKernel    = 0x800", "BeamformerHipDasPath_PreferViewsKernel = 0x1000",
            "BeamformerHipDasPath_FailViewsDas     = 0x2000"),
    constants=((P.HIP_MAX_VIEWS, 1024), (P.HIP_DAS_PATH_FAIL_VIEWS_DAS, 0x2000)),
    # the structs the binding mirrors: 16 floats + 3 extents + the tag; 3 words + 1024 paths + the reason; the description + 3 words
    # + 24 kinds + 24 times + the total + the host time
    sizes=((P.HipView, 64 + 12 + 4), (P.HipViewsDescription, 12 + 1024 + 160), (P.HipViewsInfo, 1196 + 12 + 4 * 24 + 4 * 24 + 4 + 4)),
    exempt={}, device_rf_cases=("config1_small", "forces"), list_type=P.HipView, single_rf=True,
    case=_views_case,
    helper=lambda bflib, case, rf, at: bflib.beamform_views(case.acq.bp, rf, case.extra, case.acq.filters, on_device_pointer=at),
    frames=lambda case: len(case.extra), newest=lambda bflib, case, shard_planes=None: bflib.get_last_views(case.extra),
    malformed=lambda case: _bad_views(case, 1), too_large=_views_too_large)


# ---- burst views

def _burst_views_case(which, name=None):
    if which in ("malformed", "devices", "too_large"):
        n = {"malformed": 3, "devices": 2, "too_large": 4}[which]
        acq = cases.make("config1_small")
        return Case(acq, np.ascontiguousarray(np.stack([acq.rf] * n)), patches(min(n, 3)))
    # the inputs of tests/test_gpu_burst_views.py prepared(): the case, five noise frames of seed 6000, four of the kernel tests' views
    acq = case_of("rca_cubic_real" if which == "tombstones" else "config1_small")
    return Case(acq, noise_frames(acq, 5, 6000), four_views(acq))


def _burst_views_helper(bflib, case, rf, device_pointer):
    frames = bflib.beamform_burst_views(case.acq.bp, rf, case.extra, case.acq.filters, on_device_pointer=device_pointer)
    return [frame for row in frames for frame in row]


def _burst_views_malformed(case):
    """the counts and their product, then the list, then the description's address"""
    return [Row(dict(view_count=0), E.BufferOverflow), Row(dict(view_count=P.HIP_MAX_VIEWS + 1), E.BufferOverflow),
            Row(dict(count=17, view_count=241), E.BufferOverflow, describe=True),            # 17 x 241 = 4097 frames
            Row(dict(count=0), E.BufferOverflow, push=False, describe=True),
            *_bad_views(case, 2), Row(dict(out=None), E.InvalidAccess, push=False, describe=True)]


def _4096_small_frames_are_described(case):
    """the most frames a push may queue, 4 x 1024 single voxels"""
    voxel = lib.view((1, 1, 1), (0, 0, 10e-3), (0, 0, 10e-3))
    d = lib.describe_burst_views(case.acq.bp, 4, [voxel] * 1024, case.acq.filters)
    assert d.rung == 2 and d.frame_kernel_views == 1024 and d.das_launches == 4, d.reason


def _burst_views_too_large():
    """1024 x 1024 complex voxels are 8 MiB a frame: 4 RF frames on 256 such views are twice the default 4 GiB ring (4 x 128 fit) -- the
    small views in front of the large ones do not hide them --; extents whose product wraps 64 bits; and the most frames a push may
    queue, which are not refused"""
    case = _burst_views_case("too_large")
    return [(dataclasses.replace(case, extra=[BIG_VIEW] * 256), {}, None),
            (dataclasses.replace(case, extra=patches(1) * 64 + [BIG_VIEW] * 192), {}, None),
            (dataclasses.replace(case, extra=[_wrapping_view()]), {}, None), (case, {}, _4096_small_frames_are_described)]


def _rung(rung):
    return lambda info, case: (info.route.rung, info.frame_count, info.view_count) == (rung, len(case.rf), len(case.extra))


BURST_VIEWS = PushKind(
    name="burst_views",
    symbols=("beamformer_hip_push_data_burst_views_with_compute", "beamformer_hip_push_device_data_burst_views_with_compute",
             "beamformer_hip_describe_burst_views", "beamformer_hip_get_last_burst_views_info"),
    kernels=(Kernels("das_burst_views_kernel", 12, max_vgprs=128, no_lds=True, no_sgpr_spills=True),),
    info=Info(P.HipBurstViewsInfo, "beamformer_hip_get_last_burst_views_info", "first_frame_id", lambda i: i.frame_count * i.view_count),
    routes=(Route("rung1", 0, _rung(1)), Route("rung2", NO_BURST, _rung(2)), Route("rung3", NO_VIEWS, _rung(3))),
    whole_grid=True, fails_on_flag=True, max_count=P.HIP_MAX_BURST_FRAMES,
    pushed=("count", "list", "view_count", "slot"), described=("slot", "count", "list", "view_count", "out"),
    description=P.HipBurstViewsDescription,
    # 7 words + 1024 paths + the reason; the description + 4 words + 24 kinds + 24 times + the total + the host time
    sizes=((P.HipBurstViewsDescription, 28 + 1024 + 160), (P.HipBurstViewsInfo, 1212 + 16 + 4 * 24 + 4 * 24 + 4 + 4)),
    layout=(("BeamformerHipBurstViewsDescription", P.HipBurstViewsDescription, ("path", "reason")),
            ("BeamformerHipBurstViewsInfo", P.HipBurstViewsInfo, ("view_count", "stage_ms", "decide_us"))),
    exempt={}, list_type=P.HipView,
    case=_burst_views_case, helper=_burst_views_helper, frames=lambda case: len(case.rf) * len(case.extra),
    newest=lambda bflib, case, shard_planes=None: bflib.get_last_views([v for v in case.extra for _ in range(len(case.rf))]),
    malformed=_burst_views_malformed, too_large=_burst_views_too_large)


# ---- variants

def _variants_case(which, name=None):
    interp, iq, cw = {"device_rf": ("linear", True, True), "tombstones": ("cubic", False, False), "newest_info": ("cubic", False, False)}.get(
        which, ("linear", True, False))
    acq = vc.block(interp, iq, cw)
    return Case(acq, np.ascontiguousarray(acq.rf), vc.candidates(acq.bp), shard=(4, 6) if which in ("refusals", "graphs") else (0, 1))


def _variants_malformed(case):
    """the description's counts; a tag out of range; a field that is not finite, a speed of sound that is not above zero: InvalidAccess,
    with a line on stderr"""
    good, V = case.extra, P.HipDasVariant
    rows = [Row(dict(count=P.HIP_MAX_VARIANTS + 1), E.BufferOverflow, push=False, describe=True),
            Row(dict(count=0), E.BufferOverflow, push=False, describe=True), Row(dict(tag=7), E.InvalidImagePlane)]
    for field, value in (("speed_of_sound", math.nan), ("speed_of_sound", math.inf), ("speed_of_sound", 0.0), ("speed_of_sound", -1540.0),
                         ("time_offset", math.nan), ("time_offset", -math.inf), ("f_number", math.nan), ("f_number", math.inf)):
        rows.append(Row(dict(extra=_changed(good, V, 2, **{field: value})), E.InvalidAccess, "variant 2", describe=True))
    return rows + [Row(dict(extra=_changed(good, V, 1, speed_of_sound=math.nan)), E.InvalidAccess, "variant 1")]


def _variants_too_large():
    """4096 x 4096 complex voxels are 128 MiB a frame: one fits the default 4 GiB ring, 64 of them are twice its size"""
    case = _on_block(_variants_case("malformed"), (4096, 1, 4096))
    return [(dataclasses.replace(case, extra=[lib.variant_of(case.acq.bp)] * 64), {}, None)]


VARIANTS = PushKind(
    name="variants",
    symbols=("beamformer_hip_push_data_variants_with_compute", "beamformer_hip_push_device_data_variants_with_compute",
             "beamformer_hip_describe_variants", "beamformer_hip_get_last_variants_info"),
    kernels=(Kernels("das_variants_kernel", 12, max_vgprs=128, no_lds=True),),
    info=Info(P.HipVariantsInfo, "beamformer_hip_get_last_variants_info", "first_frame_id", lambda i: i.variant_count),
    routes=(Route("variants kernel", vc.PREFER, lambda info, case: info.route.kernel_variants == len(case.extra)),
            Route("per-variant route", vc.NO_KERNEL, lambda info, case: info.route.kernel_variants == 0)),
    whole_grid=True, fails_on_flag=True, max_count=P.HIP_MAX_VARIANTS,
    pushed=("list", "count", "tag", "slot"), described=("slot", "list", "count", "out"), description=P.HipVariantsDescription,
    header=("#define BEAMFORMER_HIP_MAX_VARIANTS 64u", "BeamformerHipDasPath_NoVariantsKernel = 0x4000",
            "BeamformerHipDasPath_PreferVariantsKernel = 0x8000"),
    constants=((P.HIP_MAX_VARIANTS, 64), (vc.NO_KERNEL, 0x4000), (vc.PREFER, 0x8000)),
    # the structs the binding mirrors: three floats; 6 words + 64 paths + 64 flags + the reason; the description + 3 words + 24 kinds
    # + 24 times + the total + the host time
    sizes=((P.HipDasVariant, 12), (P.HipVariantsDescription, 24 + 64 + 64 + 160), (P.HipVariantsInfo, 312 + 12 + 4 * 24 + 4 * 24 + 4 + 4)),
    exempt={}, list_type=P.HipDasVariant, single_rf=True,
    case=_variants_case,
    helper=lambda bflib, case, rf, at: list(bflib.beamform_variants(case.acq.bp, rf, case.extra, case.acq.filters, on_device_pointer=at).copy()),
    frames=lambda case: len(case.extra),
    newest=lambda bflib, case, shard_planes=None: list(bflib.get_last_frames(case.acq.bp, len(case.extra), shard_planes=shard_planes)),
    malformed=_variants_malformed, too_large=_variants_too_large)


KINDS = (BURST, READI_SWEEP, READI_IMAGE, VIEWS, BURST_VIEWS, VARIANTS)
IDS = [kind.name for kind in KINDS]
