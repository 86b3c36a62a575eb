"""The ingest matrix of tests/ingest_cases.py on the device, bit for bit: every upload route of csrc/executor.cpp's decide_upload,
every lane width of ingest_copy_kernel under a non-identity mapping, all three instantiations of ingest_a1s2_kernel with real and
complex kinds, both kernels' grid-stride loops past their first trip, A1S2 results that wrap, overflow, round at a tie or are
subnormal -- and the fences between the routes where pushes of different routes meet in one of the three RF slots.

Every case is {Decode (None), DAS}: the DAS input (beamformer_hip_copy_das_input) is the ingested RF through at most an exact
conversion.  Bars: bit identity everywhere -- against the oracle's capture, against tests/ingest_cases.py's own numpy reference, between
a host push and a device-resident push, between a burst's frame and a single push, between a frame of a sequence and that frame
pushed alone --; the one exception is the frame against the oracle, tests/parity.py's compare() at tests/cases.py's tolerance().
tests/test_ingest_host.py holds what the matrix must cover, judged without a device."""
import ctypes as C

import numpy as np
import pytest

from ogl_beamforming_amd import params as P
from tests import ingest_cases as IC
from tests.das_push import compare, last_timings
from tests.stage_checks import as_bits, check_das_input, oracle_run, push

pytestmark = pytest.mark.gpu

R = P.UploadRoute
LOG = []                      # (test, case, what the library described for the push that ran)
_REFERENCE = {}
OFFSETS = (0, 2, 4, 8)


def reference(oracle, name):
    """(frame, nearest flags, DAS input) of the oracle, computed once per case and left unchanged"""
    if name not in _REFERENCE:
        ref, flags, ref_in = oracle_run(oracle, IC.make(name))
        ref.setflags(write=False)
        ref_in.setflags(write=False)
        _REFERENCE[name] = (ref, flags, ref_in)
    return _REFERENCE[name]


def note(test, name, d, extra=""):
    kernel = ("none", f"ingest_copy_kernel, {d.copy_bytes} bytes per lane", f"ingest_a1s2_kernel<{('int16_t', 'float', '_Float16')[d.a1s2_base]}>")[d.ingest_kernel]
    LOG.append(f"{test:<10} {name:<28} {d.name.decode():<20} {kernel}{extra}")


def device_info(bflib):
    info = P.HipDeviceInfo()
    assert bflib.library().beamformer_hip_get_device_info(0, C.byref(info)), bflib.last_error()
    return info


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(as_bits(a), as_bits(b))


# ------------------------------------------------------------------------------------------------ every case, host push

@pytest.mark.parametrize("name", sorted(IC.CASES))
def test_host_push(name, bflib, oracle, hooks):
    c, acq = IC.CASES[name], IC.make(name)
    ref, flags, ref_in = reference(oracle, name)
    mapped = IC.mapped_rf(acq)
    d = bflib.describe_upload(acq.bp, acq.rf.nbytes)
    assert (R(d.route), d.ingest_kernel, d.copy_bytes) == (c.route, c.kernel, c.width), d.name
    gpu, gpu_in = push(bflib, acq, hooks, poison=True)
    note("host", name, d)
    verdict, _ = check_das_input(bflib, oracle, acq, gpu_in, ref_in, name)
    assert verdict == "bit-identical", "a stage between the RF and DAS is not exact: the case does not pin the ingest"
    assert same_bits(gpu_in, IC.das_input_of(acq, mapped)), "the DAS input is not the numpy reference of the mapped RF"
    info = device_info(bflib)
    assert info.rf_bytes == mapped.nbytes
    assert info.rf_checksum == IC.rf_checksum(mapped), "the RF slot's checksum is not the numpy reference's"
    if c.group != "planted":            # (their DAS input holds +-inf: only it and the checksum are judged)
        compare(gpu, ref, acq, flags)


# ------------------------------------------------------------------------------------------------ device-resident pushes

DEVICE_CASES = IC.SMALL + ["big_shuffled_padded"]


@pytest.mark.parametrize("name", DEVICE_CASES)
def test_device_push_at_every_alignment(name, bflib, hooks):
    """the same RF from a caller's device buffer, at 0, 2, 4 and 8 bytes into a larger allocation: the lane width follows the pointer,
    the bits do not change"""
    import torch
    c, acq = IC.CASES[name], IC.make(name)
    L = bflib.library()
    host, host_in = push(bflib, acq, hooks, poison=True)
    host = host.copy()
    host_sum = device_info(bflib).rf_checksum
    nbytes = acq.rf.nbytes
    raw = torch.from_numpy(acq.rf.view(np.uint8).reshape(-1).copy())
    buffer = torch.empty(nbytes + 64, dtype=torch.uint8, device="cuda")
    assert buffer.data_ptr() % 16 == 0
    widths = []
    for offset in OFFSETS:
        buffer.fill_(0xFF)
        view = buffer[offset: offset + nbytes]
        view.copy_(raw)
        torch.cuda.synchronize()
        d = bflib.describe_upload(acq.bp, nbytes, device_pointer=view.data_ptr())
        assert R(d.route) == c.device_route, d.name
        assert L.beamformer_hip_push_device_data_with_compute(C.c_void_p(view.data_ptr()), nbytes, 0, 0), bflib.last_error()
        frame = bflib.get_last_frame(acq.bp)
        das_in = bflib.das_input(acq.bp)
        note("device", name, d, f"  (+{offset})")
        assert same_bits(das_in, host_in), f"offset {offset}: the DAS input differs from the host push's"
        assert same_bits(frame, host), f"offset {offset}: the frame differs from the host push's"
        info = device_info(bflib)
        if info.rf_bytes:
            assert info.rf_checksum == host_sum, offset
        else:
            assert R(d.route) == R.DeviceBorrowed, "only a borrowed buffer reports no checksum"
        assert (R(d.route) == R.DeviceBorrowed) == (info.rf_bytes == 0)
        widths.append(int(d.copy_bytes))
    if c.kernel == 1 and c.device_route == R.DeviceIngest:
        assert widths == [c.width, 2, min(4, c.width), min(4, c.width)], widths


def test_device_cases_reach_every_device_route(bflib):
    reached = {R(bflib.describe_upload(IC.make(n).bp, IC.make(n).rf.nbytes, device_pointer=1 << 40).route) for n in DEVICE_CASES}
    assert reached == {R.DeviceBorrowed, R.DeviceCopy, R.DeviceIngest}


# ------------------------------------------------------------------------------------------------ bursts

@pytest.mark.parametrize("name", IC.SMALL + ["burst_2MiB"])
def test_burst_frames_are_single_pushes(name, bflib, hooks):
    """every frame's DAS input of a burst (one upload, one ingest launch with a frame dimension) is that frame's RF pushed alone"""
    big = name == "burst_2MiB"
    acq = IC.burst_case() if big else IC.make(name)
    n = 5 if big else 3
    frames = IC.burst_frames(acq, n)
    hooks.set("SCRATCH_POISON")
    singles = []
    for k in range(n):
        bflib.beamform(acq.bp, frames[k])
        singles.append(bflib.das_input(acq.bp))
    d = bflib.describe_upload(acq.bp, acq.rf.nbytes, n)
    assert R(d.route) == (R.CopyEngineStaged if big else R.PinnedInPlace) and d.ingest_kernel == (2 if acq.bp.contrast_mode else 1)
    bflib.beamform_burst(acq.bp, frames)
    note("burst", name, d, f"  ({n} frames)")
    for k in range(n):
        assert same_bits(bflib.das_input(acq.bp, frame=k), singles[k]), f"frame {k} of the burst"
    assert not same_bits(singles[0], singles[1]), "the burst's frames do not differ: nothing would show a mixed-up frame"


# ------------------------------------------------------------------------------------------------ routes meeting in the RF slots

MEETING = ("Int16_w2_pad37", "big_direct", "big_shuffled_padded")      # pinned-in-place (on the device: device-ingest), direct, staged
WALK = (0, 0, 1, 1, 2, 2, 0, 2, 1, 0)                                  # ten symbols whose nine transitions are the nine ordered pairs
PUSHES = 30


def kind_of(n):
    """the case of push n: RF slot n % 3 sees pushes n % 3, n % 3 + 3, ... -- WALK under a relabelling of its own"""
    return (WALK[n // 3] + n % 3) % 3


def scale_of(n):
    """... and its factor: every case meets every factor, and no two consecutive pushes of one RF slot are the same case at the same factor"""
    return (1, 2, 4)[(n + n // 3) % 3]


def test_the_walk_puts_every_ordered_pair_into_every_rf_slot():
    for slot in range(3):
        seen = [kind_of(n) for n in range(slot, PUSHES, 3)]
        assert {(a, b) for a, b in zip(seen, seen[1:])} == {(a, b) for a in range(3) for b in range(3)}
    assert {scale_of(n) for n in range(PUSHES)} == {1, 2, 4}
    assert {(kind_of(n), scale_of(n)) for n in range(PUSHES)} == {(k, s) for k in range(3) for s in (1, 2, 4)}
    assert all((kind_of(n), scale_of(n)) != (kind_of(n + 3), scale_of(n + 3)) for n in range(PUSHES - 3))


HEAVY_GRID = (1024, 1, 1024)


@pytest.mark.parametrize("mode", ["host", "host_buffer_overwritten", "device_small", "compute_bound"])
def test_routes_meeting_in_the_rf_slots(mode, bflib):
    """30 pushes of three parameter blocks with no read in between: a small push (read in place, or device-resident), a direct
    copy-engine push and a staged one follow each other in every order in every RF slot, so every fence of enqueue_upload /
    finish_upload between two routes is the only thing that keeps a slot's RF, raw staging and pinned memory intact.
    On 256 voxels a frame's kernels take less time than its 8.5 MiB copy, so the compute stream waits for the copy stream and a copy
    never finds the slot's last reader still running; compute_bound beamforms the same RF on 1024 x 1024 voxels (1.1e9 terms a
    large frame: its DAS time is printed beside the push), where the copy stream runs ahead of the kernels and only the `consumed`
    fence holds a slot's next copy back."""
    import torch
    L = bflib.library()
    L.beamformer_set_global_timeout(0xFFFFFFFF)
    bflib.set_hook("SCRATCH_POISON", None)
    acqs = [IC.make(n, HEAVY_GRID) if mode == "compute_bound" else IC.make(n) for n in MEETING]
    for acq in acqs:
        assert acq.rf.dtype == np.int16 and np.abs(acq.rf).max() < 8000      # x4 stays an int16, and exact in every stage
    alone = []
    for acq in acqs:
        L.beamformer_hip_shutdown()
        alone.append(bflib.beamform(acq.bp, acq.rf).copy())
        assert np.abs(alone[-1]).max() > 0
    assert L.beamformer_reserve_parameter_blocks(3)
    try:
        for slot, acq in enumerate(acqs):
            assert L.beamformer_push_simple_parameters_at(C.byref(acq.bp), slot), bflib.last_error()
        scaled = [{s: np.ascontiguousarray(acq.rf * np.int16(s)) for s in (1, 2, 4)} for acq in acqs]
        on_device = {}
        if mode == "device_small":
            on_device = {s: torch.from_numpy(scaled[0][s].view(np.uint8).reshape(-1).copy()).cuda() for s in (1, 2, 4)}
            torch.cuda.synchronize()
        staging = [np.empty_like(acq.rf) for acq in acqs]

        def push_one(kind, scale):
            rf = scaled[kind][scale]
            if kind == 0 and on_device:
                return L.beamformer_hip_push_device_data_with_compute(C.c_void_p(on_device[scale].data_ptr()), rf.nbytes, 0, kind)
            if mode == "host_buffer_overwritten":          # the caller may reuse its buffer as soon as the push returns
                staging[kind][...] = rf
                ok = L.beamformer_push_data_with_compute(staging[kind].ctypes.data_as(C.c_void_p), rf.nbytes, 0, kind)
                staging[kind].view(np.uint8)[...] = 0xFF
                return ok
            return L.beamformer_push_data_with_compute(rf.ctypes.data_as(C.c_void_p), rf.nbytes, 0, kind)

        # every block's plan is committed by a push of its own first: no push of the sequence replans (a replan drains the stream)
        for kind in range(3):
            assert push_one(kind, 1), bflib.last_error()
        assert L.beamformer_hip_synchronize()
        for n in range(PUSHES):
            assert push_one(kind_of(n), scale_of(n)), (n, bflib.last_error())
        frames = bflib.get_last_frames(acqs[0].bp, PUSHES)
        t = last_timings(bflib)                            # (the newest push's DAS stage: printed, not judged)
        das_ms = sum(t.stage_ms[i] for i in range(t.stage_count) if t.stage_kind[i] == int(P.ShaderKind.DAS))
        wrong = [n for n in range(PUSHES) if not same_bits(frames[n], alone[kind_of(n)] * np.float32(scale_of(n)))]
        assert not wrong, (f"pushes {wrong} (case, scale: {[(MEETING[kind_of(n)], scale_of(n)) for n in wrong]}) are not their scale times "
                           "the frame of their case pushed alone")
    finally:
        assert L.beamformer_reserve_parameter_blocks(1)
    routes = [bflib.describe_upload(acq.bp, acq.rf.nbytes, device_pointer=(1 << 40) if (k == 0 and mode == "device_small") else None)
              for k, acq in enumerate(acqs)]
    assert [R(d.route) for d in routes] == [R.DeviceIngest if mode == "device_small" else R.PinnedInPlace, R.CopyEngineDirect, R.CopyEngineStaged]
    for d, name in zip(routes, MEETING):
        note("meeting", name, d, f"  ({mode}: 30 pushes, every ordered pair of routes in every RF slot; the last push's DAS took {das_ms:.3f} ms)")


# ------------------------------------------------------------------------------------------------ the record

def test_log_of_what_ran():
    """prints what the tests above pushed: per case the route, the ingest kernel and its lane width or scalar type"""
    print()
    for line in LOG:
        print("ingest:", line)
