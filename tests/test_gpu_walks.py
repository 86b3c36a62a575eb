"""Every copy of the DAS block-to-tile map at its regime edges, on the device: the entries of tests/walk_cases.py (what each is
there for: that module; that the planner really gives it that regime: tests/test_walks_host.py) pushed through the C ABI with the
SCRATCH_POISON hook set -- the ring slot holds NaN before the frame, so a tile no block wrote keeps its NaN and fails compare()'s
NaN-position check, and a tile written from another tile's position fails its bars.  No tolerance of its own: the bars are
tests/parity.py compare()'s at cases.tolerance = 1e-4.

An entry is pushed once with the poison and once without (the same bits); its checks share those frames and each has its own test
id.  Slab entries push the whole frame and the slab, both poisoned; burst entries one burst of kBurstMinFrames noise frames."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

from tests import walk_cases as W
from tests.das_push import compare, last_timings, same_bits
from tests.parity import reference

pytestmark = pytest.mark.gpu

NAMES = [e.name for e in W.ENTRIES]
SLABS = [e.name for e in W.ENTRIES if e.slab]
BURSTS = [e.name for e in W.ENTRIES if e.burst]
CHECKED = [e.name for e in W.ENTRIES if e.checked]


# one module-scoped parameter per entry: pytest then runs an entry's checks one after the other, and they share its frames
@pytest.fixture(scope="module", params=NAMES)
def entry(request):
    return W.BY_NAME[request.param]


@pytest.fixture(scope="module", params=SLABS)
def slab_entry(request):
    return W.BY_NAME[request.param]


@dataclasses.dataclass
class Pushed:
    frame: np.ndarray          # under SCRATCH_POISON
    again: np.ndarray          # pushed again without it
    path: int
    violations: int


def push(bflib, entry, acq, poison, slab=None):
    """one push of the acquisition under the entry's mode and hooks: (frame, das path, staged window violations)"""
    L = bflib.library()
    for name, value in entry.hooks:
        bflib.set_hook(name, value)
    if poison:
        bflib.set_hook("SCRATCH_POISON", "1")
    rf = np.ascontiguousarray(acq.rf)
    try:
        assert L.beamformer_push_simple_parameters(C.byref(acq.bp)), bflib.last_error()
        L.beamformer_hip_set_das_path(entry.mode)
        assert L.beamformer_hip_set_output_shard(0, *(slab or (0, 0))), bflib.last_error()
        L.beamformer_set_global_timeout(0xFFFFFFFF)
        assert L.beamformer_push_data_with_compute(rf.ctypes.data_as(C.c_void_p), rf.nbytes, 0, 0), bflib.last_error()
        frame = bflib.get_last_frame(acq.bp, shard_planes=slab[1] if slab else None).copy()
        t = last_timings(bflib)
        return frame, int(t.das_path), int(t.staged_window_violations)
    finally:
        L.beamformer_hip_set_output_shard(0, 0, 0)
        L.beamformer_hip_set_das_path(0)
        bflib.set_hook("SCRATCH_POISON", None)
        for name, _ in entry.hooks:
            bflib.set_hook(name, None)


@functools.lru_cache(maxsize=2)
def whole_frame(whole):
    """(acquisition, oracle frame, its flags, the library's whole frame under the poison and without) of an entry without its slab:
    entries that differ only in the slab share it"""
    from ogl_beamforming_amd import lib as bflib
    from oracle import binding as oracle
    acq = whole.make()
    ref, _, flags = reference(oracle, acq)
    frame, path, violations = push(bflib, whole, acq, poison=True)
    again, path_again, _ = push(bflib, whole, acq, poison=False)
    assert path_again == path
    return acq, ref, flags, Pushed(frame, again, path, violations)


@functools.lru_cache(maxsize=2)
def slab_frame(entry):
    from ogl_beamforming_amd import lib as bflib
    acq = whole_frame(entry.whole)[0]
    frame, path, violations = push(bflib, entry, acq, poison=True, slab=entry.slab)
    again, _, _ = push(bflib, entry, acq, poison=False, slab=entry.slab)
    return Pushed(frame, again, path, violations)


def test_the_frame_reports_the_entrys_das_path(entry):
    assert whole_frame(entry.whole)[3].path == entry.path
    if entry.slab:
        assert slab_frame(entry).path == entry.path


def test_poisoned_frame_against_the_oracle(entry):
    """a tile that was never written keeps the poison's NaN; a tile written from another position is off by the frame's own scale"""
    name = entry.name
    acq, ref, flags, pushed = whole_frame(entry.whole)
    verdict = compare(pushed.frame, ref, acq, flags, path=pushed.path, label=f"walks/{name}")
    print(f"{name}: max_rel_err {verdict.max_rel_err:.3e} ({verdict.bar} bar)")


def test_pushed_again_without_the_poison_bit_identical(entry):
    pushed = whole_frame(entry.whole)[3]
    assert same_bits(pushed.frame, pushed.again)
    if entry.slab:
        part = slab_frame(entry)
        assert same_bits(part.frame, part.again)


def test_poisoned_slab_is_the_whole_frames_planes(slab_entry):
    """the slab frame, pushed poisoned as well, bit for bit the same planes of the oracle-checked whole frame"""
    entry, name = slab_entry, slab_entry.name
    acq, ref, flags, pushed = whole_frame(entry.whole)
    compare(pushed.frame, ref, acq, flags, path=pushed.path, label=f"walks/{name}/whole")
    first, count = entry.slab
    part = slab_frame(entry)
    assert part.frame.shape[0] == count and not np.isnan(part.frame).any()
    assert same_bits(part.frame, np.ascontiguousarray(pushed.frame[first: first + count]))


@pytest.mark.parametrize("name", CHECKED)
def test_no_term_leaves_its_staged_window(name):
    """STAGED_CHECKED on one entry of each staged kernel: every term range-checked, violations counted"""
    entry = W.BY_NAME[name]
    assert entry.checked and ("STAGED_CHECKED", "1") in entry.hooks
    assert whole_frame(entry.whole)[3].violations == 0
    if entry.slab:
        assert slab_frame(entry).violations == 0


@pytest.mark.parametrize("name", BURSTS)
def test_burst_kernel_walks_the_same_tiles(name, bflib, oracle, hooks):
    """das_burst.hip calls general_tile itself: a burst of kBurstMinFrames noise frames of the general-kernel entry, poisoned, every frame
    against the oracle's frame of its RF"""
    entry = W.BY_NAME[name]
    acq = entry.make()
    L = bflib.library()
    rf = np.random.default_rng(entry.seed).normal(0, 1.0, (W.BURST_FRAMES,) + acq.rf.shape).astype(acq.rf.dtype)
    hooks.set("SCRATCH_POISON")
    L.beamformer_hip_set_das_path(entry.mode)
    try:
        described = bflib.describe_burst(acq.bp, W.BURST_FRAMES, acq.filters)
        assert described.burst_kernel, described.reason
        frames = bflib.beamform_burst(acq.bp, rf, acq.filters).copy()
        info = bflib.last_burst_info()
        assert info.frame_count == W.BURST_FRAMES and info.route.burst_kernel, info.route.reason
    finally:
        L.beamformer_hip_set_das_path(0)
    for k in range(W.BURST_FRAMES):
        acq_k = dataclasses.replace(acq, rf=rf[k])
        ref, _, flags = reference(oracle, acq_k)
        compare(frames[k], ref, acq_k, flags, label=f"walks/{name}/burst/{k}")
