"""What every multi-frame push owes its caller, on the device, asked of all six kinds of tests/push_kinds.py.  csrc/executor.cpp runs
them through one function (push_frames / walk_plan): ids, tombstones, the upload and the record behind beamformer_hip_get_last_*_info
are one text, so each rule is one test, parametrised over the kinds (and over a kind's routes where the rule depends on the route),
with the kind's constants read from its record.  A kind is left out of a rule only through its record's `exempt`.

Parity against the oracle, the ladders and everything else that is about one kind alone are in that kind's own test_gpu_*.py module.
Das path flag 0x2000 is the only failure a test here causes: a refusal on the host, in walk_plan, before any DAS launch."""
import ctypes as C

import numpy as np
import pytest

from ogl_beamforming_amd import params as P
from tests.das_push import same_bits, single_push
from tests.push_kinds import BURST, BURST_VIEWS, FAIL_DAS, IDS, KINDS, VIEWS, frame_id, two_devices_asked_for
from tests.scaffold import automatic_path  # noqa: F401

pytestmark = pytest.mark.gpu
E = P.LibError


@pytest.fixture(autouse=True)
def two_parameter_blocks(automatic_path, bflib):
    """(the READI image's refusals push a block that is not READI in a second slot)"""
    L = bflib.library()
    L.beamformer_reserve_parameter_blocks(2)
    yield
    L.beamformer_reserve_parameter_blocks(1)


def all_same_bits(frames, expected):
    assert len(frames) == len(expected)
    for k, (frame, other) in enumerate(zip(frames, expected)):
        assert same_bits(frame, other), k


FLAGGED = [(kind, route) for kind in KINDS if kind.fails_on_flag for route in kind.routes]


@pytest.mark.parametrize("kind,route", FLAGGED, ids=[f"{kind.name}-{route.name}" for kind, route in FLAGGED])
def test_a_push_that_fails_leaves_a_tombstone_under_every_one_of_its_ids(kind, route, bflib):
    """das path flag 0x2000 fails the push at its DAS stage: its ids are taken, its frames placed, nothing launched there -- what a
    refused launch leaves.  Every reader of "the newest frame" then FAILS instead of serving an older record (or reporting success
    with the caller's buffer unwritten); older good frames stay exportable; the flag touches no single push; the next good push of the
    kind takes the next ids, reports its route and is served whole."""
    L = bflib.library()
    case = kind.case("tombstones")
    acq, F, N = case.acq, kind.frames(case), kind.rf_frames(case)
    rf, data, size = kind.data(case)
    flag = case.path | route.flag
    L.beamformer_hip_set_das_path(flag)
    good = kind.push(bflib, case)
    assert len(good) == F
    newest = frame_id(L).frame_id
    assert kind.info.read(L) == (newest - F + 1, F)
    L.beamformer_hip_set_das_path(flag | FAIL_DAS)
    # the flag fails no single push
    one = kind.first_rf(case)
    assert same_bits(single_push(bflib, acq, one), bflib.beamform(acq.bp, one, acq.filters))
    older = bflib.get_last_frame(acq.bp).copy()
    newest = frame_id(L).frame_id
    assert not kind.raw(L, case, data, size)
    assert bflib.last_error()[0] == E.InvalidAccess
    sentinel = np.full(sum((f.nbytes + 63) // 64 * 64 for f in good) // 4 + older.nbytes // 4 + 64, -7.0, np.float32)
    sptr = sentinel.ctypes.data_as(C.c_void_p)
    for count in sorted({1, N, F}):       # the newest frame is missing: an error, and nothing of the failed push is served
        assert not L.beamformer_get_last_frames(sptr, sentinel.nbytes, count)
        assert bflib.last_error()[0] == E.InvalidAccess and (sentinel == -7.0).all()
    assert not L.beamformer_hip_get_last_frame_info(C.byref(P.HipFrameInfo()))
    assert kind.info.read(L) == E.InvalidAccess
    assert not L.beamformer_hip_get_last_frame_timings(C.byref(P.HipFrameTimings()))
    assert not L.beamformer_hip_frame_min_max((C.c_float * 2)())
    assert (sentinel == -7.0).all()
    # the last F + 1 frames: F tombstones are skipped, the older good frame is still exported; the call reports the missing newest one
    assert not L.beamformer_get_last_frames(sptr, sentinel.nbytes, F + 1)
    assert np.array_equal(sentinel[: older.nbytes // 4].view(np.uint32), older.reshape(-1).view(np.uint32))
    assert (sentinel[(older.nbytes + 63) // 64 * 16:] == -7.0).all()
    # every row of the failed push in the 32-frame table stays zero
    table = P.ComputeStatsTable()
    assert L.beamformer_compute_timings(C.byref(table), -1)
    for k in range(F):
        assert not any(table.times[(newest + 1 + k) % 32][col] for col in range(int(table.shader_count)))
    # the library is not wedged: the failed push consumed its F ids, the next good one takes the next F and is served whole
    L.beamformer_hip_set_das_path(flag)
    again = kind.push(bflib, case)
    assert kind.info.read(L) == (newest + 1 + F, F)
    assert route.reported(kind.info.newest(L), case)
    all_same_bits(again, good)


def test_only_the_newest_multi_frame_push_serves_its_info(bflib):
    """every beamformer_hip_get_last_*_info serves a push of its kind only while that push is the newest one, complete: after a good push
    of each kind in turn exactly that kind's call succeeds and the others are InvalidAccess (a sweep is served by the burst's call); after
    a single push, and after a push failed by flag 0x2000, none succeeds"""
    L = bflib.library()
    getters = list(dict.fromkeys(kind.info.getter for kind in KINDS))
    assert len(getters) == 5
    structs = {kind.info.getter: kind.info.struct for kind in KINDS}

    def served():
        return [getter for getter in getters if getattr(L, getter)(C.byref(structs[getter]())) or bflib.last_error()[0] != E.InvalidAccess]

    prepared = {kind.name: kind.case("newest_info") for kind in KINDS}
    for kind in KINDS:
        case = prepared[kind.name]
        L.beamformer_hip_set_das_path(case.path)
        kind.push(bflib, case)
        assert served() == [kind.info.getter], kind.name
    burst = prepared[BURST.name]
    bflib.beamform(burst.acq.bp, burst.rf[0], burst.acq.filters)
    assert served() == []
    # one RF frame on the views goes through the burst views push's code
    pair = prepared[BURST_VIEWS.name]
    VIEWS.push(bflib, prepared[VIEWS.name])
    assert served() == [VIEWS.info.getter]
    BURST_VIEWS.push(bflib, pair, rf=pair.rf[:1])
    assert served() == [BURST_VIEWS.info.getter]
    BURST_VIEWS.push(bflib, pair, rf=pair.rf[:2])
    bflib.beamform(pair.acq.bp, pair.rf[0], pair.acq.filters)
    assert served() == []
    for kind in KINDS:
        if kind.fails_on_flag:
            case = prepared[kind.name]
            L.beamformer_hip_set_das_path(case.path)
            kind.push(bflib, case)
            assert served() == [kind.info.getter], kind.name
            L.beamformer_hip_set_das_path(case.path | FAIL_DAS)
            rf, data, size = kind.data(case)
            assert not kind.raw(L, case, data, size) and bflib.last_error()[0] == E.InvalidAccess
            assert served() == [], kind.name
            L.beamformer_hip_set_das_path(0)


DEVICE_RF = [(kind, name) for kind in KINDS for name in kind.device_rf_cases]


@pytest.mark.parametrize("kind,name", DEVICE_RF, ids=[kind.name + ("-" + name if name else "") for kind, name in DEVICE_RF])
def test_device_resident_rf_equals_host_rf(kind, name, bflib):
    import torch
    case = kind.case("device_rf", name)
    bflib.library().beamformer_hip_set_das_path(case.path)
    host = kind.push(bflib, case)
    assert len(host) == kind.frames(case)
    dev = torch.from_numpy(np.ascontiguousarray(case.rf).view(np.uint8).reshape(-1)).cuda()
    torch.cuda.synchronize()
    device = kind.push(bflib, case, device_pointer=dev.data_ptr())
    all_same_bits(device, host)


@pytest.mark.parametrize("kind", KINDS, ids=IDS)
def test_a_refused_push_queues_nothing(kind, bflib, capfd):
    """the refusals of tests/test_push_contract_host.py with a device up -- the kind's malformed pushes, an output shard where the kind
    takes none, several devices --: no id is consumed, the newest frame and the kind's info stay what they were, and the same push
    afterwards gives the same bits"""
    L = bflib.library()
    case = kind.case("refusals")
    acq, F = case.acq, kind.frames(case)
    rf, data, size = kind.data(case)
    L.beamformer_hip_set_das_path(case.path)
    good = kind.push(bflib, case)
    newest = frame_id(L).frame_id
    served = kind.info.read(L)
    assert served == (newest - F + 1, F)

    def nothing_was_queued():
        assert frame_id(L).frame_id == newest and kind.info.read(L) == served

    for row in kind.malformed(case):
        if row.push:
            capfd.readouterr()
            assert not kind.raw(L, case, data, size, **row.overrides) and bflib.last_error()[0] == row.error, row
            assert row.word is None or row.word in capfd.readouterr().err, row
            nothing_was_queued()
    if kind.whole_grid:
        try:
            assert L.beamformer_hip_set_output_shard(0, *case.shard)
            capfd.readouterr()
            assert not kind.raw(L, case, data, size)
            assert bflib.last_error()[0] == E.InvalidAccess and "not sharded" in capfd.readouterr().err
        finally:
            assert L.beamformer_hip_set_output_shard(0, 0, 0)
        nothing_was_queued()
    # the newest frame is still the last one of the good push
    assert same_bits(kind.newest(bflib, case)[-1], good[-1])
    with two_devices_asked_for(L):
        assert L.beamformer_push_simple_parameters(C.byref(acq.bp))
        capfd.readouterr()
        assert not kind.raw(L, case, data, size)
        assert bflib.last_error()[0] == E.InvalidAccess
        assert "one device" in capfd.readouterr().err
        assert not L.beamformer_hip_get_last_frame_info(C.byref(P.HipFrameInfo()))                # nothing was queued
    L.beamformer_hip_set_das_path(case.path)
    all_same_bits(kind.push(bflib, case), good)


@pytest.mark.parametrize("kind", KINDS, ids=IDS)
def test_frame_graphs_change_nothing(kind, bflib):
    L = bflib.library()
    case = kind.case("graphs")
    L.beamformer_hip_set_das_path(case.path)
    plain = kind.push(bflib, case)
    try:
        L.beamformer_hip_enable_frame_graphs(1)
        for _ in range(2):            # (a plan's first frame never runs from a graph)
            graphs = kind.push(bflib, case)
        all_same_bits(graphs, plain)
    finally:
        L.beamformer_hip_enable_frame_graphs(0)


SHARDED = [kind for kind in KINDS if not kind.whole_grid]


@pytest.mark.parametrize("kind", SHARDED, ids=[kind.name for kind in SHARDED])
def test_an_output_shard_is_honoured(kind, bflib):
    """the kinds whose frames are the block's own grid: the planes of the shard, the same bits as those planes of the whole frame"""
    L = bflib.library()
    case = kind.case("shard")
    first, planes = case.shard
    rf, data, size = kind.data(case)
    whole = kind.push(bflib, case)
    try:
        assert L.beamformer_hip_set_output_shard(0, first, planes)
        assert kind.raw(L, case, data, size), bflib.last_error()
        assert kind.sharded_route(bflib)
        part = kind.newest(bflib, case, shard_planes=planes)
    finally:
        assert L.beamformer_hip_set_output_shard(0, 0, 0)
    assert len(part) == len(whole)
    for k in range(len(whole)):
        assert same_bits(part[k], np.ascontiguousarray(whole[k][first:first + planes])), k
