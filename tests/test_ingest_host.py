"""The ingest matrix of tests/ingest_cases.py on the CPU: its numpy reference against the oracle's channel map, bit for bit, before
either judges the device; and -- through beamformer_hip_describe_upload, which needs no device -- that every case takes the upload
route, the ingest kernel and the lane width its name promises, and that the matrix as a whole reaches every route, width and A1S2
instantiation of csrc/executor.cpp's decide_upload and csrc/stages.hip's ingest kernels."""
import os
import re

import numpy as np
import pytest

from ogl_beamforming_amd import lib
from ogl_beamforming_amd import params as P
from oracle import binding as oracle
from tests import ingest_cases as IC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = P.UploadRoute
DEVICE_POINTER = 0x7F0000000000          # a 4 KiB-aligned address: nothing dereferences it


def overlap_bytes():
    src = open(os.path.join(ROOT, "ogl_beamforming_amd", "csrc", "executor.cpp")).read()
    m = re.search(r"constexpr\s+uint64_t\s+kOverlapBytes\s*=\s*(\d+)ull\s*<<\s*(\d+)\s*;", src)
    assert m, "kOverlapBytes not found in csrc/executor.cpp"
    return int(m.group(1)) << int(m.group(2))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("name", sorted(IC.CASES))
def test_numpy_reference_is_the_oracles_channel_map(name):
    acq = IC.make(name)
    ours, theirs = IC.mapped_rf(acq), oracle.channel_map(acq.bp, acq.rf)
    assert ours.shape == theirs.shape and ours.dtype == theirs.dtype
    assert np.array_equal(bits(ours), bits(theirs)), name
    c = IC.CASES[name]
    if c.mapping != "identity":
        assert [int(acq.bp.channel_mapping[ch]) for ch in range(c.channels)] != list(range(c.channels)), "the mapping drawn is the identity"
    if c.contrast:                     # only transmit 0's samples are produced, the rest of the row is zero
        k = c.samples * IC.scalars(c.kind)
        assert ours[:, :k].any() and not bits(ours[:, k:]).any()


@pytest.mark.parametrize("name", sorted(IC.CASES))
def test_every_case_takes_the_route_its_name_promises(name):
    c, acq = IC.CASES[name], IC.make(name)
    threshold = overlap_bytes()
    d = lib.describe_upload(acq.bp, acq.rf.nbytes)
    assert d.upload_bytes == acq.rf.nbytes and d.rf_bytes == IC.mapped_rf(acq).nbytes
    assert (acq.rf.nbytes >= threshold) == (c.route != R.PinnedInPlace), (acq.rf.nbytes, threshold)
    if c.group in ("small", "planted"):
        assert acq.rf.nbytes < threshold and d.route == R.PinnedInPlace
    if c.group == "large":
        assert threshold <= acq.rf.nbytes <= 10 << 20
    assert (R(d.route), d.ingest_kernel, d.copy_bytes) == (c.route, c.kernel, c.width), (d.name, d.ingest_kernel, d.copy_bytes)
    assert d.name.decode() == {R.PinnedInPlace: "pinned-in-place", R.CopyEngineDirect: "copy-engine-direct", R.CopyEngineStaged: "copy-engine-staged"}[c.route]
    assert d.a1s2_base == IC.BASE_OF[IC.numpy_base(c.kind)]
    on_device = lib.describe_upload(acq.bp, acq.rf.nbytes, device_pointer=DEVICE_POINTER)
    assert R(on_device.route) == c.device_route, on_device.name
    assert on_device.ingest_kernel == (c.kernel if c.device_route == R.DeviceIngest else 0)
    assert on_device.copy_bytes == (c.width if on_device.ingest_kernel == 1 else 0)


def test_matrix_reaches_every_route_width_and_a1s2_kind():
    host, device, widths, a1s2 = set(), set(), set(), set()
    for name, c in IC.CASES.items():
        acq = IC.make(name)
        d = lib.describe_upload(acq.bp, acq.rf.nbytes)
        host.add(R(d.route))
        if c.group == "small" or name == "big_shuffled_padded":           # what the device tests push from a device buffer
            device.add(R(lib.describe_upload(acq.bp, acq.rf.nbytes, device_pointer=DEVICE_POINTER).route))
        if d.ingest_kernel == 1 and c.mapping != "identity":
            widths.add(int(d.copy_bytes))
        if d.ingest_kernel == 2:
            a1s2.add((int(d.a1s2_base), IC.scalars(c.kind)))
    assert host | device == set(R) and host == {R.PinnedInPlace, R.CopyEngineDirect, R.CopyEngineStaged}
    assert widths == {16, 4, 2}
    assert {base for base, _ in a1s2} == {0, 1, 2}, "an instantiation of ingest_a1s2_kernel never runs"
    assert {base for base, n in a1s2 if n == 2} == {0, 1, 2}, "a complex A1S2 kind never runs"
    # ... and the small cases alone: six kinds x contrast off / on, three widths under a shuffled mapping
    small = [IC.CASES[n] for n in IC.SMALL]
    assert {(c.kind, c.contrast) for c in small} == {(k, on) for k in P.DataKind for on in (False, True)}
    assert {c.width for c in small if c.mapping == "shuffled" and not c.contrast} == {16, 4, 2}


def test_burst_routes():
    """a burst's route goes by its total: three small frames stay pinned in place, five frames of 2 MiB go over the copy engine; the
    ingest kernel always runs, and the raw frame stride enters the lane width"""
    acq = IC.make("Int16_w16_identity")
    d = lib.describe_upload(acq.bp, acq.rf.nbytes, 3)
    assert (R(d.route), d.ingest_kernel, d.copy_bytes) == (R.PinnedInPlace, 1, 16)
    assert R(lib.describe_upload(acq.bp, acq.rf.nbytes, 3, device_pointer=DEVICE_POINTER).route) == R.DeviceIngest
    odd = IC.make("Int16_w2_pad37")                        # 8784 bytes per raw frame = 16 x 549: the rows alone decide
    assert lib.describe_upload(odd.bp, odd.rf.nbytes, 3).copy_bytes == 2
    quad = IC.make("Int16_w4_pad2")                        # 8224 = 4 x 2056
    assert lib.describe_upload(quad.bp, quad.rf.nbytes, 3).copy_bytes == 4
    big = IC.burst_case()
    threshold = overlap_bytes()
    assert big.rf.nbytes < threshold <= 5 * big.rf.nbytes
    assert R(lib.describe_upload(big.bp, big.rf.nbytes).route) == R.PinnedInPlace
    d = lib.describe_upload(big.bp, big.rf.nbytes, 5)
    assert (R(d.route), d.ingest_kernel, d.upload_bytes) == (R.CopyEngineStaged, 1, 5 * big.rf.nbytes)
    L = lib.library()
    assert not L.beamformer_hip_describe_upload(0, big.rf.nbytes - 2, 1, None, P.HipUploadDescription())
    assert lib.last_error()[0] == P.LibError.DataSizeMismatch
    assert not L.beamformer_hip_describe_upload(0, big.rf.nbytes, 0, None, P.HipUploadDescription())


@pytest.mark.parametrize("name", IC.LONG)
def test_long_rows_take_a_second_trip_of_the_grid_stride_loop(name):
    c, acq = IC.CASES[name], IC.make(name)
    d = lib.describe_upload(acq.bp, acq.rf.nbytes)
    row_bytes = d.rf_bytes // c.channels
    lane = d.copy_bytes if d.ingest_kernel == 1 else np.dtype(IC.numpy_base(c.kind)).itemsize
    assert row_bytes // lane > IC.COPY_TRIP, (row_bytes, lane)
    assert row_bytes // lane < 2 * IC.COPY_TRIP, "no need for a third trip"
    assert [int(acq.bp.channel_mapping[ch]) for ch in range(2)] == [1, 0]


def test_device_pointer_alignment_lowers_the_lane_width():
    acq = IC.make("Int16_w16_pad40")
    got = [int(lib.describe_upload(acq.bp, acq.rf.nbytes, device_pointer=DEVICE_POINTER + off).copy_bytes) for off in (0, 2, 4, 8, 16)]
    assert got == [16, 2, 4, 4, 16]
    # the rows bound it from above; a host push does not depend on the caller's pointer at all
    quad = IC.make("Int16_w4_pad2")
    assert [int(lib.describe_upload(quad.bp, quad.rf.nbytes, device_pointer=DEVICE_POINTER + off).copy_bytes) for off in (0, 2, 4, 8)] == [4, 2, 4, 4]


@pytest.mark.parametrize("name", IC.PLANTED)
def test_planted_extremes_are_in_the_oracles_das_input(name):
    c, acq = IC.CASES[name], IC.make(name)
    captured = {}
    oracle.beamform(acq.bp, acq.rf, acq.filters, das_input=captured)
    das_in = captured["data"]
    mapped = IC.mapped_rf(acq)
    assert np.array_equal(bits(das_in), bits(IC.das_input_of(acq, mapped))), "the oracle's DAS input is not the mapped RF converted"
    assert not np.isnan(das_in).any()
    triples, expect = IC.PLANTS[name]
    seen = set()
    for ch, s, i in IC.planted_positions(name):
        got = float(das_in[ch, 0, s])
        if expect[i] is not None:
            assert got == expect[i], (ch, s, triples[i], got)
        seen.add(got)
    values = np.array([das_in[ch, 0, s] for ch, s, _ in IC.planted_positions(name)], np.float32)
    if name == "planted_Int16":
        exact = np.array([a - b - cc for a, b, cc in triples])
        assert (np.abs(exact) > 32767).sum() >= 8, "too few triples leave the int16 range"
    if name == "planted_Float16":
        tiny = np.abs(values[np.isfinite(values) & (values != 0)])
        assert np.isposinf(values).any() and np.isneginf(values).any() and (tiny < 2.0 ** -14).any()
    if name == "planted_Float32":
        tiny = np.abs(values[np.isfinite(values) & (values != 0)])
        assert np.isposinf(values).any() and np.isneginf(values).any() and (tiny < 2.0 ** -126).any()
