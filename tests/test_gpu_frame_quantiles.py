"""Frame quantiles on the device (beamformer_hip_quantiles_last_frames; csrc/frame_quantiles.hip).  Frames are produced by ordinary pushes
and downloaded; the expected rows are the numpy reference (tests/frame_quantiles_ref.py) applied to those downloaded arrays -- parity of
the frames themselves is other tests' business.

There is no tolerance anywhere: every field is compared for equality, the floats by their bits.  The definition is integer counting
over float32 values numpy forms by the same basic IEEE operations, so nothing else would be honest.  Every call prints the bytes of the
boxes it ranked and its device time."""
import ctypes as C

import numpy as np
import pytest

from ogl_beamforming_amd import params as P
from tests import frame_peaks_ref
from tests import frame_quantiles_ref as ref
from tests import variants_cases as vc
from tests.ring_frames import bits, metrics_block as block, BOX, finer, FRACTIONS, map_view, placement_onto, ranked, region_of, variants_push
from tests.scaffold import automatic_path  # noqa: F401

pytestmark = pytest.mark.gpu
E = P.LibError


@pytest.fixture(autouse=True)
def map_reset(automatic_path, bflib):
    yield
    bflib.localisation_map_reset(None)


def test_block_a_three_variants_of_a_complex_plane(bflib):
    frames, ids = variants_push("A")
    assert np.iscomplexobj(frames)
    rows, _, _, _ = bflib.quantiles_last_frames(3, FRACTIONS)
    assert [int(r.frame_id) for r in rows] == ids
    expected = ranked(frames, FRACTIONS)
    # the three frames' medians differ: a kernel that reads one frame for every row fails above
    medians = [e["rows"][0]["value_bits"] for e in expected]
    assert len(set(medians)) == 3, medians
    # f = 0 and f = 1 are the extremes, and the repeat repeats
    for e in expected:
        assert e["rows"][4]["rank"] == 0 and e["rows"][1]["rank"] == e["voxels"] - 1 and e["rows"][0] == e["rows"][5]
    ranked(frames, FRACTIONS, ((5, 0, 7), (11, 1, 21)))


def test_block_b_real_frames(bflib):
    frames, _ = variants_push("B")
    assert frames.dtype == np.float32
    ranked(frames, FRACTIONS)
    ranked(frames, FRACTIONS, ((5, 0, 7), (11, 1, 21)))
    # one fraction, the most the call takes, and the thresholds of real frames are the values
    ranked(frames, [0.25])
    expected = ranked(frames, np.linspace(0.0, 1.0, P.HIP_MAX_QUANTILES))
    assert all(bits(q["threshold"]) == q["value_bits"] for e in expected for q in e["rows"])


def d3_frame(bflib):
    acq = block("D3")
    frame = bflib.beamform(acq.bp, acq.rf, acq.filters).copy()
    assert frame.shape == (32, 16, 16) and np.iscomplexobj(frame)
    return frame


def test_block_d3_nan_voxels_take_part_in_no_rank(bflib):
    frame = d3_frame(bflib)
    nan = int(np.isnan(frame).sum())
    assert nan >= 64
    for box in (None, BOX):
        want = ranked([frame], FRACTIONS, box)[0]
        assert want["non_finite"] >= (nan if box is None else 1) and want["voxels"] + want["non_finite"] == int(np.prod(want["region_count"]))
        assert np.isfinite([q["value"] for q in want["rows"]]).all()
    # a box without any finite voxel: every number 0
    z, y, x = (int(v[0]) for v in np.nonzero(np.isnan(frame)))
    want = ranked([frame], FRACTIONS, ((x, y, z), (1, 1, 1)))[0]
    assert want["voxels"] == 0 and want["non_finite"] == 1
    rows, records, tables, _ = bflib.quantiles_last_frames(1, FRACTIONS, region_of(((x, y, z), (1, 1, 1))), histograms=True)
    assert not tables.any() and all((r.rank, r.below, r.equal, r.value, r.magnitude, r.threshold) == (0, 0, 0, 0.0, 0.0, 0.0) for r in records)


def test_mixed_grids_and_kinds_in_one_call(bflib):
    a, forces = block("A"), block("forces")
    frame_a = bflib.beamform(a.bp, a.rf, a.filters).copy()
    frame_f = bflib.beamform(forces.bp, forces.rf, forces.filters).copy()
    assert np.iscomplexobj(frame_a) and frame_a.shape == (40, 1, 24) and frame_f.dtype == np.float32 and frame_f.shape == (32, 16, 16)
    ranked([frame_a, frame_f], FRACTIONS)
    ranked([frame_a, frame_f], FRACTIONS, ((2, 0, 3), (9, 1, 20)))


def test_deep_passes_decide(bflib):
    """Ranks chosen in numpy so that the second and the third digit pass each have something to decide, the preconditions asserted before
    the call.  Block D3's frame does not serve: its 2464 finite voxels hold 154 distinct values (the geometry is symmetric) and no two of
    them share a 1024-key window.  Block C's does, the smallest of the suite with 8192 voxels that does: 16 x 16 x 32, complex, every value
    its own, several hundred windows of two keys or more."""
    acq = block("C")
    frame = bflib.beamform(acq.bp, acq.rf, acq.filters).copy()
    assert frame.shape == (32, 16, 16) and np.iscomplexobj(frame) and frame.size >= 8192
    values, _ = ref.finite_bits(frame)
    ordered = np.sort(values)
    n = len(ordered)
    keys = np.unique(ordered)
    windows, coarse = keys >> np.uint32(10), keys >> np.uint32(20)
    # (a) a 1024-key window with two distinct keys or more: the ranks of its two lowest keys differ in bits 9..0 only
    shared, counts = np.unique(windows, return_counts=True)
    assert (counts >= 2).any(), "block C holds no window of two distinct keys"
    in_window = keys[windows == shared[np.argmax(counts >= 2)]]
    a1, a2 = (int(np.searchsorted(ordered, k)) for k in in_window[:2])
    # (b) two keys of one coarse bin in different windows; (c) a key of another coarse bin than (a)'s
    b1 = b2 = c = None
    for bin_ in np.unique(coarse):
        mine = keys[coarse == bin_]
        if b1 is None and len(np.unique(mine >> np.uint32(10))) >= 2:
            b1, b2 = int(np.searchsorted(ordered, mine[0])), int(np.searchsorted(ordered, mine[-1]))
        if c is None and bin_ != in_window[0] >> np.uint32(20):
            c = int(np.searchsorted(ordered, mine[0]))
    assert None not in (b1, b2, c)
    picked = [a2, b1, c, a1, b2]
    fractions = [r / (n - 1) for r in picked]
    # the preconditions, on the ranks the definition gives these fractions
    assert [int(r) for r in ref.ranks(fractions, n)] == picked
    at = ordered[picked]
    assert at[0] >> 10 == at[3] >> 10 and at[0] != at[3]                                    # pass 3 decides between a1 and a2
    assert at[1] >> 20 == at[4] >> 20 and at[1] >> 10 != at[4] >> 10                        # pass 2 decides between b1 and b2
    assert at[2] >> 20 != at[0] >> 20                                                       # pass 1 decides between a and c
    print(f"  n {n}, distinct keys {len(keys)}, windows of two keys or more {int((counts >= 2).sum())}; ranks {picked}, keys {[hex(int(k)) for k in at]}")
    want = ranked([frame], fractions)[0]
    assert [q["value_bits"] for q in want["rows"]] == [int(k) for k in at]
    ranked([frame], fractions, BOX)


def queued_map_frame(bflib):
    """a localisation map of block B's three variants, deposited three times, queued as a frame: mostly zeros, few distinct values"""
    acq = block("B")
    frames, _ = variants_push("B")
    grid = map_view(finer(vc.POINTS), vc.LO, vc.HI)
    A = placement_onto(grid, acq.bp.das_voxel_transform, vc.POINTS)
    thresholds = [0.1 * float(np.abs(f).max()) for f in frames]
    bflib.localisation_map_reset(grid.output_points)
    for use_offsets in (True, True, False):
        bflib.accumulate_peaks_last_frames(3, thresholds, A, use_offsets)
    frame_id, _ = bflib.queue_localisation_map(0.37, tag=5)
    return bflib.copy_frame(frame_id)


def test_ties_a_queued_localisation_map_and_an_all_zero_frame(bflib):
    queued = queued_map_frame(bflib)
    distinct = np.unique(queued)
    print(f"  the queued map: {queued.shape}, {int((queued == 0).sum())} zeros of {queued.size}, distinct values {distinct}")
    assert queued.dtype == np.float32 and 2 * int((queued == 0).sum()) > queued.size and 3 <= len(distinct) <= 64
    want = ranked([queued], [0.0, 0.5, 0.9, 0.99, 0.999, 1.0, 0.995])[0]
    zeros = int((queued == 0).sum())
    assert (want["rows"][1]["value"], want["rows"][1]["below"], want["rows"][1]["equal"]) == (0.0, 0, zeros)       # f = 0.5 lands in the plateau
    assert want["rows"][5]["value"] == distinct[-1] and want["rows"][5]["below"] + want["rows"][5]["equal"] == queued.size
    ranked([queued], [0.5, 0.999], ((3, 0, 2), (80, 1, 150)))
    # zero weights: an all-zero frame (of either sign of zero: q is +0)
    first, _ = bflib.mix_last_frames(1, np.zeros((1, 1), np.complex64))
    zero = bflib.copy_frame(first)
    assert zero.shape == queued.shape and not zero.any()
    want = ranked([zero], FRACTIONS)[0]
    assert all((q["value_bits"], q["below"], q["equal"]) == (0, 0, zero.size) for q in want["rows"])
    # and the two frames in one call, each with its own plateau
    ranked([queued, zero], FRACTIONS)


def test_without_histograms_the_other_outputs_are_the_same_bytes(bflib):
    frames, _ = variants_push("A")
    for box in (None, ((5, 0, 7), (11, 1, 21))):
        with_rows, with_records, tables, _ = bflib.quantiles_last_frames(3, FRACTIONS, region_of(box), histograms=True)
        rows, records, none, _ = bflib.quantiles_last_frames(3, FRACTIONS, region_of(box), histograms=False)
        assert none is None and tables is not None
        assert bytes(rows) == bytes(with_rows) and bytes(records) == bytes(with_records)
    ranked(frames, FRACTIONS, histograms=False)


def test_the_same_call_twice_and_split_calls_give_the_same_bytes(bflib):
    variants_push("C")
    K, each = len(FRACTIONS), C.sizeof(P.HipFrameQuantile) * len(FRACTIONS)

    def without_first(rows):
        """a frame's row without `first`, which says where in THIS call's records the frame's stand"""
        return [bytes(r)[:52] + bytes(r)[56:] for r in rows]

    assert P.HipFrameQuantiles.first.offset == 52
    for box in (None, BOX):
        region = region_of(box)
        three, three_records, three_tables, _ = bflib.quantiles_last_frames(3, FRACTIONS, region, histograms=True)
        again, again_records, again_tables, _ = bflib.quantiles_last_frames(3, FRACTIONS, region, histograms=True)
        assert bytes(three) == bytes(again) and bytes(three_records) == bytes(again_records) and three_tables.tobytes() == again_tables.tobytes()
        one, one_records, one_tables, _ = bflib.quantiles_last_frames(1, FRACTIONS, region, histograms=True)
        two, two_records, two_tables, _ = bflib.quantiles_last_frames(2, FRACTIONS, region, histograms=True)
        assert without_first(one) == without_first(three)[2:] and without_first(two) == without_first(three)[1:]
        assert bytes(one_records) == bytes(three_records)[2 * each:] and bytes(two_records) == bytes(three_records)[each:]
        assert one_tables.tobytes() == three_tables[2:].tobytes() and two_tables.tobytes() == three_tables[1:].tobytes()
        assert [int(r.first) for r in three] == [0, K, 2 * K] and int(one[0].first) == 0
    # no region is the explicit whole-frame box, byte for byte
    whole = bflib.quantiles_last_frames(3, FRACTIONS, bflib.frame_region((0, 0, 0), (16, 16, 32)))
    none = bflib.quantiles_last_frames(3, FRACTIONS)
    assert bytes(whole[0]) == bytes(none[0]) and bytes(whole[1]) == bytes(none[1])


@pytest.mark.parametrize("which", ["A", "B"])
def test_closing_the_loop_the_threshold_of_a_quantile_handed_to_find_peaks(which, bflib):
    frames, _ = variants_push(which)
    for box in (None, ((5, 0, 7), (11, 1, 21))):
        rows, records, _, _ = bflib.quantiles_last_frames(3, [0.99], region_of(box))
        thresholds = [float(r.threshold) for r in records]
        found, _, _ = bflib.find_peaks_last_frames(3, thresholds, 64, region_of(box))
        for k, frame in enumerate(frames):
            values, _ = ref.finite_bits(frame, *(box if box else (None, None)))
            q = values.view(np.float32)
            level = frame_peaks_ref.level(frame, np.float32(thresholds[k]))
            eligible = int((q >= level).sum())
            print(f"  {which} frame {k} box {box}: value {float(records[k].value)!r} threshold {thresholds[k]!r} level {float(level)!r}: "
                  f"above_threshold {int(found[k].above_threshold)}, numpy {eligible}, n - below {int(rows[k].voxels - records[k].below)}")
            assert found[k].threshold == np.float32(thresholds[k]) and level <= records[k].value
            assert int(found[k].above_threshold) == eligible >= int(rows[k].voxels) - int(records[k].below) >= 1
            # nothing else is eligible unless its q lies in [fl(T * T), value)
            assert eligible - (int(rows[k].voxels) - int(records[k].below)) == int(((q >= level) & (q < records[k].value)).sum())


def test_refusals_on_a_live_device_leave_the_outputs_alone(bflib):
    L = bflib.library()
    L.beamformer_hip_shutdown()                       # (the ids start again: three frames are all this device has queued)
    _, ids = variants_push("A")
    assert ids == [0, 1, 2]
    K = 3
    frames, records = (P.HipFrameQuantiles * 8)(), (P.HipFrameQuantile * (8 * K))()
    tables = np.full((8, P.HIP_QUANTILE_BINS), 0xA5A5A5A5, np.uint32)
    C.memset(frames, 0x5A, C.sizeof(frames))
    C.memset(records, 0x5A, C.sizeof(records))
    untouched = (bytes(frames), bytes(records), tables.tobytes())
    ms = C.c_float(-1.0)

    def refused(kind, count, fractions, region=None):
        values = (C.c_double * max(1, len(fractions)))(*fractions)
        assert not L.beamformer_hip_quantiles_last_frames(count, None if region is None else C.byref(region), values, len(fractions), frames, records,
                                                          tables.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(ms))
        assert bflib.last_error()[0] == kind and (bytes(frames), bytes(records), tables.tobytes()) == untouched and ms.value == -1.0

    good = [0.0, 0.5, 1.0]
    refused(E.BufferOverflow, 0, good)
    refused(E.BufferOverflow, 1, [])
    refused(E.BufferOverflow, 1, [0.5] * (P.HIP_MAX_QUANTILES + 1))
    refused(E.InvalidAccess, 1, [0.0, float("nan"), 1.0])
    refused(E.InvalidAccess, 1, [0.0, 1.5, 1.0])
    # a zero count in a region, regions that do not fit the 24 x 1 x 40 frames
    refused(E.InvalidAccess, 3, good, bflib.frame_region((0, 0, 0), (24, 0, 40)))
    refused(E.InvalidAccess, 3, good, bflib.frame_region((0, 0, 0), (25, 1, 40)))
    refused(E.InvalidAccess, 3, good, bflib.frame_region((1, 0, 0), (24, 1, 40)))
    refused(E.InvalidAccess, 1, good, bflib.frame_region((0xFFFFFFFF, 0, 0), (2, 1, 1)))
    # more frames than were ever queued
    refused(E.InvalidAccess, 4, good)
    # and the call still serves
    rows, _, _, _ = bflib.quantiles_last_frames(3, good)
    assert [int(r.stored) for r in rows] == [3, 3, 3]
