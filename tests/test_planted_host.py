"""Planted frames on the CPU (tests/planted.py): the oracle returns every hazard frame as it was planted -- one term a voxel, weight
1 --, describe_das names the kernel that will plant it on the device, and every hazard frame HAS what its docstring claims, measured
with the references the device tests judge against: so that tests/test_gpu_planted.py cannot pass because a hazard went missing."""
import numpy as np
import pytest

from ogl_beamforming_amd import lib
from oracle import binding as oracle
from tests import autocorr_ref, ensemble_ref, motion_ref, spatial_ref
from tests import frame_metrics_ref, frame_peaks_ref, frame_quantiles_ref
from tests import planted
from tests.planted_ref import (HAZARDS, PLATEAU_SHAPES, SHAPES, TAPS, autocorr_int64, convolve_int64, correlate_int64, exact, gram_int64, hazard,
                               integer_weights, mix_int64, to_kind)


@pytest.mark.parametrize("name,points,cplx", HAZARDS, ids=lambda v: str(v).replace(" ", ""))
def test_the_oracle_returns_what_was_planted_and_the_general_kernel_will_plant_it(name, points, cplx):
    values = hazard(name, points, cplx)
    assert values.shape == points[::-1] and np.iscomplexobj(values) == cplx
    acq = planted.block(values)
    frame, pairs = oracle.beamform(acq.bp, acq.rf, acq.filters)
    want = planted.expected(values)
    print(f"  {name} {points} {'complex' if cplx else 'real'}: pairs {pairs} of {acq.voxels} voxels")
    assert pairs == acq.voxels == values.size
    assert planted.same(frame, want)
    # -0 is the one thing that changes: the frame holds none, the planted array of `specials` does
    assert not (np.signbit(frame.view(np.float32)) & (frame.view(np.float32) == 0)).any()
    path, kernel, label, _, _ = lib.describe_das(acq.bp, acq.filters)
    assert (path, kernel) == (0, "das_kernel"), (path, kernel, label)


def test_same_tells_bits_apart_and_asks_nan_for_nan():
    want = planted.expected(np.array([[1.0, np.nan], [-0.0, planted.SUB_MIN]], np.float32))
    assert not np.signbit(want[1, 0, 0]) and planted.same(want.copy(), want)
    for at, value in (((0, 0, 0), np.nextafter(np.float32(1), np.float32(2))), ((0, 0, 1), 0.0), ((1, 0, 0), -0.0), ((1, 0, 1), 0.0)):
        other = want.copy()
        other[at] = value
        assert not planted.same(other, want), at
    assert not planted.same(want.astype(np.complex64), want) and not planted.same(want[:1], want)


# ----------------------------------------------------------------------------- teeth

@pytest.mark.parametrize("points", SHAPES)
@pytest.mark.parametrize("make", [planted.specials, planted.squares])
def test_specials_and_squares_hold_the_planned_non_finite_voxels_and_a_tied_maximum(make, points):
    values, plan = make(points)
    frame = planted.expected(values)
    X, Y, Z = points
    boxes = [None, ((1, 0, 1), (X - 2, Y, Z - 2)), ((0, 0, 0), (X // 2 + 1, max(1, Y // 2), Z // 2 + 1))]
    for box in boxes:
        row = frame_metrics_ref.metrics(frame, *(box if box else (None, None)))
        owed = planted.box_numbers(plan, box)
        print(f"  {make.__name__} {points} box {box}: non_finite {row['non_finite']}, pairs {row['gradient_pairs']}, max at {row['max_index']}")
        assert (row["non_finite"], row["gradient_pairs"]) == (owed["non_finite"], owed["gradient_pairs"])
        if owed["max_index"] is not None:
            assert row["max_index"] == owed["max_index"]
    whole = planted.box_numbers(plan)
    # the maximum is tied, and the lower flat index of the tie is the planned one; the second box cuts special voxels off
    assert len(plan["largest"]) >= 2 and whole["max_index"] == min(plan["largest"], key=lambda at: planted._flat(points, at))
    assert 0 < planted.box_numbers(plan, boxes[1])["non_finite"] < whole["non_finite"] >= 5
    q = frame_peaks_ref.decision(frame)
    at = lambda p: q[p[2], p[1], p[0]]
    assert all(not np.isfinite(at(p)) for p in plan["non_finite"]) and int((~np.isfinite(q)).sum()) == len(plan["non_finite"])
    assert all(at(p) == 0 for p in plan["zero"]) and all(0 < at(p) < planted.FLT_MIN for p in plan["subnormal"])
    assert len(plan["zero"]) >= 2 and len(plan["subnormal"]) >= 2
    if make is planted.squares:
        # nothing planted is infinite or NaN: q alone makes the voxel non-finite; and a q of 0 sits on a voxel that is not zero
        assert np.isfinite(frame.real).all() and np.isfinite(frame.imag).all()
        assert any(frame[p[2], p[1], p[0]] != 0 for p in plan["zero"])
        kinds = set(plan["kind"].values())
        assert kinds == {0, 1, 2, 3, 4}
        one = [p for p, k in plan["kind"].items() if k == 1][0]
        v = frame[one[2], one[1], one[0]]
        assert np.isfinite(np.float32(v.real * v.real)) and np.isfinite(np.float32(v.imag * v.imag)) and np.isinf(at(one))
    # quantiles: the non-finite voxels are in no rank, the zeros are the lowest plateau
    ranked = frame_quantiles_ref.quantiles(frame, [0.0, 1.0])
    assert ranked["non_finite"] == len(plan["non_finite"]) and ranked["voxels"] == frame.size - len(plan["non_finite"])
    assert (ranked["rows"][0]["value"], ranked["rows"][0]["below"], ranked["rows"][0]["equal"]) == (0.0, 0, len(plan["zero"]))


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("points", PLATEAU_SHAPES)
def test_plateaus_give_one_peak_each_at_the_lowest_flat_index_and_the_planned_fits(points, cplx):
    values, plan = planted.plateaus(points, cplx=cplx)
    frame = planted.expected(values)
    sizes = sorted(len(v) for v in plan["plateaus"].values())
    assert sizes[0] == 1 and 2 in sizes and sizes[-1] == (27 if points[1] > 1 else 24) and all(n <= 27 for n in sizes)
    q = frame_peaks_ref.decision(frame)
    for name, voxels in plan["plateaus"].items():
        heights = {float(q[z, y, x]) for x, y, z in voxels if np.isfinite(q[z, y, x])}
        assert len(heights) == 1 and heights.pop() >= (planted.HEIGHT ** 2 if cplx else planted.HEIGHT), name
    found = frame_peaks_ref.peaks(frame, float(planted.HEIGHT))
    index = [tuple(int(v) for v in i) for i in found["index"]]
    print(f"  {points} {'complex' if cplx else 'real'}: {found['found']} peaks at the plateaus' height, {found['above_threshold']} eligible voxels")
    # eligible: the plateaus' voxels but the NaN one, and the lower neighbours "rounding" and "collision" bring along
    assert index == plan["peaks"] and found["above_threshold"] == sum(sizes) - 1 + (2 if cplx else 1)
    # the lowest flat index of every plateau is one of them, and no two peaks are adjacent
    for voxels in plan["plateaus"].values():
        assert min(voxels, key=lambda at: planted._flat(points, at)) in index
    for a in index:
        assert not any(a != b and all(abs(i - j) <= 1 for i, j in zip(a, b)) for b in index)
    # the fits: +0.5, -0 with the axis fitted, +0 where den == 0 leaves it unfitted -- and -0.5 on the complex frame
    seen = set()
    for (at, axis), (offset, fitted) in plan["offsets"].items():
        k = index.index(at)
        got = found["offset"][k, axis]
        assert bool(found["fitted"][k] >> axis & 1) == fitted and got == offset and np.signbit(got) == np.signbit(np.float32(offset)), (at, axis)
        seen.add((float(offset), bool(np.signbit(np.float32(offset))), fitted))
    assert {(0.5, False, True), (0.0, True, True), (0.0, False, False)} <= seen and ((-0.5, True, True) in seen) == cplx
    # threshold 0: the background's own ties make peaks too, and the plateaus' are among them
    everywhere = frame_peaks_ref.peaks(frame, 0.0)
    assert everywhere["found"] > 4 * found["found"] and set(plan["peaks"]) <= {tuple(int(v) for v in i) for i in everywhere["index"]}
    # metrics: the NaN voxel, and two voxels tied for max_abs
    row = frame_metrics_ref.metrics(frame)
    owed = planted.box_numbers(plan)
    assert (row["non_finite"], row["gradient_pairs"], row["max_index"]) == (1, owed["gradient_pairs"], owed["max_index"])
    m = row["magnitude"]
    assert len(plan["largest"]) == 2 and all(m[z, y, x] == row["max_abs"] == planted.BIG for x, y, z in plan["largest"])


def test_radix_puts_ranks_on_every_pass_boundary():
    values, plan = planted.radix()
    frame = planted.expected(values)
    assert frame.size == 8192
    bits, non_finite = frame_quantiles_ref.finite_bits(frame)
    ordered = np.sort(bits)
    n = len(ordered)
    assert (n, non_finite) == (8192, 0) and np.array_equal(ordered, plan["keys"])
    fractions = [f for part in plan["fractions"] for f in part]
    assert all(len(part) <= 16 for part in plan["fractions"])
    # the preconditions, on the ranks the definition gives these fractions (the style of test_deep_passes_decide)
    assert [int(r) for r in frame_quantiles_ref.ranks(fractions, n)] == plan["ranks"]
    rows = frame_quantiles_ref.quantiles(frame, fractions)["rows"]
    keys = np.array([r["value_bits"] for r in rows], np.uint32)
    assert len(np.unique(keys >> np.uint32(20))) >= 3 and 0 in keys >> np.uint32(20) and 2039 in keys >> np.uint32(20)
    by_rank = dict(zip(plan["ranks"], keys))
    a, b = (int(by_rank[r]) for r in plan["groups"]["bit 0"])
    assert a >> 10 == b >> 10 and a != b                                            # pass 3 alone decides
    a, b = (int(by_rank[r]) for r in plan["groups"]["bit 10"])
    assert a >> 20 == b >> 20 and a >> 10 != b >> 10 and a & 0x3FF == b & 0x3FF     # pass 2 alone decides
    a, b = (int(by_rank[r]) for r in plan["groups"]["bit 20"])
    assert a >> 20 != b >> 20 and a & 0xFFFFF == b & 0xFFFFF                         # pass 1 alone decides
    # the tie fills half the frame, and ranks sit on its first and its last index and on either side of it
    first, last = plan["tie"]
    assert last - first + 1 == n // 2 and {first - 1, first, last, last + 1} <= set(plan["ranks"])
    tie = [r for r in rows if r["value_bits"] == planted.RADIX_TIE]
    assert len(tie) == 2 and all((r["below"], r["equal"]) == (first, n // 2) for r in tie)
    print(f"  ranks {plan['ranks']}, keys {[hex(int(k)) for k in keys]}")


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("K", [3, 17])
@pytest.mark.parametrize("points", PLATEAU_SHAPES)
def test_integer_frames_make_every_reference_exact(points, K, cplx):
    frames = planted.integers(K, points, cplx=cplx)
    assert frames.shape == (K,) + points[::-1] and np.abs(planted.expected(frames[0]).view(np.float32)).max() == 64
    assert not np.array_equal(frames[0], frames[1])
    # gram
    G, voxels, non_finite, _ = ensemble_ref.gram(list(frames))
    assert (voxels, non_finite) == (frames[0].size, 0) and np.array_equal(G, gram_int64(frames).astype(np.complex128))
    # mix: K -> 3 frames
    W = integer_weights(3, K, cplx)
    mixed, _ = ensemble_ref.mix(list(frames), W)
    mr, mi = mix_int64(frames, W)
    assert max(np.abs(mr).max(), np.abs(mi).max()) < 2 ** 24
    assert np.array_equal(mixed, to_kind(mr, mi, cplx, mixed.dtype))
    # autocorrelate: the identity form (K rows), and -- K == 3 -- the filtered form; every running sum stays below 2^24
    for weights in ([None, W] if K == 3 else [None]):
        y = exact(frames) if weights is None else (mr, mi)
        ar, ai = autocorr_int64(*y, 3)
        ai[0] = 0
        rows = len(y[0])
        assert 2 * rows * max(np.abs(y[0]).max(), np.abs(y[1]).max()) ** 2 < 2 ** 24
        got, _ = autocorr_ref.autocorrelate(list(frames), weights, 3)
        assert np.array_equal(got, to_kind(ar, ai, cplx, got.dtype))
    # convolve
    taps = (TAPS[0], None if points[1] == 1 else TAPS[1], TAPS[2])
    cr, ci = convolve_int64(frames[1], taps)
    got, _ = spatial_ref.convolve(frames[1], taps)
    assert np.array_equal(got, to_kind(cr, ci, cplx, got.dtype)) and np.array_equal(spatial_ref.convolve_float32(frames[1], taps), got.astype(frames.dtype))
    # correlate: the first three frames, the window (1, 1 | 0, 2)
    window = (1, 0 if points[1] == 1 else 1, 2)
    table, _ = motion_ref.correlate(list(frames[:3]), 1, window)
    want = correlate_int64(frames[:3], 1, window)
    for n, name in enumerate(("re", "im", "energy_reference", "energy_frame", "terms")):
        assert np.array_equal(table[0][name], want[n].astype(table[name].dtype)), name
