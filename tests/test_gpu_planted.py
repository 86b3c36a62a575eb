"""The frame operations on PLANTED frames (tests/planted.py): frames whose voxels the test chose -- ties, infinities, squares that
overflow or underflow, subnormals, keys that differ in one bit, small integers -- planted through blocks whose DAS sum has one term a
voxel with weight 1.  Every push asserts that the frame came back as planted; every test asserts that the hazard it aims at is
present in the DOWNLOADED frame and runs its reference on that frame.

Every result is judged by the test of its own operation: its reference, its comparator and its bars are imported from there, and
nothing here restates them (as tests/test_gpu_frame_ops_shared_state.py does).  What this file adds is compared for equality: planned
counts, planned indices, planned offsets, the int64 results of the integer frames.  There is no tolerance in this file."""
import numpy as np
import pytest

from tests import frame_peaks_ref, frame_quantiles_ref, localisation_ref, tracks_ref
from tests import planted
from tests import ring_frames
from tests import planted_ref
from tests import variants_cases as vc
from tests.ring_frames import planted_burst as burst, planted_push as push, region_of
from tests.scaffold import automatic_path  # noqa: F401

pytestmark = pytest.mark.gpu
PLANE, WAVE, VOLUME = planted.PLANE, planted.WAVE, planted.VOLUME
HEIGHT = float(planted.HEIGHT)
SHIFT = (1, 0, 2)


def grid_name(points, cplx):
    return f"planted_{'x'.join(str(p) for p in points)}_{'complex' if cplx else 'real'}"


# the planted shapes by names of this file's in the ensemble tests' GRIDS: the comparators of mix, autocorrelate, convolve and warp
# ask their module's block for the shape and the kind of the frames they download, and for nothing else
for _points in (PLANE, WAVE, VOLUME):
    for _cplx in (False, True):
        ring_frames.GRIDS[grid_name(_points, _cplx)] = (_points, vc.LO if _points[1] == 1 else vc.LO3, vc.HI if _points[1] == 1 else vc.HI3, _cplx)


@pytest.fixture(autouse=True)
def maps_reset(automatic_path, bflib):
    yield
    bflib.localisation_map_reset(None)
    bflib.track_map_reset(None)


def at(array, position):
    return array[position[2], position[1], position[0]]


def present(frame, plan):
    """the planned hazards are in the downloaded frame: q is not finite exactly at the planned voxels, 0 and subnormal where planned,
    and the planned voxels tie for the largest finite magnitude"""
    q = frame_peaks_ref.decision(frame)
    holes = {tuple(int(v) for v in i[::-1]) for i in np.argwhere(~np.isfinite(q))}
    assert holes == set(plan["non_finite"]) and len(holes) >= 1
    assert all(at(q, p) == 0 for p in plan.get("zero", [])) and all(0 < at(q, p) < planted.FLT_MIN for p in plan.get("subnormal", []))
    largest = [at(q, p) for p in plan["largest"]]
    assert len(largest) >= 2 and len(set(float(v) for v in largest)) == 1 and largest[0] == q[np.isfinite(q)].max()


def cut(points):
    """a box whose faces cut through the planted voxels: they sit at 0, 1, n / 3, n / 2, n - 2 and n - 1 of every axis; the box runs
    from 1 to n / 2, so some lie on its faces, some one voxel outside them"""
    X, Y, Z = points
    return (1, min(1, Y - 1), 1), (X // 2, max(1, Y // 2), Z // 2)


def inner(points):
    """the frame without its outermost voxels along every axis of more than one point"""
    return tuple(min(1, n - 1) for n in points), tuple(max(1, n - 2) for n in points)


def halves(points):
    """the boxes that tile a frame, every axis of more than one point cut in two"""
    spans = [[(0, n)] if n == 1 else [(0, n // 2), (n // 2, n - n // 2)] for n in points]
    return [((x[0], y[0], z[0]), (x[1], y[1], z[1])) for z in spans[2] for y in spans[1] for x in spans[0]]


HAZARDS = [("specials", p, False) for p in (PLANE, WAVE, VOLUME)] + [("squares", p, True) for p in (PLANE, WAVE, VOLUME)] + \
          [("plateaus", p, c) for p in (PLANE, VOLUME) for c in (False, True)]
IDS = [f"{n}-{'x'.join(str(v) for v in p)}-{'complex' if c else 'real'}" for n, p, c in HAZARDS]


def make(name, points, cplx, seed=0):
    if name == "specials":
        return planted.specials(points, seed)
    if name == "squares":
        return planted.squares(points, seed)
    return planted.plateaus(points, seed, cplx)


# ----------------------------------------------------------------------------- planting on the device

@pytest.mark.parametrize("name,points,cplx", planted_ref.HAZARDS, ids=lambda v: str(v).replace(" ", ""))
def test_every_hazard_frame_comes_back_as_planted(name, points, cplx, bflib):
    values = planted_ref.hazard(name, points, cplx)
    frame, _ = push(values)
    parts = frame.view(np.float32)
    assert frame.shape == points[::-1] and not (np.signbit(parts) & (parts == 0)).any()
    # the subnormals and the largest floats are in the frame, not flushed and not saturated
    if name == "specials":
        assert (np.abs(parts) == planted.SUB_MIN).any() and (np.abs(parts) == planted.SUB_MAX).any() and (np.abs(parts) == planted.FLT_MAX).any()
    if name == "radix":
        assert (np.abs(parts).view(np.uint32) == planted.RADIX_LOWEST).sum() == 1


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("K", [3, 6])
@pytest.mark.parametrize("points", [PLANE, VOLUME])
def test_a_burst_plants_every_frame_in_its_own_slot(points, K, cplx, bflib):
    """K = 3: the per-frame route; K = 6 on the plane: das_burst.hip, a thread applying a term's geometry to four frames (the volume's
    family has no burst kernel: its six frames run one by one)"""
    stack = planted.integers(K, points, cplx=cplx)
    route = bflib.describe_burst(planted.block(stack[0]).bp, K)
    assert int(route.burst_kernel) == (1 if K == 6 and points == PLANE else 0), route.reason
    frames, ids = burst(stack)
    info = bflib.last_burst_info()
    assert (int(info.first_frame_id), int(info.frame_count), int(info.route.burst_kernel)) == (ids[0], K, int(route.burst_kernel))
    # no two frames are equal, so a frame in another frame's slot cannot pass above
    assert all(not np.array_equal(frames[a], frames[b]) for a in range(K) for b in range(a + 1, K))
    for k in range(K):
        assert np.array_equal(bflib.copy_frame(ids[k]).view(np.uint32), frames[k].view(np.uint32))


# ----------------------------------------------------------------------------- score

@pytest.mark.parametrize("name,points,cplx", HAZARDS, ids=IDS)
def test_score(name, points, cplx, bflib):
    values, plan = make(name, points, cplx)
    frame, _ = push(values)
    present(frame, plan)
    boxes = [None, cut(points), inner(points)]
    if name == "plateaus":
        # ... and a box that holds only the second of the two voxels tied for max_abs
        tie = plan["largest"][1]
        first = (tie[0], tie[1] // 2, tie[2] // 2)
        boxes.append((first, tuple(n - f for n, f in zip(points, first))))
    for box in boxes:
        rows, _ = bflib.score_last_frames(1, region_of(box))
        ring_frames.check_row(rows[0], frame, box, what=f"{name} {points} box {box}")
        owed = planted.box_numbers(plan, box)
        assert (int(rows[0].non_finite), [int(n) for n in rows[0].gradient_pairs]) == (owed["non_finite"], owed["gradient_pairs"])
        if owed["max_index"] is not None:
            assert tuple(int(v) for v in rows[0].max_index) == owed["max_index"]
    whole = planted.box_numbers(plan)
    assert whole["max_index"] is not None and (name != "plateaus" or planted.box_numbers(plan, boxes[3])["max_index"] == plan["largest"][1])
    assert name == "plateaus" or 0 < planted.box_numbers(plan, boxes[2])["non_finite"] < whole["non_finite"]


# ----------------------------------------------------------------------------- find_peaks

def indices(row, peaks):
    return [tuple(int(v) for v in i) for i in ring_frames.peak_records(row, peaks)["index"]]


@pytest.mark.parametrize("name,points,cplx", HAZARDS, ids=IDS)
def test_find_peaks(name, points, cplx, bflib):
    values, plan = make(name, points, cplx)
    frame, _ = push(values)
    present(frame, plan)
    q = frame_peaks_ref.decision(frame)
    for threshold in (0.0, HEIGHT if name == "plateaus" else 1.0):
        rows, peaks, found = ring_frames.check_peaks([frame], threshold, what=f"{name} {points} at {threshold}")
        whole = indices(rows[0], peaks)
        assert found[0]["found"] == len(whole) >= 2
        if name == "plateaus" and threshold:
            # eligible at equality: t == q on the real frame, fl(t * t) == q on the complex one
            level = frame_peaks_ref.level(frame, threshold)
            assert int((q == level).sum()) >= sum(len(v) for k, v in plan["plateaus"].items() if k not in ("rounding", "collision")) - 1
            assert whole == plan["peaks"]
            records = ring_frames.peak_records(rows[0], peaks)
            for (position, axis), (offset, fitted) in plan["offsets"].items():
                record = records[whole.index(position)]
                assert bool(record["fitted"] >> axis & 1) == fitted, (position, axis)
                assert record["offset"][axis] == offset and np.signbit(record["offset"][axis]) == np.signbit(np.float32(offset)), (position, axis)
        # tiled into boxes: the tiles' lists concatenate to the whole frame's -- no peak invented at a face, none doubled
        tiled = []
        for box in halves(points):
            rows, peaks, _ = ring_frames.check_peaks([frame], threshold, box=box, what=f"{name} {points} at {threshold}, tile {box}")
            tiled += indices(rows[0], peaks)
        assert sorted(tiled, key=lambda p: planted._flat(points, p)) == whole


# ----------------------------------------------------------------------------- quantiles

def test_quantiles_of_the_radix_frame(bflib):
    values, plan = planted.radix()
    frame, _ = push(values)
    bits, non_finite = frame_quantiles_ref.finite_bits(frame)
    assert non_finite == 0 and np.array_equal(np.sort(bits), plan["keys"])             # every planted key is in the downloaded frame
    keys = []
    for fractions in plan["fractions"]:
        want = ring_frames.ranked([frame], fractions, histograms=True)[0]
        keys += [q["value_bits"] for q in want["rows"]]
        assert [q["rank"] for q in want["rows"]] == plan["ranks"][len(keys) - len(fractions):len(keys)]
        ring_frames.ranked([frame], fractions, histograms=False)
        for box in (ring_frames.BOX, cut(VOLUME)):
            ring_frames.ranked([frame], fractions, box, histograms=True)
            ring_frames.ranked([frame], fractions, box, histograms=False)
    assert keys == [int(plan["keys"][r]) for r in plan["ranks"]]
    first, last = plan["tie"]
    assert keys[plan["ranks"].index(first)] == keys[plan["ranks"].index(last)] == planted.RADIX_TIE
    assert keys[0] == planted.RADIX_LOWEST and keys[-1] == planted.RADIX_HIGHEST


@pytest.mark.parametrize("name,points,cplx", HAZARDS[:6], ids=IDS[:6])
def test_quantiles_leave_out_the_non_finite_voxels_and_the_zeros_are_the_lowest_plateau(name, points, cplx, bflib):
    values, plan = make(name, points, cplx)
    frame, _ = push(values)
    present(frame, plan)
    zeros = len(plan["zero"])
    fractions = [0.0, 1.0, 0.5, (zeros - 1) / (frame.size - len(plan["non_finite"]) - 1), zeros / (frame.size - len(plan["non_finite"]) - 1)]
    for box in (None, cut(points)):
        for histograms in (True, False):
            want = ring_frames.ranked([frame], fractions, box, histograms=histograms)[0]
        assert want["non_finite"] == planted.box_numbers(plan, box)["non_finite"]
        assert np.isfinite([q["value"] for q in want["rows"]]).all()
    # (the whole frame) rank 0 and the last rank of the plateau of zeros hold 0, the rank behind it the smallest q above 0
    rows = ring_frames.ranked([frame], fractions)[0]["rows"]
    assert [(r["rank"], r["value_bits"], r["below"], r["equal"]) for r in (rows[0], rows[3])] == [(0, 0, 0, zeros), (zeros - 1, 0, 0, zeros)]
    assert rows[4]["rank"] == rows[4]["below"] == zeros and 0 < rows[4]["value"] < planted.FLT_MIN


# ----------------------------------------------------------------------------- accumulate_peaks and pair_peaks

@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("points", [PLANE, VOLUME])
def test_plateaus_moved_by_a_known_shift_deposit_and_pair(points, cplx, bflib):
    values, plan = planted.plateaus(points, cplx=cplx)
    frames, ids = zip(push(values), push(planted.moved(values, SHIFT)))
    frames = list(frames)
    assert frame_peaks_ref.peaks(frames[0], HEIGHT)["found"] == len(plan["peaks"]) >= 12
    acq = planted.block(values)
    lo, hi = planted.extent(points)
    # deposits: the frames' own grid (an offset of +-0.5 is a bin boundary there) and a grid four times finer
    for grid in (ring_frames.map_view(points, lo, hi), ring_frames.map_view(ring_frames.finer(points), lo, hi)):
        A = ring_frames.placement_onto(grid, acq.bp.das_voxel_transform, points)
        for use_offsets in (True, False):
            counts, rows, info = ring_frames.run_localise(grid, frames, HEIGHT, A, use_offsets)
            if cplx:
                expected, numbers = ring_frames.binned_records(grid.output_points, 2, HEIGHT, A, use_offsets)
            else:
                expected, numbers = localisation_ref.accumulate(grid.output_points, frames, HEIGHT, A, use_offsets)
            ring_frames.same_localise(counts, expected)
            ring_frames.check_rows(rows, numbers, frames, HEIGHT)
            assert [n["found"] for n in numbers] == [len(plan["peaks"]), len(plan["peaks"]) - 1] and int(counts.sum()) == int(info.deposited)

    # pairs: x stretched by 3 and z by 2, so that the shift (1, 0, 2) is the displacement (3, 0, 4) of length 5 exactly
    S = np.array([[3.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 2.0, 0]])
    field = (3 * points[0], points[1], 2 * points[2])

    def reference(reach, use_offsets, counts=None, sums=None):
        if cplx:
            return tracks_ref.pair_records(ring_frames.peak_lists(2, HEIGHT), S, reach, use_offsets, counts, sums)
        return tracks_ref.pair_frames(frames, HEIGHT, S, reach, ring_frames.CAP, use_offsets, counts=counts, sums=sums)
    for use_offsets in (False, True):
        bflib.track_map_reset(field)
        rows, got = ring_frames.pair(2, HEIGHT, S, 5.0, use_offsets=use_offsets, deposit=True)
        counts, sums = tracks_ref.empty_map(field)
        want, numbers = reference(5.0, use_offsets, counts, sums)
        ring_frames.same_pairs_call(rows, got, want, numbers, 2, HEIGHT)
        ring_frames.same_map(field, counts, sums)
        if not use_offsets:
            # every pair is a peak and its image: the displacement is exactly the shift, its distance^2 == reach^2 -- and pairs
            # with every peak of the second frame; the peak of the plateau that left the frame is the one without a partner
            assert len(got) >= 8 and (got["displacement"] == [3.0, 0.0, 4.0]).all() and (got["distance2"] == 25.0).all()
            assert numbers[0]["unpaired"] == [1, 0] and numbers[0]["pairs"] == len(plan["peaks"]) - 1
    # one ulp below the distance: nothing is within reach
    below = float(np.nextafter(np.float32(5.0), np.float32(0.0)))
    rows, got = ring_frames.pair(2, HEIGHT, S, below, use_offsets=False)
    want, numbers = reference(below, False)
    ring_frames.same_pairs_call(rows, got, want, numbers, 2, HEIGHT)
    assert len(got) == 0 and numbers[0]["pairs"] == 0


# ----------------------------------------------------------------------------- gram, mix, autocorrelate, convolve, correlate

def same_values(got, want):
    """equal float for float (an int64 result has no -0: by value)"""
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want)


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("K", [3, 17])
@pytest.mark.parametrize("points", [PLANE, VOLUME])
def test_integer_frames_give_the_int64_results(points, K, cplx, bflib):
    which = grid_name(points, cplx)
    stack = planted.integers(K, points, cplx=cplx)
    frames, ids = burst(stack)
    assert np.abs(frames.view(np.float32)).max() == 64 and (frames.view(np.float32) == np.rint(frames.view(np.float32))).all()
    # gram: the whole frame, and a box
    G, _ = ring_frames.check_gram(frames, ids, what=which)
    assert np.array_equal(G, planted_ref.gram_int64(frames).astype(np.complex128))
    box = cut(points)
    G, _ = ring_frames.check_gram(frames, ids, box, what=which + " box")
    (x0, y0, z0), (nx, ny, nz) = box
    assert np.array_equal(G, planted_ref.gram_int64(frames[:, z0:z0 + nz, y0:y0 + ny, x0:x0 + nx]).astype(np.complex128))
    # mix: K -> 3
    W = planted_ref.integer_weights(3, K, cplx)
    out, _ = ring_frames.check_mix(which, frames, ids, W, what=which)
    mixed = planted_ref.mix_int64(frames, W)
    assert same_values(out, planted_ref.to_kind(*mixed, cplx, frames.dtype))
    # autocorrelate: the identity form, and -- K == 3 -- behind the mix's weights
    for weights in ([None, W] if K == 3 else [None]):
        frames, ids = burst(stack)
        out, _ = ring_frames.check_autocorr(which, frames, ids, weights, 3, what=which)
        re, im = planted_ref.autocorr_int64(*(planted_ref.exact(frames) if weights is None else mixed), 3)
        im[0] = 0
        assert same_values(out, planted_ref.to_kind(re, im, cplx, frames.dtype))
    # convolve: integer taps, ZERO mode
    taps = (planted_ref.TAPS[0], None if points[1] == 1 else planted_ref.TAPS[1], planted_ref.TAPS[2])
    frames, ids = burst(stack)
    out, _ = ring_frames.check_convolve(which, frames, ids, taps, what=which)
    for k in range(K):
        assert same_values(out[k], planted_ref.to_kind(*planted_ref.convolve_int64(frames[k], taps), cplx, frames.dtype)), k
    # correlate: the three newest frames against the middle one
    frames, ids = burst(stack)
    window = (1, 0 if points[1] == 1 else 1, 2)
    table, _, _ = ring_frames.check_correlate(frames[K - 3:], ids[K - 3:], 1, window, what=which)
    want = planted_ref.correlate_int64(frames[K - 3:], 1, window)
    for n, name in enumerate(("re", "im", "energy_reference", "energy_frame", "terms")):
        assert np.array_equal(table[0][name], want[n].astype(table[name].dtype)), name


SPECIAL_WEIGHTS = np.array([[1, -1, 1], [0, 1, 0], [-1, 1, 1]], np.complex64)
SPECIAL_TAPS = (np.array([1, -1, 1], np.float32), np.array([-1, 1, 1], np.float32), np.array([1, 1, -1], np.float32))


@pytest.mark.parametrize("points", [PLANE, VOLUME])
def test_the_same_calls_on_frames_that_hold_the_special_voxels(points, bflib):
    """three real `specials` frames, the special voxels at the same places in each, the noise around them its own.  Weights and taps
    are 0 and +-1, so that no product rounds: what is compared is what an inf, a NaN, FLT_MAX and a subnormal DO in each call."""
    which = grid_name(points, False)
    made = [planted.specials(points, seed) for seed in range(3)]
    stack, plan = [m[0] for m in made], made[0][1]
    frames, ids = burst(stack)
    for frame in frames:
        present(frame, plan)
    holes = len(plan["non_finite"])
    # GRAM: "a voxel that is not finite in some frame counts in non_finite and in no entry"; the squares of FLT_MAX and of the
    # subnormals are doubles ("Each float is widened to double")
    for box in (None, cut(points)):
        G, _ = ring_frames.check_gram(frames, ids, box, what=which)
        assert np.isfinite(G.real).all() and G.real.max() >= float(planted.FLT_MAX) ** 2
    _, info, _ = bflib.gram_last_frames(3)
    assert (int(info.non_finite), int(info.voxels)) == (holes, frames[0].size - holes)
    # MIX: "no weight is skipped for being zero, so a voxel that is not finite in some frame is not finite in every output (plain
    # IEEE)": row 1 copies frame 1 but for 0 * inf and 0 * NaN; FLT_MAX - FLT_MAX + FLT_MAX stays FLT_MAX, the subnormals stay exact
    out, _ = ring_frames.check_mix(which, frames, ids, SPECIAL_WEIGHTS, what=which)
    finite = np.isfinite(frames).all(axis=0)
    assert np.array_equal(out[1][finite].view(np.uint32), frames[1][finite].view(np.uint32)) and np.isnan(out[1][~finite]).all()
    assert int((~finite).sum()) == holes and (np.abs(out[0][finite]) == planted.FLT_MAX).any() and (np.abs(out[0]) == planted.SUB_MIN).any()
    # AUTOCORRELATE: "ONE float32 fmaf chain ... Plain IEEE otherwise": FLT_MAX * FLT_MAX is +inf although every source is finite
    # there, and the product of two subnormals is 0
    frames, ids = burst(stack)
    out, _ = ring_frames.check_autocorr(which, frames, ids, None, 2, what=which)
    big = [p for p in plan["largest"]]
    assert all(np.isposinf(at(out[0], p)) for p in big) and all(at(out[0], p) == 0 for p in plan["subnormal"])
    # CONVOLVE, Zero mode: "a voxel that is not finite makes every output whose support covers it not finite, as the mix does"
    taps = (SPECIAL_TAPS[0], None if points[1] == 1 else SPECIAL_TAPS[1], SPECIAL_TAPS[2])
    frames, ids = burst(stack)
    out, _ = ring_frames.check_convolve(which, frames, ids, taps, what=which)
    assert all(not np.isfinite(at(out[0], p)) for p in plan["non_finite"]) and np.isfinite(out[0]).sum() > out[0].size // 2
    # ... Normalised mode: "the terms of the non-finite source voxels SKIPPED": the holes are filled
    frames, ids = burst(stack)
    positive = tuple(None if h is None else np.abs(h) for h in taps)
    out, _ = ring_frames.check_convolve(which, frames, ids, positive, mode=ring_frames.NORMALISED, what=which + " normalised")
    # CORRELATE: "ref[v] finite and f_k[v + s] finite": the terms leave the holes out, the sums are the Gram matrix's doubles
    frames, ids = burst(stack)
    window = (1, 0 if points[1] == 1 else 1, 1)
    table, expected, _ = ring_frames.check_correlate(frames, ids, 1, window, [((0, 0, 0), points), cut(points)], what=which)
    centre = (0, 1, window[2], window[1], window[0])
    assert int(table["terms"][centre]) == frames[0].size - holes and table["re"][centre] == table["energy_reference"][centre] > float(planted.FLT_MAX) ** 2


# ----------------------------------------------------------------------------- warp

def support_is_finite(frame, shift, reach):
    """per voxel v: every source voxel within `reach` = (below, above) of v + shift along every axis of more than one point lies in
    the frame and is finite"""
    finite = np.isfinite(frame.real) & np.isfinite(frame.imag) if np.iscomplexobj(frame) else np.isfinite(frame)
    padded = np.pad(finite, [(8, 8)] * 3, constant_values=False)
    out = np.ones(frame.shape, bool)
    Z, Y, X = frame.shape
    spans = [range(-reach[0], reach[1] + 1) if n > 1 else range(1) for n in (X, Y, Z)]
    for dz in spans[2]:
        for dy in spans[1]:
            for dx in spans[0]:
                x, y, z = 8 + shift[0] + dx, 8 + (shift[1] + dy if Y > 1 else 0), 8 + shift[2] + dz
                out &= padded[z:z + Z, y:y + Y, x:x + X]
    return out


@pytest.mark.parametrize("name,points,cplx", [h for h in HAZARDS if h[0] != "squares" and h[1] != WAVE], ids=[i for i, h in zip(IDS, HAZARDS) if h[0] != "squares" and h[1] != WAVE])
def test_warp_by_a_zero_field_and_by_an_integer_shift(name, points, cplx, bflib):
    """"a source voxel under the support that is not finite makes the output not finite, no weight is skipped for being zero": where
    the support holds none, the weights are 1 and 0 and the chains return the source's bits, subnormals and FLT_MAX included"""
    which = grid_name(points, cplx)
    stack = [make(name, points, cplx, seed)[0] for seed in (0, 1)]
    plan = make(name, points, cplx)[1]
    for shift in ((0, 0, 0), (2, 0 if points[1] == 1 else -1, -3)):
        for interpolation in (ring_frames.LINEAR, ring_frames.CUBIC):
            frames, ids = burst(stack)
            present(frames[0], plan)
            case = dict(field=np.array([shift, [-s for s in shift]], np.float32).reshape(2, 1, 1, 1, 3), nodes=(1, 1, 1), node_first=(0, 0, 0), node_step=(1, 1, 1))
            out, _, _, _ = ring_frames.check_warp(which, frames, ids, case, None, interpolation, ring_frames.WARP_ZERO, what=f"{name} {points} moved by {shift}", same_masks=True)
            reach = (0, 1) if interpolation == ring_frames.LINEAR else (1, 2)
            for n, sign in ((0, 1), (1, -1)):
                d = tuple(sign * s for s in shift)
                clean = support_is_finite(frames[n], d, reach)
                # out[v] = frame[v + d]: move the frame by -d (what moves in is never compared: its support is not in the frame)
                Z, Y, X = frames[n].shape
                moved = np.full(frames[n].shape, np.nan, frames[n].dtype)
                zs, ys, xs = (slice(max(0, -s), min(m, m - s)) for s, m in ((d[2], Z), (d[1], Y), (d[0], X)))
                zt, yt, xt = (slice(max(0, s), min(m, m + s)) for s, m in ((d[2], Z), (d[1], Y), (d[0], X)))
                moved[zs, ys, xs] = frames[n][zt, yt, xt]
                assert clean.sum() > frames[n].size // 3 and not np.isnan(moved[clean].view(np.float32)).any()
                assert np.array_equal(out[n][clean].view(np.uint32), moved[clean].view(np.uint32)), (shift, interpolation, n)
