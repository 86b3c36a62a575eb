"""The calls on frames already in the ring, one after the other in one process: what they share on the device -- the scratch and the
pinned block that score, quantiles, find_peaks, gram, gram_boxes, correlate, accumulate_peaks, pair_peaks, track_peaks and draw_tracks
carve their tables from, the scratch the last three size by the peaks they find, the table of the queued runs, the two deposit maps --
has to grow from one call to the next and come back after a shutdown, which no test of one operation notices.

Every result is judged by the test of its own operation: its reference, its comparator and its bars are imported from there, and
nothing here restates them."""
import ctypes as C

import numpy as np
import pytest

from ogl_beamforming_amd import lib as bf
from ogl_beamforming_amd import params as P
from tests import localisation_ref
from tests import ring_frames
from tests import track_chains_ref, track_draw_ref, tracks_ref
from tests import variants_cases as vc
from tests.frame_info import newest_info
from tests.ring_frames import region_of
from tests.scaffold import automatic_path  # noqa: F401

pytestmark = pytest.mark.gpu
E = P.LibError
K = 4
# two complex planes through the ensemble tests' own block and burst (their GRIDS, by names of this file's): the tables of the second
# are larger than everything the first left allocated
ring_frames.GRIDS.update(frame_ops_small=((16, 1, 8), vc.LO, vc.HI, True), frame_ops_large=((64, 1, 32), vc.LO, vc.HI, True))
MAP_POINTS = (8, 1, 8)
REGIONS = [((1, 0, 1), (13, 1, 5)), ((3, 0, 3), (13, 1, 5))]        # two boxes for correlate, the second against the small frame's far corner
SCORE_BOX = ((5, 0, 3), (3, 1, 2))
REACH = 3.0                                                         # map voxels: a voxel and a half of the small frames along z
BOTH = track_chains_ref.POINTS | track_chains_ref.LINKS


@pytest.fixture(autouse=True)
def maps_reset(automatic_path, bflib):
    yield
    bflib.localisation_map_reset(None)
    bflib.track_map_reset(None)


def map_of(which):
    """the 8 x 1 x 8 map over the frames' own box, and the placement of the frames of `which` onto it"""
    acq = ring_frames.block(which)
    grid = ring_frames.map_view(MAP_POINTS, vc.LO, vc.HI)
    return grid, ring_frames.placement_onto(grid, acq.bp.das_voxel_transform, ring_frames.GRIDS[which][0])


def the_newer_calls(which, frames, thresholds, A):
    """quantiles, gram_boxes, pair_peaks, track_peaks and draw_tracks on the K newest frames, each judged as its own test judges it, the
    three that deposit on fresh maps of MAP_POINTS; returns every call's bytes, and both maps as the draw call leaves them"""
    out = {}
    # quantiles: its own check, then the call's bytes
    ring_frames.ranked(list(frames), ring_frames.FRACTIONS)
    rows, records, tables, _ = bf.quantiles_last_frames(K, ring_frames.FRACTIONS, histograms=True)
    out["quantiles"] = bytes(rows), bytes(records), tables.tobytes()
    # gram_boxes, two boxes, against gram one box at a time
    want = ring_frames.singles(K, REGIONS)
    grams, infos, _ = bf.gram_boxes_last_frames(K, [region_of(box) for box in REGIONS])
    ring_frames.same_as_singles(grams, infos, want, which)
    out["gram_boxes"] = grams.tobytes(), [bytes(i) for i in infos]
    # pair_peaks, depositing
    records = ring_frames.peak_lists(K, thresholds)
    bf.track_map_reset(MAP_POINTS)
    rows, pairs = ring_frames.pair(K, thresholds, A, REACH, deposit=True)
    counts, sums = tracks_ref.empty_map(MAP_POINTS)
    want, numbers = tracks_ref.pair_records(records, A, REACH, counts=counts, sums=sums)
    ring_frames.same_pairs_call(rows, pairs, want, numbers, K, thresholds)
    ring_frames.same_map(MAP_POINTS, counts, sums)
    assert sum(w["pairs"] for w in numbers) >= 1
    out["pairs"] = bytes(rows), pairs.tobytes()
    # track_peaks, min_length 2, both deposits; then without records: the same rows, the maps once more
    density, counts, sums = ring_frames.fresh_maps(MAP_POINTS)
    got = ring_frames.track(K, thresholds, A, REACH, 2, deposit=BOTH)
    want = track_chains_ref.chain_records(records, A, REACH, 2, True, deposit=BOTH, point_map=density, counts=counts, sums=sums)
    ring_frames.same_tracks_call(got, want, K, thresholds)
    ring_frames.same_maps(MAP_POINTS, density, counts, sums)
    assert len(want["tracks"]) >= 1
    rows, none, nothing, _ = bf.track_peaks_last_frames(K, thresholds, A, REACH, ring_frames.CAP, 2, deposit=BOTH, records=False)
    assert bytes(rows) == bytes(got[0]) and len(none) == 0 and len(nothing) == 0
    ring_frames.same_maps(MAP_POINTS, 2 * density, 2 * counts, 2 * sums)
    out["tracks"] = [bytes(v) for v in got]
    # draw_tracks, smooth 1, both deposits; track_map_copy beside localisation_map_copy
    density, counts, sums = ring_frames.fresh_point_and_track_maps(MAP_POINTS, MAP_POINTS)
    rows = ring_frames.draw(K, thresholds, A, REACH, 2, 1, deposit=BOTH)
    want = track_draw_ref.draw_records(records, A, REACH, 2, 1, True, deposit=BOTH, point_map=density, counts=counts, sums=sums)
    ring_frames.same_rows(rows, want, K, thresholds)
    point_info, link_info = ring_frames.same_point_and_track_maps(MAP_POINTS, MAP_POINTS, density, counts, sums)
    ring_frames.same_infos(point_info, link_info, 1, want["rows"], BOTH)
    out["drawn"] = bytes(rows)
    out["maps"] = bf.localisation_map_copy(MAP_POINTS)[0].tobytes(), *(v.tobytes() for v in bf.track_map_copy(MAP_POINTS)[:2])
    return out


def the_order(which):
    """the calls on the K newest frames, each judged as its own test judges it; returns what a later run can be compared with"""
    frames, ids = ring_frames.ensemble(which, K)
    assert frames.shape[1:] == ring_frames.GRIDS[which][0][::-1] and np.iscomplexobj(frames)
    thresholds = ring_frames.fraction_of_max(frames, 0.25)
    grid, A = map_of(which)
    # 1. score, whole frames
    scored, _ = bf.score_last_frames(K)
    for k in range(K):
        ring_frames.check_row(scored[k], frames[k], what=f"{which} {k}")
    # 2. find_peaks
    peak_rows, peaks, found = ring_frames.check_peaks(list(frames), thresholds, what=which)
    assert all(r["found"] >= 2 for r in found)
    # 3. gram
    G, _ = ring_frames.check_gram(frames, ids, what=which)
    # 4. correlate, two regions, window (1, 0, 1)
    table, _, _ = ring_frames.check_correlate(frames, ids, K // 2, (1, 0, 1), REGIONS, what=which)
    # 5. accumulate_peaks into the map
    counts, deposits, info = ring_frames.run_localise(grid, frames, thresholds, A)
    expected, numbers = localisation_ref.accumulate(grid.output_points, frames, thresholds, A)
    ring_frames.same_localise(counts, expected)
    assert (info.calls, int(info.deposited)) == (1, sum(n["found"] for n in numbers)) and int(counts.sum()) == int(info.deposited) >= K
    # 6. score again, a 3 x 1 x 2 region
    boxed, _ = bf.score_last_frames(K, region_of(SCORE_BOX))
    for k in range(K):
        ring_frames.check_row(boxed[k], frames[k], SCORE_BOX, what=f"{which} {k} box")
        assert (boxed[k].frame_id, boxed[k].parameter_block, boxed[k].data_kind, tuple(boxed[k].points)) == \
               (scored[k].frame_id, scored[k].parameter_block, scored[k].data_kind, tuple(scored[k].points))
    # 7. find_peaks again: the bytes of 2.
    again_rows, again_peaks, _ = ring_frames.check_peaks(list(frames), thresholds, what=which + " again")
    assert bytes(again_rows) == bytes(peak_rows) and bytes(again_peaks) == bytes(peaks)
    # (the deposit rows last: their check asks find_peaks once more)
    ring_frames.check_rows(deposits, numbers, frames, thresholds)
    # 8. the newer calls, and at the end of the walk each of them again: the bytes of its first run
    newer = the_newer_calls(which, frames, thresholds, A)
    assert the_newer_calls(which, frames, thresholds, A) == newer
    return dict(frames=frames, scored=scored, peak_rows=peak_rows, peaks=peaks, gram=G, table=table, counts=counts, newer=newer)


def numbers_of(row):
    """a HipFrameMetrics row without the frame's id: what depends on the frame's voxels and the box alone"""
    raw = bytearray(bytes(row))
    offset = P.HipFrameMetrics.frame_id.offset
    raw[offset:offset + 4] = b"\0\0\0\0"
    return bytes(raw)


def test_the_scratch_grows_from_small_frames_to_large_ones_and_every_call_finds_its_tables(bflib):
    small = the_order("frame_ops_small")
    large = the_order("frame_ops_large")
    assert large["frames"].nbytes == 16 * small["frames"].nbytes
    # ... and back: the small frames again, in memory the large ones left behind -- every byte as the first time
    again = the_order("frame_ops_small")
    assert np.array_equal(again["frames"].view(np.uint32), small["frames"].view(np.uint32))
    assert [numbers_of(r) for r in again["scored"]] == [numbers_of(r) for r in small["scored"]]
    assert bytes(again["peaks"]) == bytes(small["peaks"]) and again["gram"].tobytes() == small["gram"].tobytes()
    assert again["table"].tobytes() == small["table"].tobytes() and again["counts"].tobytes() == small["counts"].tobytes()
    # the rows carry the frames' ids; the pair, track and point records and both maps do not: byte for byte
    first, second = small["newer"], again["newer"]
    assert second["pairs"][1] == first["pairs"][1] and second["tracks"][1:] == first["tracks"][1:] and second["maps"] == first["maps"]

def mix_and_score(which, frames, ids):
    """two mixes of the K newest frames queued behind them (the ensemble tests' check), then their metrics rows"""
    out, first = ring_frames.check_mix(which, frames, ids, ring_frames.weights(2, K, 7901), tag=3, what=which)
    rows, _ = bf.score_last_frames(2)
    for j in range(2):
        ring_frames.check_row(rows[j], out[j], what=f"{which} mix {j}")
        assert (int(rows[j].frame_id), int(rows[j].image_plane_tag)) == (first + j, 3)
    return out, first, rows


def test_queued_runs_behind_reduce_calls(bflib):
    which = "frame_ops_small"
    acq = ring_frames.block(which)
    frames, ids = ring_frames.ensemble(which, K)
    before = bytes(bf.last_burst_info())
    grid, A = map_of(which)
    counts, _, _ = ring_frames.run_localise(grid, frames, ring_frames.fraction_of_max(frames, 0.25), A)
    assert len(np.unique(counts)) >= 2
    out, first, _ = mix_and_score(which, frames, ids)
    scale = 0.37
    frame_id, ms = bf.queue_localisation_map(scale, tag=5)
    assert ms > 0
    # get_last_frames serves the map frame: a block of the map's grid says its shape
    bp = type(acq.bp).from_buffer_copy(acq.bp)
    bp.output_points[:3] = list(MAP_POINTS)
    queued = bf.get_last_frames(bp, 1)[0]
    expected = localisation_ref.queued_frame(counts, scale)
    assert queued.dtype == np.float32 and np.array_equal(queued.view(np.uint32), expected.view(np.uint32))
    # consecutive ids: the burst's, the two mixes, the map
    assert [first, first + 1, frame_id] == [ids[-1] + 1, ids[-1] + 2, ids[-1] + 3] and int(newest_info(bf.library()).frame_id) == frame_id
    info = bf.frame_info(frame_id)
    assert tuple(info.points) == MAP_POINTS and info.data_kind == int(P.DataKind.Float32)
    # the mixes are still served by their ids, and the burst is still the newest multi-frame push, its info as it was
    assert np.array_equal(bf.copy_frame(first + 1).view(np.uint32), out[1].view(np.uint32))
    assert bytes(bf.last_burst_info()) == before
    ring_frames.same_localise(bf.localisation_map_copy()[0], counts)


def test_a_shutdown_releases_everything_and_the_calls_start_again(bflib):
    L = bflib.library()
    which = "frame_ops_small"
    frames, ids = ring_frames.ensemble(which, K)
    grid, A = map_of(which)
    ring_frames.run_localise(grid, frames, ring_frames.fraction_of_max(frames, 0.25), A)
    scored, _ = bf.score_last_frames(K)
    out, _, mixed_rows = mix_and_score(which, frames, ids)
    bf.track_map_reset(MAP_POINTS)
    assert tuple(bf.track_map_copy(MAP_POINTS)[2].points) == MAP_POINTS              # the track map exists

    L.beamformer_hip_shutdown()
    counts, info = np.full(int(np.prod(MAP_POINTS)), 0xA5A5A5A5, np.uint32), P.HipMapInfo()
    sums, track_info = np.full(3 * counts.size, 0x5A, np.int64), P.HipTrackMapInfo()

    def no_map():
        assert not L.beamformer_hip_localisation_map_copy(counts.ctypes.data_as(C.POINTER(C.c_uint32)), counts.size, C.byref(info))
        assert bf.last_error()[0] == E.InvalidAccess and (counts == 0xA5A5A5A5).all() and not bytes(info).strip(b"\0")
        assert not L.beamformer_hip_track_map_copy(counts.ctypes.data_as(C.POINTER(C.c_uint32)), sums.ctypes.data_as(C.POINTER(C.c_int64)), counts.size,
                                                   C.byref(track_info))
        assert bf.last_error()[0] == E.InvalidAccess and (counts == 0xA5A5A5A5).all() and (sums == 0x5A).all() and not bytes(track_info).strip(b"\0")

    no_map()
    assert L.beamformer_hip_set_devices((C.c_int32 * 1)(0), 1)
    frames2, ids2 = ring_frames.ensemble(which, K)
    assert ids2 == list(range(K)) and np.array_equal(frames2.view(np.uint32), frames.view(np.uint32))
    no_map()                                            # a device again, but the map went with the old one
    scored2, _ = bf.score_last_frames(K)
    for k in range(K):
        ring_frames.check_row(scored2[k], frames2[k], what=f"after the shutdown {k}")
    assert [numbers_of(r) for r in scored2] == [numbers_of(r) for r in scored]
    out2, first2, mixed_rows2 = mix_and_score(which, frames2, ids2)
    assert first2 == K and out2.tobytes() == out.tobytes() and [numbers_of(r) for r in mixed_rows2] == [numbers_of(r) for r in mixed_rows]
    no_map()
    # until a reset: an empty map, nothing counted
    bf.localisation_map_reset(MAP_POINTS)
    empty, info = bf.localisation_map_copy(MAP_POINTS)
    assert not empty.any() and (info.calls, int(info.deposited), int(info.outside)) == (0, 0, 0)
    bf.track_map_reset(MAP_POINTS)
    empty, no_sums, track_info = bf.track_map_copy(MAP_POINTS)
    assert not empty.any() and not no_sums.any()
    assert (track_info.calls, int(track_info.pairs), int(track_info.deposited), int(track_info.outside)) == (0, 0, 0, 0)
