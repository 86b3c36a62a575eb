"""The host side of the drawn tracks (beamformer_hip_draw_tracks_last_frames, include/ogl_beamformer_hip.h): the numpy reference
(tests/track_draw_ref.py) against an independent scalar restatement -- Python floats, one sample at a time --, the properties its bins
owe, the row's layout, the refusals that are decided before any device state is looked at, and the planted plans of
tests/test_gpu_track_draw.py, checked here for what they claim.  No device is needed.  Every comparison is of integers or bit
patterns."""
import ctypes as C
import math
import os
import struct
import subprocess

import numpy as np

from ogl_beamforming_amd import lib as bf
from ogl_beamforming_amd import params as P
from tests import planted, tracks_ref
from tests import track_plans
from tests import track_chains_ref as chains
from tests import track_draw_ref as ref
from tests.track_plans import EQUALITY_BOX, FAR_AWAY, FAR_EDGE, OWN, PLANE_FIELD, WIDE, draw_plan, scaled, times

E = P.LibError
ROOT = track_plans.ROOT
IDENTITY, HEIGHT, LEVEL, REACH = track_plans.IDENTITY, track_plans.HEIGHT, track_plans.LEVEL, track_plans.REACH
POINTS, LINKS = ref.POINTS, ref.LINKS


# ----------------------------------------------------------------------------- the planted plans


def every_link(out):
    return [link for track in out["links"] for link in track]


def deposited(out_rows, kind):
    return sum(r[f"{kind}_deposited"] for r in out_rows), sum(r[f"{kind}_outside"] for r in out_rows)


def drawn_on(stack, placement, reach, min_length, w, point_field=None, track_field=None):
    """the reference on a planted stack with fresh maps: (out, density, counts, sums)"""
    coordinates = track_plans.coordinates_of(stack, placement)
    density = np.zeros(point_field[::-1], np.uint32) if point_field else None
    counts, sums = tracks_ref.empty_map(track_field) if track_field else (None, None)
    deposit = (POINTS if point_field else 0) | (LINKS if track_field else 0)
    out = ref.draw_positions(coordinates, reach, min_length, w, deposit=deposit, point_map=density, counts=counts, sums=sums)
    return out, density, counts, sums


def test_the_draw_plan_is_what_it_claims():
    stack, voxels = draw_plan()
    for k, where in voxels.items():
        assert frame_peaks(stack[k]) == len(where) - (1 if k == 1 else 0)               # the line of two voxels is one peak
    coordinates = track_plans.coordinates_of(stack, IDENTITY)
    everything = chains.chain_positions(coordinates, REACH, 1)
    assert sorted(everything["lengths"]) == [1, 2, 4, 6, 6, 6, 6]
    runs = [everything["points"]["position"][int(t["first"]):int(t["first"]) + int(t["length"])] for t in everything["tracks"]]
    moves = sorted({float(np.abs(q - p).max()) for run in runs for p, q in zip(run[:-1], run[1:])})
    assert moves == [0.0, 1.0, 1.5]

    # 48 x: S reaches 72, beyond a lane group of 16 and a wave of 64; both maps hold a corner
    name, A, reach, point_field, track_field = WIDE
    out, density, counts, sums = drawn_on(stack, A, reach, 1, 0, point_field, track_field)
    links = every_link(out)
    assert max(len(B) for skipped, d, B, drawn in links if not skipped) == 72 and not any(skipped for skipped, *_ in links)
    assert any(len(B) == 1 and not d.any() for skipped, d, B, drawn in links)          # the stationary link: e = 0, S = 1
    for kind in ("points", "links"):
        inside, outside = deposited(out["rows"], kind)
        assert inside >= 100 and outside >= 100
    assert int(density.sum()) == deposited(out["rows"], "points")[0] and int(counts.sum()) == deposited(out["rows"], "links")[0]

    # 4096 x: the links of 1.5 voxels have e = 6144 and are skipped, those of one voxel have e = 4096 exactly and draw 4096 samples
    name, A, reach, point_field, track_field = FAR_AWAY
    out, density, counts, sums = drawn_on(stack, A, reach, 1, 0, point_field, track_field)
    links = every_link(out)
    assert sorted(float(np.abs(d).max()) for skipped, d, B, drawn in links if skipped) == [6144.0, 6144.0]
    assert {float(np.abs(d).max()) for skipped, d, B, drawn in links if not skipped} == {0.0, 4096.0}
    total = ref.totals(out["rows"])
    assert total["links_skipped"] == 2 and total["samples"] > 4096 and not density.any() and not counts.any() and not sums.any()
    # ... and the skipped links WOULD have crossed the maps: drawn without the limit, 2 x 6144 samples fall into them
    head = A[:, :3] @ np.array([11.0, 0.0, 10.0]) + A[:, 3]
    assert tuple(head) == (2.0, 0.0, 0.0) and point_field[2] > 6144
    name, A, reach, point_field, track_field = FAR_EDGE
    out, density, counts, sums = drawn_on(stack, A, reach, 1, 0, point_field, track_field)
    assert ref.totals(out["rows"])["links_skipped"] == 2
    for kind in ("points", "links"):
        inside, outside = deposited(out["rows"], kind)
        assert inside >= 4096 and outside >= 4096

    # the plan of its own: repeats across link boundaries, a stationary bubble, negative coordinates, both maps cut
    name, A, reach, point_field, track_field = OWN
    for w in (0, 1):
        out, density, counts, sums = drawn_on(stack, A, reach, 1, w, point_field, track_field)
        across = [(n, i) for n, track in enumerate(out["links"]) for i, (skipped, d, B, drawn) in enumerate(track) if i and not skipped and not drawn[0]]
        moving = [(n, i) for n, i in across if out["links"][n][i][1].any()]
        assert len(across) >= 5 and (w or len(moving) >= 1)             # the stationary bubble's links, and (w = 0) the turn of A
        assert any((B < 0).any() for skipped, d, B, drawn in every_link(out))
        for kind in ("points", "links"):
            inside, outside = deposited(out["rows"], kind)
            assert inside >= 10 and outside >= 10
        assert ref.totals(out["rows"])["lone"] == 1


def frame_peaks(frame):
    from tests import frame_peaks_ref
    return frame_peaks_ref.peaks(frame, LEVEL)["found"]


def test_the_plane_plan_under_the_draw_calls_of_the_gpu_file():
    stack, _ = track_plans.plane_plan()
    field = times(PLANE_FIELD, 4)
    seen = set()
    for min_length in (1, 3, 12):
        for w in (0, 1, 3, 8):
            out, density, counts, sums = drawn_on(stack, scaled(4), 6.0, min_length, w, field, field)
            total = ref.totals(out["rows"])
            kept = [int(t["length"]) for t in out["tracks"]]
            assert total["lone"] == kept.count(1) and total["links_skipped"] == 0
            assert total["samples"] - total["repeats"] == sum(deposited(out["rows"], "points")) == sum(deposited(out["rows"], "links"))
            if min_length == 12:
                assert not kept and not any(total.values())
                continue
            assert deposited(out["rows"], "points")[1] >= 1 and deposited(out["rows"], "links")[1] >= 1 and total["repeats"] >= 1
            seen |= {(w, length, w >= length) for length in kept}
    # the window is clipped at both ends of every length from 2 to 11, and w = 8 exceeds the tracks of 2 to 8
    assert {length for w, length, _ in seen} == {1, 2, 3, 5, 6, 8, 9, 11} and all((8, length, True) in seen for length in (2, 3, 5, 6, 8))
    # maps of different sizes: a sample inside one and outside the other
    out, density, counts, sums = drawn_on(stack, scaled(4), 6.0, 1, 1, (40, 1, 160), field)
    assert deposited(out["rows"], "points")[0] < deposited(out["rows"], "links")[0]


def test_the_equality_frames_have_no_repeat_and_no_link_beyond_one_cell():
    """what the GPU file's equality with the track call stands on: the draw plan boxed to x >= 9, without offsets, under the identity"""
    stack, _ = draw_plan()
    found = [frame_peaks_boxed(f) for f in stack]
    coordinates = [tracks_ref.positions(r["index"], r["offset"], IDENTITY, use_offsets=False) for r in found]
    out = ref.draw_positions(coordinates, REACH, 1, 0)
    links = every_link(out)
    assert len(links) >= 8 and all(not skipped and len(B) == 1 and drawn.all() for skipped, d, B, drawn in links)
    assert ref.totals(out["rows"])["repeats"] == 0
    counts, sums = tracks_ref.empty_map(planted.PLANE)
    chains.chain_positions(coordinates, REACH, 1, LINKS, counts=counts, sums=sums)
    mine = tracks_ref.empty_map(planted.PLANE)
    ref.draw_positions(coordinates, REACH, 1, 0, deposit=LINKS, counts=mine[0], sums=mine[1])
    assert mine[0].tobytes() == counts.tobytes() and mine[1].tobytes() == sums.tobytes() and int(counts.sum()) == len(links)


def frame_peaks_boxed(frame):
    from tests import frame_peaks_ref
    return frame_peaks_ref.peaks(frame, LEVEL, EQUALITY_BOX[0], EQUALITY_BOX[1])


# ----------------------------------------------------------------------------- the reference against a scalar restatement

def scalar_draw(track, w):
    """one track's points (a list of 3-tuples of Python floats) drawn one sample at a time: [(link, k, bin, repeat)] and the skipped links"""
    L = len(track)
    s = []
    for i in range(L):
        lo, hi = max(0, i - w), min(L - 1, i + w)
        if w == 0:
            s.append(tuple(track[i]))
            continue
        row = []
        for r in range(3):
            total = track[lo][r]
            for j in range(lo + 1, hi + 1):
                total = total + track[j][r]
            row.append(total / float(hi - lo + 1))
        s.append(tuple(row))
    samples, skipped, before = [], [], None
    for i in range(L - 1):
        d = [s[i + 1][r] - s[i][r] for r in range(3)]
        e = max(abs(v) for v in d) if not any(math.isnan(v) for v in d) else math.nan
        if not e <= 4096.0:
            skipped.append(i)
            before = None
            continue
        S = max(1, int(math.ceil(e)))
        for k in range(S):
            t = (float(k) + 0.5) / float(S)
            B = tuple(math.floor((s[i][r] + d[r] * t) + 0.5) * 1.0 for r in range(3))
            samples.append((i, k, B, before is not None and B == before))
            before = B
    return samples, skipped, s


def test_the_reference_against_a_scalar_restatement_and_its_own_properties():
    rng = np.random.default_rng(9800)
    seen_skip = seen_repeat = 0
    for case in range(40):
        L = int(rng.integers(2, 14))
        step = [0.3, 1.0, 2.5, 40.0, 3000.0][case % 5]
        track = np.cumsum(rng.normal(0.0, step, (L, 3)), axis=0) + rng.uniform(-20, 20, 3)
        if case % 4 == 0:
            track = np.round(track)                                    # integer coordinates: samples on cell borders, stationary links
        if case % 7 == 0:
            track[L // 2] = track[L // 2 - 1]
        if case == 11:
            track[1, 0] = 1.7e308
            track[2, 0] = 1.7e308                                      # a window's sum overflows: links that are not finite are skipped
        for w in (0, 1, 2, 8):
            with np.errstate(over="ignore", invalid="ignore"):
                s = ref.smooth(track, w)
                links = ref.draw_track(s)
            samples, skipped, scalar_s = scalar_draw([tuple(float(v) for v in row) for row in track], w)
            assert np.asarray(scalar_s, np.float64).tobytes() == s.tobytes()
            if w == 0:
                assert s.tobytes() == track.tobytes()                  # w = 0 returns the positions' bytes
            assert [i for i, (skip, *_) in enumerate(links) if skip] == skipped
            mine = [(i, k, tuple(float(v) for v in B[k]), not bool(drawn[k])) for i, (skip, d, B, drawn) in enumerate(links) if not skip
                    for k in range(len(B))]
            assert [(i, k, struct.pack("<3d", *B), rep) for i, k, B, rep in mine] == [(i, k, struct.pack("<3d", *B), rep) for i, k, B, rep in samples]
            seen_skip += len(skipped)
            for skip, d, B, drawn in links:
                if skip:
                    continue
                kept = B[drawn]
                seen_repeat += int((~drawn).sum())
                # consecutive drawn bins of a link differ by at most 1 an axis -- c steps by |d_r| / S <= 1, and where that is 1 EXACTLY
                # (the axis of a whole-numbered extent) every c_r lies on a cell border and the rounding of t decides its side: there a
                # step may be 0 or 2, and no more --, B is monotone an axis, and a drawn bin never repeats within the link
                steps = np.diff(kept, axis=0)
                on_borders = np.abs(d) > len(B) * (1.0 - 2.0 ** -40)
                assert (np.abs(steps) <= np.where(on_borders, 2, 1)[None, :]).all()
                assert ((steps >= 0) | (d[None, :] < 0)).all() and ((steps <= 0) | (d[None, :] > 0)).all()
                assert len({row.tobytes() for row in kept + 0.0}) == len(kept)
                assert len(B) == max(1, int(np.ceil(np.abs(d).max())))
    assert seen_skip >= 3 and seen_repeat >= 20


def test_samples_minus_repeats_adds_up_on_random_frames():
    rng = np.random.default_rng(9801)
    for case in range(6):
        K = int(rng.integers(3, 8))
        base = rng.integers(0, 12, (int(rng.integers(6, 24)), 3)).astype(np.float64)
        coordinates = []
        for n in range(K):
            here = (base + n * np.array([0.5, 0.0, 0.25]))[rng.random(len(base)) < 0.9] * 3.0
            coordinates.append(here[np.argsort(rng.random(len(here)))])
        field = (30, 30, 30)
        for w in (0, 2):
            density = np.zeros(field[::-1], np.uint32)
            counts, sums = tracks_ref.empty_map(field)
            out = ref.draw_positions(coordinates, 2.25, 2, w, deposit=POINTS | LINKS, point_map=density, counts=counts, sums=sums)
            for row in out["rows"]:
                drawn = row["samples"] - row["repeats"]
                assert drawn == row["points_deposited"] + row["points_outside"] == row["links_deposited"] + row["links_outside"]
            total = ref.totals(out["rows"])
            assert int(density.sum()) == total["points_deposited"] and int(counts.sum()) == total["links_deposited"] and total["samples"] > 0
            assert density.tobytes() == counts.tobytes()                # maps of one size: the same bins
            assert total["kept_links"] == sum(len(track) for track in out["links"])


# ----------------------------------------------------------------------------- the row and the refusals

def test_the_row_has_the_headers_layout(tmp_path):
    assert C.sizeof(P.HipDrawnFrame) == 64
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "ogl_beamformer_hip.h"', "int main(void) {",
             '  printf("smooth %u\\n", (unsigned)BEAMFORMER_HIP_MAX_TRACK_SMOOTH);',
             '  printf("link_samples %.1f\\n", (double)BEAMFORMER_HIP_MAX_LINK_SAMPLES);',
             '  printf("size %zu\\n", sizeof(BeamformerHipDrawnFrame));']
    lines += [f'  printf("{name} %zu\\n", offsetof(BeamformerHipDrawnFrame, {name}));' for name, _ in P.HipDrawnFrame._fields_]
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    said = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(said["smooth"]) == P.HIP_MAX_TRACK_SMOOTH == ref.MAX_SMOOTH == 8
    assert float(said["link_samples"]) == P.HIP_MAX_LINK_SAMPLES == ref.MAX_SAMPLES == 4096.0
    assert int(said["size"]) == C.sizeof(P.HipDrawnFrame)
    for name, kind in P.HipDrawnFrame._fields_:
        assert int(said[name]) == getattr(P.HipDrawnFrame, name).offset, name
    assert sum(C.sizeof(kind) for _, kind in P.HipDrawnFrame._fields_) == 64             # no padding: the fields fill the struct
    assert [name for name, _ in P.HipDrawnFrame._fields_][4:14] == list(ref.COUNTERS)
    with open(os.path.join(ROOT, "include", "ogl_beamformer_hip.h")) as header:
        assert "static_assert(sizeof(BeamformerHipDrawnFrame) == 64" in header.read()


def test_refusals_that_need_no_device():
    L = bf.library()
    assert L.beamformer_hip_track_map_reset(None) and L.beamformer_hip_localisation_map_reset(None)
    rows = (P.HipDrawnFrame * 4)()
    C.memset(rows, 0xA5, C.sizeof(rows))
    untouched = bytes(rows)
    ms = C.c_float(-1.0)
    level, identity = (C.c_float * 4)(0.0, 0.0, 0.0, 0.0), np.tile(np.eye(3, 4).reshape(-1), 4)

    def refused(kind, count=3, thresholds=level, threshold_count=1, placements=identity, placement_count=1, reach=2.0, cap=16, min_length=2,
                smooth=1, deposit=0, out_rows=rows):
        pointer = None if placements is None else np.ascontiguousarray(placements, np.float64).ctypes.data_as(C.POINTER(C.c_double))
        assert not L.beamformer_hip_draw_tracks_last_frames(count, None, thresholds, threshold_count, pointer, placement_count, 1, reach, cap,
                                                            min_length, smooth, deposit, out_rows, C.byref(ms))
        assert bf.last_error()[0] == kind and bytes(rows) == untouched and ms.value == -1.0

    # everything the track call refuses, with its error kinds
    for count in (0, 1, P.HIP_MAX_SCORED_FRAMES + 1):
        refused(E.BufferOverflow, count=count)
    refused(E.BufferOverflow, cap=0)
    refused(E.BufferOverflow, cap=P.HIP_MAX_PEAKS_PER_FRAME + 1)
    refused(E.BufferOverflow, min_length=0)
    refused(E.BufferOverflow, min_length=P.HIP_MAX_SCORED_FRAMES + 1)
    refused(E.InvalidAccess, thresholds=None)
    refused(E.InvalidAccess, placements=None)
    refused(E.InvalidAccess, threshold_count=2)
    refused(E.InvalidAccess, placement_count=2)
    refused(E.InvalidAccess, placement_count=0)
    refused(E.InvalidAccess, thresholds=(C.c_float * 1)(-1.0))
    refused(E.InvalidAccess, thresholds=(C.c_float * 1)(float("nan")))
    for bad in (float("nan"), float("inf"), -float("inf")):
        broken = identity.copy()
        broken[12 * 2 + 7] = bad
        refused(E.InvalidAccess, placements=broken, placement_count=3)
        refused(E.InvalidAccess, reach=bad)
    refused(E.InvalidAccess, reach=-1.0)
    refused(E.InvalidAccess, reach=float(np.nextafter(np.float32(1048576.0), np.float32(np.inf))))
    # the call's own
    for smooth in (P.HIP_MAX_TRACK_SMOOTH + 1, 0xFFFFFFFF):
        refused(E.BufferOverflow, smooth=smooth)
    for deposit in (4, 7, 0x80000000, 0xFFFFFFFF):
        refused(E.InvalidAccess, deposit=deposit)
    refused(E.InvalidAccess, out_rows=None)
    for deposit in (1, 2, 3):
        refused(E.InvalidAccess, deposit=deposit)                        # a bit without its map: both were released above
