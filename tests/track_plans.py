"""The plans of moving points that the track-chain and track-draw tests replay, on the host and on the device."""
import os

import numpy as np

from tests import frame_peaks_ref
from tests import planted
from tests import tracks_ref


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY = np.eye(3, 4)
HEIGHT, LEVEL, REACH = 8.0, 4.0, 1.5


def plane_plan():
    """K = 11 frames of planted.PLANE, zero but for isolated voxels of HEIGHT, each at least 2 voxels from any other of its frame; under
    the identity placement and reach 1.5: tracks of the lengths [1, 1, 2, 3, 5, 6, 8, 9, 11], 37 pairs and one forward choice that is
    not mutual.  Returns (stack (K, Z, 1, X), the spots: {frame: [(x, z)]})"""
    K, (X, _, Z) = 11, planted.PLANE
    spots = {k: [] for k in range(K)}
    for k in range(K):
        spots[k].append((2, 2 + k))                                  # moves one voxel a frame, all 11 frames
        if 2 <= k <= 9:
            spots[k].append((6, 20))                                 # length 8: neither begins in frame 0 nor ends in frame 10
        if 1 <= k <= 9:
            spots[k].append((10, 20))                                # length 9
        if k in (4, 5):
            spots[k].append((14, 5 + k))                             # length 2
        spots[k].append((18, 2 + k + (3 if k >= 5 else 0)))          # jumps 4 voxels between frames 4 and 5: tracks of 5 and 6
    spots[7].append((14, 30))                                        # alone
    spots[3] += [(20, 20), (22, 20)]                                 # both choose (21, 20) of frame 4, which returns the lower rank:
    spots[4].append((21, 20))                                        # a tie that leaves one choice unreturned, and a track of 3
    spots[5].append((21, 21))
    stack = np.zeros((K, Z, 1, X), np.float32)
    for k, where in spots.items():
        for x, z in where:
            stack[k, z, 0, x] = HEIGHT
    return stack, spots


VOLUME_SHIFT = (1, 0, 0)


def volume_plan():
    """K = 5 frames of planted.VOLUME: a lattice of every second voxel (1024 peaks), frame k moved by k voxels along x (planted.moved),
    frame 2 without the lattice rows of y = 0 mod 8 and frame 3 without those of z = 0 mod 8.  A lattice of step 2 moved by 1 leaves
    every peak EQUALLY far from its own successor and from its left neighbour's, and the tie goes to the lower rank -- almost nothing
    would pair --, so frame k's placement takes half of the motion back: the successor lies at 0.5, the other at 1.5, and the reach
    is 1.  Returns (stack (K, Z, Y, X), placements (K, 3, 4))"""
    K, (X, Y, Z) = 5, planted.VOLUME
    lattice = np.zeros((Z, Y, X), np.float32)
    lattice[::2, ::2, ::2] = HEIGHT
    stack = []
    for k in range(K):
        values = lattice.copy()
        if k == 2:
            values[:, ::8, :] = 0
        if k == 3:
            values[::8, :, :] = 0
        stack.append(planted.moved(values, tuple(k * s for s in VOLUME_SHIFT)))
    placements = np.stack([IDENTITY] * K)
    placements[:, 0, 3] = [-0.5 * k for k in range(K)]
    return np.stack(stack), placements


def coordinates_of(stack, placements, cap=65536):
    """the frames' map coordinates by the references of the peaks and of the positions"""
    A = np.asarray(placements, np.float64).reshape(-1, 3, 4)
    found = [frame_peaks_ref.peaks(f, LEVEL, cap=cap) for f in stack]
    return [tracks_ref.positions(r["index"], r["offset"], A[0 if len(A) == 1 else n]) for n, r in enumerate(found)]


def teeth(out, min_length, count):
    """the case decides something: a track kept, one dropped for its length, a kept one cut by neither end of the call's window, and
    the lengths on both sides of the bar"""
    lengths, tracks = out["lengths"], out["tracks"]
    assert len(tracks) >= 1 and len(tracks) < len(lengths)
    assert any(t["frame"] > 0 and t["frame"] + t["length"] < count and t["flags"] == 0 for t in tracks)
    assert min_length - 1 in lengths and min_length in lengths


PLANE_FIELD = (20, 1, 40)                                             # the chain tests' field over the plane plan


def scaled(factor, shift=(0.0, 0.0, 0.0)):
    """the placement m = factor * p + shift"""
    A = IDENTITY * float(factor)
    A[:, 3] = shift
    return A


def times(field, factor):
    return tuple(int(v) * factor for v in field)


def draw_plan():
    """K = 6 frames of planted.PLANE, isolated spots of HEIGHT as the plane plan's.  Under the identity and reach 1.5 -- A (x = 3): forth
    and back along z, 5 6 7 6 5 4, so the first sample of a link that turns repeats the last of the link before it; B (7, 20): stationary,
    d = 0, S = 1, every link after the first a repeat; C (x = 11): z = 10, then a line of TWO voxels at z = 11 and 12 -- one peak at 11
    with the offset +0.5 --, then 13, then 14: two links of 1.5 voxels and one of 1; D (x = 0): z = k, along the frame's edge; E
    (16, 30) in frame 2 alone; F (20, 5 + k) in frames 3 and 4; G (14 + k, 36 - k): diagonal, both axes move.
    Returns (stack (K, Z, 1, X), the voxels: {frame: [(x, z)]})"""
    K, (X, _, Z) = 6, planted.PLANE
    voxels = {k: [] for k in range(K)}
    for k in range(K):
        voxels[k] += [(3, [5, 6, 7, 6, 5, 4][k]), (7, 20), (0, k), (14 + k, 36 - k)]
    voxels[0].append((11, 10))
    voxels[1] += [(11, 11), (11, 12)]
    voxels[2] += [(11, 13), (16, 30)]
    voxels[3] += [(11, 14), (20, 8)]
    voxels[4].append((20, 9))
    stack = np.zeros((K, Z, 1, X), np.float32)
    for k, where in voxels.items():
        for x, z in where:
            stack[k, z, 0, x] = HEIGHT
    return stack, voxels


# the GPU file's calls on the draw plan: (name, placement, reach, point field, track field)
WIDE = ("48 x", scaled(48), 72.0, (600, 1, 700), (400, 1, 1000))       # S reaches 72; each map holds a corner of it
FAR_AWAY = ("4096 x, the maps under the skipped links", scaled(4096, (2 - 4096 * 11, 0, -4096 * 10)), 6144.0, (8, 1, 8192), (8, 1, 8192))
FAR_EDGE = ("4096 x, the maps along the frame's edge", scaled(4096), 6144.0, (4, 1, 9000), (2, 1, 20000))
OWN = ("4 x, moved to negative coordinates", scaled(4, (-20.0, 0.0, -30.0)), 6.0, (60, 1, 120), (40, 1, 140))
DRAW_CALLS = (WIDE, FAR_AWAY, FAR_EDGE, OWN)
EQUALITY_BOX = ((9, 0, 0), (15, 1, 40))
