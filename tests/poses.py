"""Ten named poses of the voxel grid and of the array: functions that take an Acquisition and rewrite bp.das_voxel_transform and / or
bp.xdc_transform in place.  Every named case and every generator of tests/draws.py builds an axis-aligned grid
(configs._voxel_transform) and an array that is only translated (configs.translation); the poses put the same acquisitions off the
axes.  A plain module: no device, no library.

GENERAL  no exact zero of either matrix survives: the gates of csrc/das_select.cpp must decline the separable, staged and HERCULES
         kernels, and the "any position" kernels (das.hip, das_factored.hip, das_tile.hip) compute a tilted frame.
SPECIAL  the exact zeros survive (mirrors, a quarter turn, a sheared z column, the array the other way round): the gates still admit
         the fast paths, with delays that fall where they used to rise and windows whose minimum sits at the other end of the tile.

Conventions: both matrices are column-major 4 x 4 (16 floats).  V = das_voxel_transform takes unit-cube coordinates u to world
coordinates; X = xdc_transform takes world coordinates to the array's.  Every matrix is worked out in float64 from the stored float32
entries and rounded to float32 ONCE, when it is stored; exact zeros and +-1 are made by sign changes, row permutations and additions
to single entries, never as cos(90 deg)."""
import numpy as np

from tests import cases

MM = 1e-3


def matrix(m16):
    """the 4 x 4 float64 matrix of 16 column-major floats"""
    return np.array(m16[:], np.float64).reshape(4, 4).T


def store(m16, m):
    """round once: float64 matrix -> the 16 column-major floats of the parameter block (-0.0 stored as 0.0)"""
    m16[:] = [float(np.float32(v)) for v in (np.asarray(m, np.float64) + 0.0).T.reshape(-1)]


def rotation(axis, degrees):
    """4 x 4 rotation about world axis 0 / 1 / 2 (x / y / z), right-handed"""
    c, s = np.cos(np.radians(degrees)), np.sin(np.radians(degrees))
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    r = np.eye(4)
    r[i, i], r[i, j], r[j, i], r[j, j] = c, -s, s, c
    return r


def translate(t):
    m = np.eye(4)
    m[:3, 3] = t
    return m


def about(r, c):
    """T(c) R T(-c)"""
    return translate(c) @ r @ translate(-np.asarray(c))


def centre(bp, V):
    """the world image of the unit cube's centre: (1/2, 1/2, 1/2), or (1/2, 1/2, 0) for a grid of one z plane"""
    u = np.array([0.5, 0.5, 0.0 if int(bp.output_points[2]) == 1 else 0.5, 1.0])
    return (V @ u)[:3]


# ---- the pieces: (bp, V, X) -> (V, X), float64 throughout

TILT_GRID = rotation(1, 3.0) @ rotation(0, -2.0) @ rotation(2, 5.0)
TILT_ARRAY = rotation(2, 4.0) @ rotation(0, 1.5) @ rotation(1, -2.0)


def _tilt_grid(bp, V, X):
    return about(TILT_GRID, centre(bp, V)) @ V, X


def _tilt_array(bp, V, X):
    return V, X @ TILT_ARRAY                  # about the world origin: the array's centre in every config


def _spin_plane(bp, V, X):
    r = rotation(2, 25.0)
    V = about(r, centre(bp, V)) @ V
    V[:3, 3] += 0.3 * MM * r[:3, 1]           # off axis along the turned y direction
    return V, X


def flip(V, axis):
    """V . F, F taking unit coordinate u to 1 - u on `axis`: the origin at the far corner, the extent negative"""
    V = V.copy()
    V[:, 3] = V[:, 3] + V[:, axis]
    V[:, axis] = -V[:, axis]
    V[3, 3] = 1.0
    return V


def quarter_turns(bp, V, n):
    """n exact quarter turns about the depth axis through the grid's centre: rows 0 and 1 swapped with one sign changed"""
    for _ in range(n % 4):
        c = centre(bp, V)
        W = V.copy()
        W[0, :3], W[1, :3] = -V[1, :3], V[0, :3]
        W[0, 3] = -(V[1, 3] - c[1]) + c[0]
        W[1, 3] = (V[0, 3] - c[0]) + c[1]
        V = W
    return V


def shear(V, dx, dy):
    """planes drift laterally with z: (dx, dy) added to the x and y entries of the z column"""
    V = V.copy()
    V[0, 2] += dx
    V[1, 2] += dy
    return V


def _flip_x(bp, V, X):
    return flip(V, 0), X


def _flip_y(bp, V, X):
    return flip(V, 1), X


def _quarter(bp, V, X):
    return quarter_turns(bp, V, 1), X


def _shear(bp, V, X):
    return shear(V, 0.7 * MM, -0.4 * MM), X


def _array_half_turn(bp, V, X):
    X = X.copy()
    X[0, 0], X[1, 1] = -X[0, 0], -X[1, 1]     # the translation stays: the element order is reversed along both axes
    return V, X


def rewrite(acq, *pieces):
    """apply the pieces in order in float64 and store each matrix that changed, once"""
    bp = acq.bp
    V0, X0 = matrix(bp.das_voxel_transform), matrix(bp.xdc_transform)
    V, X = V0, X0
    for piece in pieces:
        V, X = piece(bp, V, X)
    if V is not V0:
        store(bp.das_voxel_transform, V)
    if X is not X0:
        store(bp.xdc_transform, X)
    return acq


POSES = {
    "tilt_grid": (_tilt_grid,),
    "tilt_array": (_tilt_array,),
    "tilt_both": (_tilt_grid, _tilt_array),
    "spin_plane": (_spin_plane,),
    "flip_x": (_flip_x,),
    "flip_y": (_flip_y,),
    "quarter": (_quarter,),
    "shear": (_shear,),
    "array_half_turn": (_array_half_turn,),
    "combo": (_flip_x, _shear, _array_half_turn),
}
GENERAL = ("tilt_grid", "tilt_array", "tilt_both", "spin_plane")
SPECIAL = ("flip_x", "flip_y", "quarter", "shear", "array_half_turn", "combo")
ALL = GENERAL + SPECIAL


# What a FORCED das path mode is expected to run under the poses -- written down, not derived, like cases.EXPECTED_AUTOMATIC (the rules
# live in csrc/das_select.cpp).  Per group: the das path mode, and per case the path under the GENERAL poses, under the SPECIAL poses,
# and under the poses listed by name where they differ from their class.
_HERCULES_PLANES = ("harness_hercules_small", "harness_hercules_yz_small", "hercules_plane_xz", "hercules_plane_xz_short_rows", "hercules_plane_yz",
                    "hercules_plane_yz_short_rows", "uhercules_plane_xz_sparse")
_HERCULES_VOLUMES = ("config3_small", "config5_literal_order", "config5_small", "hercules_chirp", "hercules_demod_decode_cw", "hercules_order12",
                     "hercules_real", "hercules_table_cw", "hercules_table_real_cubic", "hercules_wide_cubic_cw", "hercules_wide_cw",
                     "hercules_wide_nearest", "hercules_wide_real_swapped", "uhercules_sparse", "uhercules_table_sparse", "uhercules_wide_sparse_cubic")
_STAGED = ("config4_small", "rca_sep_ragged_cubic", "rca_staged_auto", "rca_staged_cubic", "rca_staged_cubic_short_rows", "rca_staged_fine",
           "rca_staged_ragged", "rca_staged_real", "rca_staged_real_narrow_cw", "rca_staged_real_short_rows", "rca_staged_w64", "rca_vls_staged")
EXPECTED_FORCED = {
    # flag 0x114: the block-staged factored kernel has no alignment test -- it stays under every pose
    "tile": {"mode": 0x114, "general": 5, "special": 5,
             "cases": ("tile_forces", "tile_near_field", "tile_thin_volume", "tile_tpw", "tile_tpw_w64", "tile_uforces_cw", "tile_w32")},
    # mode 6: the aligned-grid HERCULES kernel wherever a transducer axis is a function of the output row alone; a sheared z column
    # leaves that true on a grid of one plane only
    "hercules_planes": {"mode": 6, "general": 0, "special": 4, "cases": _HERCULES_PLANES},
    "hercules_volumes": {"mode": 6, "general": 0, "special": 4, "shear": 0, "combo": 0, "cases": _HERCULES_VOLUMES},
    # mode 3: the LDS-staged kernel where the delay is separable, the factored kernel where it is not
    "staged": {"mode": 3, "general": 3, "special": 2, "cases": _STAGED},
    # ... and the cases of which the row-end rule leaves the staged kernel no plane (cases.ROW_END_EVERY_PLANE): the gather kernel
    "staged_every_plane_rerouted": {"mode": 3, "general": 3, "special": 1, "cases": ("rca_staged_fine_vls_short_rows", "rca_vls_staged_short_rows")},
}


def expected_forced(group, pose):
    e = EXPECTED_FORCED[group]
    return e.get(pose, e["general" if pose in GENERAL else "special"])


def apply(acq, pose):
    return rewrite(acq, *POSES[pose])


def posed(name, pose):
    """cases.make(name) with the pose applied (pose None: the case as it is)"""
    acq = cases.make(name)
    return acq if pose is None else apply(acq, pose)


def live_share(ref):
    """the fraction of a frame's voxels that are finite and not zero"""
    return float(np.mean(np.isfinite(ref) & (ref != 0)))
