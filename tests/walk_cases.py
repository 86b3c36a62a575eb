"""The DAS tile walks at their regime edges: one tiny acquisition per (kernel, regime) at which a copy of the block-to-tile map
takes another branch.  Every DAS kernel turns blockIdx.x into a tile with the same recipe -- deal the ids to the 8 XCDs, pick a walk
order, map thread to voxel -- and that text exists six times (csrc/das_general.h general_tile, das_factored.hip, das_tile.hip,
das_hercules.hip, das_staged_cubic.hip, das_staged_shared.h staged_tile_of).  A wrong copy does not fault: a tile is never written,
or written from another tile's position.  tests/test_walks_host.py keeps this table honest without a device (the planner really
gives every entry the regime it is listed for, and the regimes cover REQUIRED); tests/test_gpu_walks.py pushes every entry with
the SCRATCH_POISON hook set, so that a tile nobody wrote is a NaN, against the CPU oracle.

A plain module: no device and no library call on import.  The entries live here and not in tests/cases.py: the per-case
parametrisations and counts over cases.CASES do not move.

Every entry isolates the walk: Float32Complex RF (Float32 for the real-sample kernel) straight into DAS -- no demodulation, no
decode, nothing staged through binary16, so cases.tolerance is 1e-4 --, 8 channels (7 x 8 for HERCULES), 2 to 6 transmits, 1024
samples, f-number 0 (every term passes, every voxel is live) except for about one entry in five, which has an f-number of 0.5 to 1
and coherency weighting (the two-sum store), and at most 250 000 voxels.

Regime tags (Entry.regime; the host test derives the same tags from beamformer_hip_describe_das and compares):
  ("xcd", kernel, walk, T)        a non-plane walk order (tile_walk 1: z fastest, 2: y fastest) over T tiles: T mod 8 and T < 8
                                  decide which block ids of the launch have no tile
  ("bands", kernel, R)            a view plane (tile_walk 3) of R tile rows in XCD-balanced bands
  ("columns", kernel, tu, tv, tz) the staged kernels' column walk over tu x tv x tz tiles (columns in groups of 4 / 2 / 1)
  ("zchunks", kernel, grid, Z)    the global-table forms of das_staged.hip: planes in chunks of 32
  ("slab", kernel, first, count)  an output shard (beamformer_hip_set_output_shard) of a 65-plane volume
  ("slab_row_ends", kernel)       a slab the row-end rule cuts into parts
  ("burst", regime)               das_burst.hip (general_tile once more) on a burst of the general-kernel entry of that regime
"""
import dataclasses

import numpy as np

from ogl_beamforming_amd import configs as cfg
from ogl_beamforming_amd import params as P

I = P.InterpolationMode
D = P.DataKind

VOLUME_LO, VOLUME_HI = (-2e-3, -2e-3, 5e-3), (2e-3, 2e-3, 9e-3)
PLANE_LO, PLANE_HI = (-2e-3, 0.0, 4e-3), (2e-3, 0.0, 12e-3)
PITCH = 4e-3 / 39                      # lateral voxel pitch of the (40, 36, Z) volume: kept when a grid gets wider, so the plan is the same
BURST_FRAMES = 5                       # csrc/das_select.h kBurstMinFrames (the host test checks it against describe_burst)

# das path modes (include/ogl_beamformer_hip.h)
GENERAL, NO_STAGING, STAGED, FACTORED, HERCULES_ANY = 1, 2, 3, 4, 6
NO_SPLIT, TILE = 0x10, 0x100

# kernel -> (das path mode, the DAS path the frame must report)
KERNELS = {
    "das":            (GENERAL | NO_SPLIT, 0),        # das.hip, one thread a voxel: the form full-size frames run
    "das_split":      (GENERAL, 0),                   # das.hip, channel loop split over waves
    "factored":       (FACTORED | NO_SPLIT, 3),       # das_factored.hip
    "factored_split": (FACTORED, 3),
    "tile":           (FACTORED | NO_SPLIT | TILE, 5),  # das_tile.hip
    "hercules":       (HERCULES_ANY, 4),              # das_hercules.hip
    "gather":         (NO_STAGING, 1),                # das_separable.hip
    "staged":         (STAGED, 2),                    # das_staged.hip, tables in LDS
    "staged_real":    (STAGED, 2),                    # das_staged_real.hip
    "staged_cubic":   (STAGED, 2),                    # das_staged_cubic.hip
    "staged_uniform": (STAGED, 2),                    # das_staged.hip, 64 x 16 tiles, transmit tables global (uniform_tables 1)
    "paired":         (STAGED, 2),                    # das_staged.hip, the channel-paired form (uniform_tables 2): the headline kernel
}
# hooks a kernel's entries need to get that kernel (the shape the planner would pick is another form of das_staged.hip)
KERNEL_HOOKS = {"staged": (("STAGED_SHAPE", "5,5,6"),), "staged_uniform": (("STAGED_SHAPE", "6,4,6"),), "paired": (("STAGED_SHAPE", "5,5,5"),)}
STAGED_FAMILY = ("gather", "staged", "staged_real", "staged_cubic", "staged_uniform", "paired")


@dataclasses.dataclass(frozen=True)
class Entry:
    name: str
    kernel: str                        # key of KERNELS
    regime: tuple                      # the regime tags the entry is there for
    points: tuple
    lo: tuple
    hi: tuple
    builder: str = "rca"               # cfg.rca / cfg.hercules / cfg.forces
    transmits: int = 4
    samples: int = 1024
    interp: int = int(I.Linear)
    real: bool = False                 # Float32 samples (the real-sample kernels)
    orientation: int = 0x12
    f_number: float = 0.0
    cw: bool = False
    plane: str = None                  # HERCULES view planes: "xz"
    depth_on_y: bool = False           # a volume whose voxel y runs along world z and voxel z along world y (tile_walk 2)
    slab: tuple = None                 # (z_first, z_count) of beamformer_hip_set_output_shard
    burst: bool = False                # pushed as a burst of BURST_FRAMES frames
    checked: bool = False              # STAGED_CHECKED: staged_window_violations must be 0
    seed: int = 0

    @property
    def mode(self):
        return KERNELS[self.kernel][0]

    @property
    def path(self):
        return KERNELS[self.kernel][1]

    @property
    def hooks(self):
        return KERNEL_HOOKS.get(self.kernel, ()) + ((("STAGED_CHECKED", "1"),) if self.checked else ())

    @property
    def whole(self):
        """the entry without its slab: entries that differ only in the slab share one acquisition, one oracle frame and one whole
        frame of the library"""
        return dataclasses.replace(self, name="", regime=(), slab=None)

    def make(self):
        kind = D.Float32 if self.real else D.Float32Complex
        if self.builder == "hercules":
            acq = cfg.hercules(self.name, 7, 8, self.samples, self.points, self.lo, self.hi, seed=self.seed, data_kind=kind, interp=I(self.interp),
                               decode=0, f_number=self.f_number, cw=self.cw, plane=self.plane)
        elif self.builder == "forces":
            acq = cfg.forces(self.name, 8, 8, self.samples, self.points, self.lo, self.hi, seed=self.seed, data_kind=kind, interp=I(self.interp),
                             decode=0, f_number=self.f_number, cw=self.cw)
        else:
            acq = cfg.rca(self.name, 8, self.transmits, self.samples, self.points, self.lo, self.hi, seed=self.seed, data_kind=kind,
                          interp=I(self.interp), demodulate=False, orientation=self.orientation, f_number=self.f_number, cw=self.cw,
                          angles=np.linspace(-6.0, 6.0, self.transmits))
        if self.depth_on_y:
            m = np.array(acq.bp.das_voxel_transform[:], np.float32).reshape(4, 4)       # row k: column k of the matrix
            m[[1, 2]] = m[[2, 1]]
            acq.bp.das_voxel_transform[:] = [float(v) for v in m.reshape(-1)]
        return acq


def _entries():
    out = []

    def add(name, kernel, regime, points, lo, hi, **kw):
        n = len(out)
        if kernel == "tile":
            kw.setdefault("transmits", 4 + n % 3)                  # das_tile.hip: from 4 transmits
        elif kernel in ("factored", "factored_split"):
            kw.setdefault("transmits", 3 + n % 4)                  # das_factored.hip: from 3 transmits a chunk
        elif kernel in ("paired", "staged_uniform"):
            kw.setdefault("transmits", 4 + 2 * (n % 2))
        else:
            kw.setdefault("transmits", 2 + n % 5)
        if n % 5 == 2 and "f_number" not in kw:                    # about one in five: the f-number test culls, the store divides two sums
            kw["f_number"], kw["cw"] = (0.5, 0.7, 1.0)[(n // 5) % 3], True
        if kernel == "staged_real":
            kw["real"] = True
        if kernel in ("staged_cubic", "tile"):
            kw["interp"] = int(I.Cubic)
        assert name not in {e.name for e in out}, name
        out.append(Entry(name, kernel, tuple(regime), tuple(points), tuple(lo), tuple(hi), seed=7000 + n, **kw))

    def plain(nx):
        """no f-number on the grids much wider than the array: it would cull every channel at their lateral ends (no live voxels there)"""
        return dict(f_number=0.0) if nx > 64 else {}

    def wide(nx, ny, z_lo=5e-3, z_hi=9e-3):
        """lo, hi of a volume of nx x ny voxels at the (40, 36) volume's lateral pitch"""
        return (-PITCH * (nx - 1) / 2, -PITCH * (ny - 1) / 2, z_lo), (PITCH * (nx - 1) / 2, PITCH * (ny - 1) / 2, z_hi)

    # ---- XCD dealing, non-plane walks: T tiles in {1, 7, 8, 9, 17} (T < 8: whole XCDs idle; T mod 8 = 0, 1, 7: the ragged tail), one
    # tile across, and one grid a kernel with two tiles across and a ragged edge.  walk 1: z fastest; walk 2 (depth on voxel y): y fastest
    fine_lo, fine_hi = (-0.4e-3, -0.1e-3, 5e-3), (0.4e-3, 0.1e-3, 5.2e-3)          # das_tile.hip: a grid fine enough for its windows
    for walk in (1, 2):
        sw = dict(depth_on_y=True) if walk == 2 else {}
        # (the world box stays: with depth on y voxel y runs over lo[2] .. hi[2] of world z and voxel z over lo[1] .. hi[1] of world y)
        lo, hi, flo, fhi = VOLUME_LO, VOLUME_HI, fine_lo, fine_hi
        along = (lambda a, b, t: (a, b, t)) if walk == 1 else (lambda a, b, t: (a, t, b))      # T tiles along the depth axis
        for T in (1, 7, 8, 9, 17):
            for kernel, orient in (("das", 0x12), ("factored", 0x22)):
                # 256-voxel tiles, 16 x 16 x 1 (8 x 8 x 4 where the grid is no larger)
                add(f"{kernel}_walk{walk}_T{T}", kernel, [("xcd", kernel, walk, T)], along(8, 8, 4) if T == 1 else along(16, 16, T), lo, hi,
                    orientation=orient, **sw)
            for kernel, orient in (("das_split", 0x12), ("factored_split", 0x22)):
                # 64-voxel tiles, 8 x 8 x 1 (4 x 4 x 4)
                add(f"{kernel}_walk{walk}_T{T}", kernel, [("xcd", kernel, walk, T)], along(4, 4, 4) if T == 1 else along(8, 8, T), lo, hi,
                    orientation=orient, **sw)
            # 1024-voxel tiles, 64 x 16 x 1 (64 x 8 x 2).  Depth on y: its 16 rows run along the walk, and a volume has two planes or more --
            # 8 tiles are 4 x 2 and 9 are 3 x 3 there; 7 and 17 are primes: one tile row of that many planes (y fastest over a single row)
            tile_points = ((64, 8, 2) if T == 1 else (64, 16, T)) if walk == 1 else {1: (64, 2, 8), 8: (64, 64, 2), 9: (64, 48, 3)}.get(T, (64, 16, T))
            add(f"tile_walk{walk}_T{T}", "tile", [("xcd", "tile", walk, T)], tile_points, flo, fhi, orientation=0x22, **sw)
        add(f"das_walk{walk}_ragged", "das", [("xcd", "das", walk, 10)], along(24, 12, 5), lo, hi, **sw)
        add(f"das_split_walk{walk}_ragged", "das_split", [("xcd", "das_split", walk, 10)], along(12, 7, 5), lo, hi, **sw)
        add(f"factored_walk{walk}_ragged", "factored", [("xcd", "factored", walk, 10)], along(24, 12, 5), lo, hi, orientation=0x22, **sw)
        add(f"factored_split_walk{walk}_ragged", "factored_split", [("xcd", "factored_split", walk, 10)], along(12, 7, 5), lo, hi, orientation=0x22, **sw)
        add(f"tile_walk{walk}_ragged", "tile", [("xcd", "tile", walk, 6 if walk == 1 else 12)], (96, 12, 3) if walk == 1 else (96, 40, 2), flo, fhi,
            orientation=0x22, **sw)
    # das_hercules.hip: 64 x 8-voxel tiles; one tile only as the one-plane slab of a volume (a grid of one plane is a view plane)
    for T in (7, 8, 9, 17):
        add(f"hercules_walk1_T{T}", "hercules", [("xcd", "hercules", 1, T)], (64, 8, T), VOLUME_LO, VOLUME_HI, builder="hercules")
    add("hercules_walk1_T1", "hercules", [("xcd", "hercules", 1, 1), ("slab", "hercules", 1, 1)], (64, 8, 2), VOLUME_LO, VOLUME_HI, builder="hercules", slab=(1, 1))
    add("hercules_walk1_ragged", "hercules", [("xcd", "hercules", 1, 12)], (100, 9, 3), VOLUME_LO, VOLUME_HI, builder="hercules")
    add("hercules_walk1_issue_grid", "hercules", [("xcd", "hercules", 1, 27)], (64, 17, 9), VOLUME_LO, VOLUME_HI, builder="hercules")
    # the row-column kernels: 32 x 32-voxel tiles (32 x 16: the cubic kernel); one tile only as a one-plane slab
    for kernel in ("gather", "staged", "staged_real", "staged_cubic"):
        ny = 16 if kernel == "staged_cubic" else 20
        lo, hi = wide(31, ny)
        for T in (7, 8, 9, 17):
            add(f"{kernel}_walk1_T{T}", kernel, [("xcd", kernel, 1, T), ("columns", kernel, 1, 1, T)], (31, ny, T), lo, hi, checked=T == 9 and kernel != "gather")
        add(f"{kernel}_walk1_T1", kernel, [("xcd", kernel, 1, 1), ("columns", kernel, 1, 1, 1), ("slab", kernel, 1, 1)], (31, ny, 2), lo, hi, slab=(1, 1))

    # ---- view planes (tile_walk 3): R tile rows -- 1, 16, 17, 32, 33 and 63 bands of one row; two rows a band: 32 bands, and 33 with the
    # last half full; three rows a band, the last band of one row.  The grid height is R x tile height - 1: the last tile row is ragged too
    for R in (1, 16, 17, 32, 33, 63, 64, 65, 97):
        add(f"das_plane_R{R}", "das", [("bands", "das", R)], (64, 4 * R - 1, 1), PLANE_LO, PLANE_HI, orientation=0x22)
        # (the split forms' tiles are 64 voxels, one row high: no ragged last row; a single tile row is a plane of 32 x 2)
        split_points = (64, R, 1) if R > 1 else (32, 2, 1)
        add(f"das_split_plane_R{R}", "das_split", [("bands", "das_split", R)], split_points, PLANE_LO, PLANE_HI, orientation=0x22)
        add(f"factored_plane_R{R}", "factored", [("bands", "factored", R)], (64, 4 * R - 1, 1), PLANE_LO, PLANE_HI, orientation=0x22)
        add(f"factored_split_plane_R{R}", "factored_split", [("bands", "factored_split", R)], split_points, PLANE_LO, PLANE_HI, orientation=0x22)
        # das_hercules.hip: 8 rows a tile, an XCD's bands deepest first
        add(f"hercules_plane_R{R}", "hercules", [("bands", "hercules", R)], (64, 8 * R - 1, 1), PLANE_LO, PLANE_HI, builder="hercules", plane="xz")
        # das_tile.hip: 16 rows a tile; rows of 20 um (10 um at R = 97: at 20 the deepest rows' echoes arrive past sample 1024, the rows end
        # inside the image and the row-end rule hands the plane to das_factored.hip)
        ny = 16 * R - 1
        add(f"tile_plane_R{R}", "tile", [("bands", "tile", R)], (64, ny, 1), (-0.4e-3, 0.0, 4e-3), (0.4e-3, 0.0, 4e-3 + ny * (10e-6 if R == 97 else 20e-6)),
            orientation=0x22)
    # two tiles across, ragged: a band is then two tiles a row (a 256-voxel tile is 256 x 1 on a plane wider than 128 voxels)
    add("das_plane_R33_wide", "das", [("bands", "das", 33)], (300, 33, 1), PLANE_LO, PLANE_HI, orientation=0x22)
    add("das_split_plane_R33_wide", "das_split", [("bands", "das_split", 33)], (65, 33, 1), PLANE_LO, PLANE_HI, orientation=0x22)
    add("factored_plane_R65_wide", "factored", [("bands", "factored", 65)], (300, 65, 1), PLANE_LO, PLANE_HI, orientation=0x22)
    add("factored_split_plane_R65_wide", "factored_split", [("bands", "factored_split", 65)], (65, 65, 1), PLANE_LO, PLANE_HI, orientation=0x22)
    add("factored_plane_R17_forces", "factored", [("bands", "factored", 17)], (64, 67, 1), PLANE_LO, PLANE_HI, builder="forces")
    add("hercules_plane_R33_wide", "hercules", [("bands", "hercules", 33)], (100, 263, 1), PLANE_LO, PLANE_HI, builder="hercules", plane="xz")
    add("tile_plane_R17_wide", "tile", [("bands", "tile", 17)], (96, 271, 1), (-0.6e-3, 0.0, 4e-3), (0.6e-3, 0.0, 4e-3 + 271 * 20e-6), orientation=0x22)

    # ---- column groups of the staged kernels' walk: tiles along u 1, 2, 3, 4, 6, 8 (columns walked 1, 2, 1, 4, 2, 4 together), along v 1 and 2,
    # planes 1 (a one-plane slab), 2 and 5
    for kernel in ("staged", "staged_real", "staged_cubic"):
        v1, v2 = (16, 20) if kernel == "staged_cubic" else (20, 36)
        for nx, tu in ((45, 2), (90, 3), (128, 4), (180, 6), (250, 8)):                # (tu = 1: the XCD entries above)
            lo, hi = wide(nx, v1)
            add(f"{kernel}_columns_u{tu}", kernel, [("columns", kernel, tu, 1, 2)], (nx, v1, 2), lo, hi, checked=tu == 4, **plain(nx))
        for nx, tu in ((90, 3), (128, 4), (180, 6)):
            lo, hi = wide(nx, v2)
            add(f"{kernel}_columns_u{tu}_v2_z5", kernel, [("columns", kernel, tu, 2, 5)], (nx, v2, 5), lo, hi, **plain(nx))
        for nx, tu in ((128, 4), (180, 6)):
            lo, hi = wide(nx, v2)
            add(f"{kernel}_columns_u{tu}_v2_z1", kernel, [("columns", kernel, tu, 2, 1), ("slab", kernel, 3, 1)], (nx, v2, 5), lo, hi, slab=(3, 1), **plain(nx))

    # ---- the global-table forms of das_staged.hip: planes in chunks of 32, a second chunk ragged or of one plane
    for nx, ny in ((129, 20), (97, 36)):
        for Z in (31, 32, 33, 64, 65):
            add(f"paired_{nx}x{ny}_Z{Z}", "paired", [("zchunks", "paired", (nx, ny), Z)], (nx, ny, Z), VOLUME_LO, VOLUME_HI, checked=(nx, Z) == (129, 33))
    for Z in (33, 64):
        add(f"staged_uniform_129x20_Z{Z}", "staged_uniform", [("zchunks", "staged_uniform", (129, 20), Z)], (129, 20, Z), VOLUME_LO, VOLUME_HI, checked=Z == 33)

    # ---- slabs of a 65-plane volume: planes 1 .. 33 and 32 .. 64 (a ragged second z chunk of the paired form either way), and plane 7 alone
    for kernel, points, kw in (("das", (40, 36, 65), {}), ("gather", (40, 36, 65), {}), ("staged", (40, 36, 65), {}), ("staged_real", (40, 36, 65), {}),
                               ("staged_cubic", (40, 36, 65), {}), ("paired", (97, 36, 65), {}), ("hercules", (64, 17, 65), dict(builder="hercules"))):
        for n, slab in enumerate(((1, 33), (32, 33), (7, 1))):
            # (the three share one acquisition: transmits, f-number and seed fixed)
            add(f"{kernel}_slab_{slab[0]}_{slab[1]}", kernel, [("slab", kernel) + slab], points, VOLUME_LO, VOLUME_HI, slab=slab, transmits=4,
                f_number=0.7 if kernel in ("gather", "paired") else 0.0, cw=kernel in ("gather", "paired"), **kw)
            out[-1] = dataclasses.replace(out[-1], seed=7900 + len(kernel))
    # rows of 384 samples end inside the deepest planes: the row-end rule (csrc/das_exact.h) hands those planes of the SLAB to the kernel behind
    add("staged_slab_row_ends", "staged", [("slab_row_ends", "staged"), ("slab", "staged", 1, 6)], (40, 36, 8), VOLUME_LO, (2e-3, 2e-3, 13e-3), samples=384,
        slab=(1, 6), transmits=4)

    # ---- das_burst.hip: general_tile on a burst of kBurstMinFrames frames
    add("burst_walk1_T9", "das", [("burst", ("xcd", "das", 1, 9))], (16, 16, 9), VOLUME_LO, VOLUME_HI, burst=True)
    add("burst_plane_R33", "das", [("burst", ("bands", "das", 33))], (64, 131, 1), PLANE_LO, PLANE_HI, orientation=0x22, burst=True)
    return out


ENTRIES = _entries()
BY_NAME = {e.name: e for e in ENTRIES}

# ---- what the table must reach, per kernel (tests/test_walks_host.py: one assertion over the whole table)
XCD_TILES = (1, 7, 8, 9, 17)
PLANE_ROWS = (1, 16, 17, 32, 33, 63, 64, 65, 97)
PLANE_KERNELS = ("das", "das_split", "factored", "factored_split", "hercules", "tile")
COLUMN_KERNELS = ("staged", "staged_real", "staged_cubic")
SLAB_KERNELS = ("das", "gather", "staged", "staged_real", "staged_cubic", "paired", "hercules")
# the walk orders a kernel can be given through a single push (tile_walk as beamformer_hip_describe_das reports it)
WALKS = {"das": (1, 2), "das_split": (1, 2), "factored": (1, 2), "factored_split": (1, 2), "tile": (1, 2), "hercules": (1,),
         "gather": (1,), "staged": (1,), "staged_real": (1,), "staged_cubic": (1,)}
# ... and those it cannot, with the rule that keeps it out
UNREACHABLE = {
    ("*", 0): "tile_walk 0 (x, then y, then z) is given to no launch: csrc/das_select.cpp tile_walk() returns 1, 2 or 3, and plan_separable sets "
              "depth_major 1 for the row-column kernels; the branch is each copy's fallback",
    ("hercules", 2): "das_hercules.hip needs a transducer lateral coordinate that is a function of the output row alone (plan_hercules: moves()); on a "
                     "volume with depth on voxel y both lateral coordinates move with voxel x or z, and the general kernel runs",
    ("gather", 2): "plan_separable takes volumes with depth on voxel z only, and gives them depth_major 1",
    ("staged", 2): "as the gather kernel: plan_staged upgrades a separable plan",
    ("staged_real", 2): "as the gather kernel",
    ("staged_cubic", 2): "as the gather kernel",
}


def required():
    need = set()
    for kernel, walks in WALKS.items():
        for walk in walks:
            need |= {("xcd", kernel, walk, T) for T in XCD_TILES}
    need |= {("bands", kernel, R) for kernel in PLANE_KERNELS for R in PLANE_ROWS}
    need |= {("zchunks", "paired", grid, Z) for grid in ((129, 20), (97, 36)) for Z in (31, 32, 33, 64, 65)}
    need |= {("slab", kernel) + slab for kernel in SLAB_KERNELS for slab in ((1, 33), (32, 33), (7, 1))}
    need |= {("slab_row_ends", "staged"), ("burst", ("xcd", "das", 1, 9)), ("burst", ("bands", "das", 33))}
    return need


REQUIRED = required()
# the column walk: every value of each count, per kernel (not every combination of the three: 36 grids a kernel)
COLUMN_VALUES = {"tiles_u": (1, 2, 3, 4, 6, 8), "tiles_v": (1, 2), "tiles_z": (1, 2, 5)}


# What beamformer_hip_describe_das reports for every entry under its mode, hooks and slab -- written down, not derived (the rules live in
# csrc/das_select.cpp): (blocks, tile_shift, split_shift, tile_walk, u_shift, v_shift, uniform_tables, row_end_planes).  blocks and tile_shift are
# the general kernel's whatever kernel runs; tile_walk of the row-column kernels is BfSeparableArgs::depth_major (bit 0 the column walk, bit 1
# STAGED_CHECKED, bit 2 planes in chunks of 32).
EXPECTED = {
    "das_walk1_T1": ((1, 1, 1), (3, 3, 2), 0, 1, 0, 0, 0, 0),
    "factored_walk1_T1": ((1, 1, 1), (3, 3, 2), 0, 1, 0, 0, 0, 0),
    "das_split_walk1_T1": ((1, 1, 1), (2, 2, 2), 1, 1, 0, 0, 0, 0),
    "factored_split_walk1_T1": ((1, 1, 1), (2, 2, 2), 1, 1, 0, 0, 0, 0),
    "tile_walk1_T1": ((1, 1, 1), (6, 3, 1), 0, 1, 0, 0, 0, 0),
    "das_walk1_T7": ((1, 1, 7), (4, 4, 0), 0, 1, 0, 0, 0, 0),
    "factored_walk1_T7": ((1, 1, 7), (4, 4, 0), 0, 1, 0, 0, 0, 0),
    "das_split_walk1_T7": ((1, 1, 7), (3, 3, 0), 1, 1, 0, 0, 0, 0),
    "factored_split_walk1_T7": ((1, 1, 7), (3, 3, 0), 1, 1, 0, 0, 0, 0),
    "tile_walk1_T7": ((1, 1, 7), (6, 4, 0), 0, 1, 0, 0, 0, 0),
    "das_walk1_T8": ((1, 1, 8), (4, 4, 0), 0, 1, 0, 0, 0, 0),
    "factored_walk1_T8": ((1, 1, 8), (4, 4, 0), 0, 1, 0, 0, 0, 0),
    "das_split_walk1_T8": ((1, 1, 8), (3, 3, 0), 1, 1, 0, 0, 0, 0),
    "factored_split_walk1_T8": ((1, 1, 8), (3, 3, 0), 1, 1, 0, 0, 0, 0),
    "tile_walk1_T8": ((1, 1, 8), (6, 4, 0), 0, 1, 0, 0, 0, 0),
    "das_walk1_T9": ((1, 1, 9), (4, 4, 0), 0, 1, 0, 0, 0, 0),
    "factored_walk1_T9": ((1, 1, 9), (4, 4, 0), 0, 1, 0, 0, 0, 0),
    "das_split_walk1_T9": ((1, 1, 9), (3, 3, 0), 1, 1, 0, 0, 0, 0),
    "factored_split_walk1_T9": ((1, 1, 9), (3, 3, 0), 1, 1, 0, 0, 0, 0),
    "tile_walk1_T9": ((1, 1, 9), (6, 4, 0), 0, 1, 0, 0, 0, 0),
    "das_walk1_T17": ((1, 1, 17), (4, 4, 0), 0, 1, 0, 0, 0, 0),
    "factored_walk1_T17": ((1, 1, 17), (4, 4, 0), 0, 1, 0, 0, 0, 0),
    "das_split_walk1_T17": ((1, 1, 17), (3, 3, 0), 1, 1, 0, 0, 0, 0),
    "factored_split_walk1_T17": ((1, 1, 17), (3, 3, 0), 1, 1, 0, 0, 0, 0),
    "tile_walk1_T17": ((1, 1, 17), (6, 4, 0), 0, 1, 0, 0, 0, 0),
    "das_walk1_ragged": ((2, 1, 5), (4, 4, 0), 0, 1, 0, 0, 0, 0),
    "das_split_walk1_ragged": ((2, 1, 5), (3, 3, 0), 1, 1, 0, 0, 0, 0),
    "factored_walk1_ragged": ((2, 1, 5), (4, 4, 0), 0, 1, 0, 0, 0, 0),
    "factored_split_walk1_ragged": ((2, 1, 5), (3, 3, 0), 1, 1, 0, 0, 0, 0),
    "tile_walk1_ragged": ((2, 1, 3), (6, 4, 0), 0, 1, 0, 0, 0, 0),
    "das_walk2_T1": ((1, 1, 1), (3, 2, 3), 0, 2, 0, 0, 0, 0),
    "factored_walk2_T1": ((1, 1, 1), (3, 2, 3), 0, 2, 0, 0, 0, 0),
    "das_split_walk2_T1": ((1, 1, 1), (2, 2, 2), 1, 2, 0, 0, 0, 0),
    "factored_split_walk2_T1": ((1, 1, 1), (2, 2, 2), 1, 2, 0, 0, 0, 0),
    "tile_walk2_T1": ((1, 1, 1), (6, 1, 3), 0, 2, 0, 0, 0, 0),
    "das_walk2_T7": ((1, 7, 1), (4, 0, 4), 0, 2, 0, 0, 0, 0),
    "factored_walk2_T7": ((1, 7, 1), (4, 0, 4), 0, 2, 0, 0, 0, 0),
    "das_split_walk2_T7": ((1, 7, 1), (3, 0, 3), 1, 2, 0, 0, 0, 0),
    "factored_split_walk2_T7": ((1, 7, 1), (3, 0, 3), 1, 2, 0, 0, 0, 0),
    "tile_walk2_T7": ((1, 1, 7), (6, 4, 0), 0, 2, 0, 0, 0, 0),
    "das_walk2_T8": ((1, 8, 1), (4, 0, 4), 0, 2, 0, 0, 0, 0),
    "factored_walk2_T8": ((1, 8, 1), (4, 0, 4), 0, 2, 0, 0, 0, 0),
    "das_split_walk2_T8": ((1, 8, 1), (3, 0, 3), 1, 2, 0, 0, 0, 0),
    "factored_split_walk2_T8": ((1, 8, 1), (3, 0, 3), 1, 2, 0, 0, 0, 0),
    "tile_walk2_T8": ((1, 4, 2), (6, 4, 0), 0, 2, 0, 0, 0, 0),
    "das_walk2_T9": ((1, 9, 1), (4, 0, 4), 0, 2, 0, 0, 0, 0),
    "factored_walk2_T9": ((1, 9, 1), (4, 0, 4), 0, 2, 0, 0, 0, 0),
    "das_split_walk2_T9": ((1, 9, 1), (3, 0, 3), 1, 2, 0, 0, 0, 0),
    "factored_split_walk2_T9": ((1, 9, 1), (3, 0, 3), 1, 2, 0, 0, 0, 0),
    "tile_walk2_T9": ((1, 3, 3), (6, 4, 0), 0, 2, 0, 0, 0, 0),
    "das_walk2_T17": ((1, 17, 1), (4, 0, 4), 0, 2, 0, 0, 0, 0),
    "factored_walk2_T17": ((1, 17, 1), (4, 0, 4), 0, 2, 0, 0, 0, 0),
    "das_split_walk2_T17": ((1, 17, 1), (3, 0, 3), 1, 2, 0, 0, 0, 0),
    "factored_split_walk2_T17": ((1, 17, 1), (3, 0, 3), 1, 2, 0, 0, 0, 0),
    "tile_walk2_T17": ((1, 1, 17), (6, 4, 0), 0, 2, 0, 0, 0, 0),
    "das_walk2_ragged": ((2, 5, 1), (4, 0, 4), 0, 2, 0, 0, 0, 0),
    "das_split_walk2_ragged": ((2, 5, 1), (3, 0, 3), 1, 2, 0, 0, 0, 0),
    "factored_walk2_ragged": ((2, 5, 1), (4, 0, 4), 0, 2, 0, 0, 0, 0),
    "factored_split_walk2_ragged": ((2, 5, 1), (3, 0, 3), 1, 2, 0, 0, 0, 0),
    "tile_walk2_ragged": ((2, 3, 2), (6, 4, 0), 0, 2, 0, 0, 0, 0),
    "hercules_walk1_T7": ((2, 1, 7), (5, 3, 0), 0, 1, 0, 0, 0, 0),
    "hercules_walk1_T8": ((2, 1, 8), (5, 3, 0), 0, 1, 0, 0, 0, 0),
    "hercules_walk1_T9": ((2, 1, 9), (5, 3, 0), 0, 1, 0, 0, 0, 0),
    "hercules_walk1_T17": ((2, 1, 17), (5, 3, 0), 0, 1, 0, 0, 0, 0),
    "hercules_walk1_T1": ((2, 1, 1), (5, 3, 0), 0, 1, 0, 0, 0, 0),
    "hercules_walk1_ragged": ((7, 1, 3), (4, 4, 0), 0, 1, 0, 0, 0, 0),
    "hercules_walk1_issue_grid": ((4, 2, 9), (4, 4, 0), 0, 1, 0, 0, 0, 0),
    "gather_walk1_T7": ((4, 3, 7), (3, 3, 0), 1, 1, 5, 5, 0, 0),
    "gather_walk1_T8": ((4, 3, 8), (3, 3, 0), 1, 1, 5, 5, 0, 0),
    "gather_walk1_T9": ((4, 3, 9), (3, 3, 0), 1, 1, 5, 5, 0, 0),
    "gather_walk1_T17": ((4, 3, 17), (3, 3, 0), 1, 1, 5, 5, 0, 0),
    "gather_walk1_T1": ((16, 1, 1), (1, 5, 0), 1, 1, 5, 5, 0, 0),
    "staged_walk1_T7": ((4, 3, 7), (3, 3, 0), 1, 1, 5, 5, 0, 0),
    "staged_walk1_T8": ((4, 3, 8), (3, 3, 0), 1, 1, 5, 5, 0, 0),
    "staged_walk1_T9": ((4, 3, 9), (3, 3, 0), 1, 3, 5, 5, 0, 0),
    "staged_walk1_T17": ((4, 3, 17), (3, 3, 0), 1, 1, 5, 5, 0, 0),
    "staged_walk1_T1": ((16, 1, 1), (1, 5, 0), 1, 1, 5, 5, 0, 0),
    "staged_real_walk1_T7": ((4, 3, 7), (3, 3, 0), 1, 1, 5, 5, 0, 0),
    "staged_real_walk1_T8": ((4, 3, 8), (3, 3, 0), 1, 1, 5, 5, 0, 0),
    "staged_real_walk1_T9": ((4, 3, 9), (3, 3, 0), 1, 3, 5, 5, 0, 0),
    "staged_real_walk1_T17": ((4, 3, 17), (3, 3, 0), 1, 1, 5, 5, 0, 0),
    "staged_real_walk1_T1": ((16, 1, 1), (1, 5, 0), 1, 1, 5, 5, 0, 0),
    "staged_cubic_walk1_T7": ((4, 2, 7), (3, 3, 0), 1, 1, 5, 4, 0, 0),
    "staged_cubic_walk1_T8": ((4, 2, 8), (3, 3, 0), 1, 1, 5, 4, 0, 0),
    "staged_cubic_walk1_T9": ((4, 2, 9), (3, 3, 0), 1, 3, 5, 4, 0, 0),
    "staged_cubic_walk1_T17": ((4, 2, 17), (3, 3, 0), 1, 1, 5, 4, 0, 0),
    "staged_cubic_walk1_T1": ((8, 1, 1), (2, 4, 0), 1, 1, 5, 4, 0, 0),
    "das_plane_R1": ((1, 1, 1), (6, 2, 0), 0, 3, 0, 0, 0, 0),
    "das_split_plane_R1": ((1, 1, 1), (5, 1, 0), 1, 3, 0, 0, 0, 0),
    "factored_plane_R1": ((1, 1, 1), (6, 2, 0), 0, 3, 0, 0, 0, 0),
    "factored_split_plane_R1": ((1, 1, 1), (5, 1, 0), 1, 3, 0, 0, 0, 0),
    "hercules_plane_R1": ((1, 2, 1), (6, 2, 0), 0, 3, 0, 0, 0, 0),
    "tile_plane_R1": ((1, 1, 1), (6, 4, 0), 0, 3, 0, 0, 0, 0),
    "das_plane_R16": ((1, 16, 1), (6, 2, 0), 0, 3, 0, 0, 0, 0),
    "das_split_plane_R16": ((1, 16, 1), (6, 0, 0), 1, 3, 0, 0, 0, 0),
    "factored_plane_R16": ((1, 16, 1), (6, 2, 0), 0, 3, 0, 0, 0, 0),
    "factored_split_plane_R16": ((1, 16, 1), (6, 0, 0), 1, 3, 0, 0, 0, 0),
    "hercules_plane_R16": ((1, 32, 1), (6, 2, 0), 0, 3, 0, 0, 0, 0),
    "tile_plane_R16": ((1, 16, 1), (6, 4, 0), 0, 3, 0, 0, 0, 0),
    "das_plane_R17": ((1, 17, 1), (6, 2, 0), 0, 3, 0, 0, 0, 0),
    "das_split_plane_R17": ((1, 17, 1), (6, 0, 0), 1, 3, 0, 0, 0, 0),
    "factored_plane_R17": ((1, 17, 1), (6, 2, 0), 0, 3, 0, 0, 0, 0),
    "factored_split_plane_R17": ((1, 17, 1), (6, 0, 0), 1, 3, 0, 0, 0, 0),
    "hercules_plane_R17": ((1, 34, 1), (6, 2, 0), 0, 3, 0, 0, 0, 0),
    "tile_plane_R17": ((1, 17, 1), (6, 4, 0), 0, 3, 0, 0, 0, 0),
    "das_plane_R32": ((1, 32, 1), (6, 2, 0), 0, 3, 0, 0, 0, 0),
    "das_split_plane_R32": ((1, 32, 1), (6, 0, 0), 1, 3, 0, 0, 0, 0),
    "factored_plane_R32": ((1, 32, 1), (6, 2, 0), 0, 3, 0, 0, 0, 0),
    "factored_split_plane_R32": ((1, 32, 1), (6, 0, 0), 1, 3, 0, 0, 0, 0),
    "hercules_plane_R32": ((1, 64, 1), (6, 2, 0), 0, 3, 0, 0, 0, 0),
    "tile_plane_R32": ((1, 32, 1), (6, 4, 0), 0, 3, 0, 0, 0, 0),
    "das_plane_R33": ((1, 33, 1), (6, 2, 0), 0, 3, 0, 0, 0, 0),
    "das_split_plane_R33": ((1, 33, 1), (6, 0, 0), 1, 3, 0, 0, 0, 0),
    "factored_plane_R33": ((1, 33, 1), (6, 2, 0), 0, 3, 0, 0, 0, 0),
    "factored_split_plane_R33": ((1, 33, 1), (6, 0, 0), 1, 3, 0, 0, 0, 0),
    "hercules_plane_R33": ((1, 66, 1), (6, 2, 0), 0, 3, 0, 0, 0, 0),
    "tile_plane_R33": ((1, 33, 1), (6, 4, 0), 0, 3, 0, 0, 0, 0),
    "das_plane_R63": ((1, 63, 1), (6, 2, 0), 0, 3, 0, 0, 0, 0),
    "das_split_plane_R63": ((1, 63, 1), (6, 0, 0), 1, 3, 0, 0, 0, 0),
    "factored_plane_R63": ((1, 63, 1), (6, 2, 0), 0, 3, 0, 0, 0, 0),
    "factored_split_plane_R63": ((1, 63, 1), (6, 0, 0), 1, 3, 0, 0, 0, 0),
    "hercules_plane_R63": ((1, 126, 1), (6, 2, 0), 0, 3, 0, 0, 0, 0),
    "tile_plane_R63": ((1, 63, 1), (6, 4, 0), 0, 3, 0, 0, 0, 0),
    "das_plane_R64": ((1, 64, 1), (6, 2, 0), 0, 3, 0, 0, 0, 0),
    "das_split_plane_R64": ((1, 64, 1), (6, 0, 0), 1, 3, 0, 0, 0, 0),
    "factored_plane_R64": ((1, 64, 1), (6, 2, 0), 0, 3, 0, 0, 0, 0),
    "factored_split_plane_R64": ((1, 64, 1), (6, 0, 0), 1, 3, 0, 0, 0, 0),
    "hercules_plane_R64": ((1, 128, 1), (6, 2, 0), 0, 3, 0, 0, 0, 0),
    "tile_plane_R64": ((1, 64, 1), (6, 4, 0), 0, 3, 0, 0, 0, 0),
    "das_plane_R65": ((1, 65, 1), (6, 2, 0), 0, 3, 0, 0, 0, 0),
    "das_split_plane_R65": ((1, 65, 1), (6, 0, 0), 1, 3, 0, 0, 0, 0),
    "factored_plane_R65": ((1, 65, 1), (6, 2, 0), 0, 3, 0, 0, 0, 0),
    "factored_split_plane_R65": ((1, 65, 1), (6, 0, 0), 1, 3, 0, 0, 0, 0),
    "hercules_plane_R65": ((1, 130, 1), (6, 2, 0), 0, 3, 0, 0, 0, 0),
    "tile_plane_R65": ((1, 65, 1), (6, 4, 0), 0, 3, 0, 0, 0, 0),
    "das_plane_R97": ((1, 97, 1), (6, 2, 0), 0, 3, 0, 0, 0, 0),
    "das_split_plane_R97": ((1, 97, 1), (6, 0, 0), 1, 3, 0, 0, 0, 0),
    "factored_plane_R97": ((1, 97, 1), (6, 2, 0), 0, 3, 0, 0, 0, 0),
    "factored_split_plane_R97": ((1, 97, 1), (6, 0, 0), 1, 3, 0, 0, 0, 0),
    "hercules_plane_R97": ((1, 194, 1), (6, 2, 0), 0, 3, 0, 0, 0, 0),
    "tile_plane_R97": ((1, 97, 1), (6, 4, 0), 0, 3, 0, 0, 0, 0),
    "das_plane_R33_wide": ((2, 33, 1), (8, 0, 0), 0, 3, 0, 0, 0, 0),
    "das_split_plane_R33_wide": ((2, 33, 1), (6, 0, 0), 1, 3, 0, 0, 0, 0),
    "factored_plane_R65_wide": ((2, 65, 1), (8, 0, 0), 0, 3, 0, 0, 0, 0),
    "factored_split_plane_R65_wide": ((2, 65, 1), (6, 0, 0), 1, 3, 0, 0, 0, 0),
    "factored_plane_R17_forces": ((1, 17, 1), (6, 2, 0), 0, 3, 0, 0, 0, 0),
    "hercules_plane_R33_wide": ((1, 132, 1), (7, 1, 0), 0, 3, 0, 0, 0, 0),
    "tile_plane_R17_wide": ((2, 17, 1), (6, 4, 0), 0, 3, 0, 0, 0, 0),
    "staged_columns_u2": ((6, 3, 2), (3, 3, 0), 1, 1, 5, 5, 0, 0),
    "staged_columns_u3": ((12, 3, 2), (3, 3, 0), 1, 1, 5, 5, 0, 0),
    "staged_columns_u4": ((16, 3, 2), (3, 3, 0), 1, 3, 5, 5, 0, 0),
    "staged_columns_u6": ((23, 3, 2), (3, 3, 0), 1, 1, 5, 5, 0, 0),
    "staged_columns_u8": ((32, 3, 2), (3, 3, 0), 1, 1, 5, 5, 0, 0),
    "staged_columns_u3_v2_z5": ((12, 5, 5), (3, 3, 0), 1, 1, 5, 5, 0, 0),
    "staged_columns_u4_v2_z5": ((16, 5, 5), (3, 3, 0), 1, 1, 5, 5, 0, 0),
    "staged_columns_u6_v2_z5": ((23, 5, 5), (3, 3, 0), 1, 1, 5, 5, 0, 0),
    "staged_columns_u4_v2_z1": ((128, 1, 1), (0, 6, 0), 1, 1, 5, 5, 0, 0),
    "staged_columns_u6_v2_z1": ((180, 1, 1), (0, 6, 0), 1, 1, 5, 5, 0, 0),
    "staged_real_columns_u2": ((6, 3, 2), (3, 3, 0), 1, 1, 5, 5, 0, 0),
    "staged_real_columns_u3": ((12, 3, 2), (3, 3, 0), 1, 1, 5, 5, 0, 0),
    "staged_real_columns_u4": ((16, 3, 2), (3, 3, 0), 1, 3, 5, 5, 0, 0),
    "staged_real_columns_u6": ((23, 3, 2), (3, 3, 0), 1, 1, 5, 5, 0, 0),
    "staged_real_columns_u8": ((32, 3, 2), (3, 3, 0), 1, 1, 5, 5, 0, 0),
    "staged_real_columns_u3_v2_z5": ((12, 5, 5), (3, 3, 0), 1, 1, 5, 5, 0, 0),
    "staged_real_columns_u4_v2_z5": ((16, 5, 5), (3, 3, 0), 1, 1, 5, 5, 0, 0),
    "staged_real_columns_u6_v2_z5": ((23, 5, 5), (3, 3, 0), 1, 1, 5, 5, 0, 0),
    "staged_real_columns_u4_v2_z1": ((128, 1, 1), (0, 6, 0), 1, 1, 5, 5, 0, 0),
    "staged_real_columns_u6_v2_z1": ((180, 1, 1), (0, 6, 0), 1, 1, 5, 5, 0, 0),
    "staged_cubic_columns_u2": ((6, 2, 2), (3, 3, 0), 1, 1, 5, 4, 0, 0),
    "staged_cubic_columns_u3": ((12, 2, 2), (3, 3, 0), 1, 1, 5, 4, 0, 0),
    "staged_cubic_columns_u4": ((16, 2, 2), (3, 3, 0), 1, 3, 5, 4, 0, 0),
    "staged_cubic_columns_u6": ((23, 2, 2), (3, 3, 0), 1, 1, 5, 4, 0, 0),
    "staged_cubic_columns_u8": ((32, 2, 2), (3, 3, 0), 1, 1, 5, 4, 0, 0),
    "staged_cubic_columns_u3_v2_z5": ((12, 3, 5), (3, 3, 0), 1, 1, 5, 4, 0, 0),
    "staged_cubic_columns_u4_v2_z5": ((16, 3, 5), (3, 3, 0), 1, 1, 5, 4, 0, 0),
    "staged_cubic_columns_u6_v2_z5": ((23, 3, 5), (3, 3, 0), 1, 1, 5, 4, 0, 0),
    "staged_cubic_columns_u4_v2_z1": ((64, 1, 1), (1, 5, 0), 1, 1, 5, 4, 0, 0),
    "staged_cubic_columns_u6_v2_z1": ((90, 1, 1), (1, 5, 0), 1, 1, 5, 4, 0, 0),
    "paired_129x20_Z31": ((17, 3, 31), (3, 3, 0), 1, 5, 5, 5, 2, 0),
    "paired_129x20_Z32": ((17, 3, 32), (3, 3, 0), 1, 5, 5, 5, 2, 0),
    "paired_129x20_Z33": ((17, 3, 33), (3, 3, 0), 1, 7, 5, 5, 2, 0),
    "paired_129x20_Z64": ((17, 3, 64), (3, 3, 0), 1, 5, 5, 5, 2, 0),
    "paired_129x20_Z65": ((17, 3, 65), (3, 3, 0), 1, 5, 5, 5, 2, 0),
    "paired_97x36_Z31": ((13, 5, 31), (3, 3, 0), 1, 5, 5, 5, 2, 0),
    "paired_97x36_Z32": ((13, 5, 32), (3, 3, 0), 1, 5, 5, 5, 2, 0),
    "paired_97x36_Z33": ((13, 5, 33), (3, 3, 0), 1, 5, 5, 5, 2, 0),
    "paired_97x36_Z64": ((13, 5, 64), (3, 3, 0), 1, 5, 5, 5, 2, 0),
    "paired_97x36_Z65": ((13, 5, 65), (3, 3, 0), 1, 5, 5, 5, 2, 0),
    "staged_uniform_129x20_Z33": ((17, 3, 33), (3, 3, 0), 1, 7, 6, 4, 1, 0),
    "staged_uniform_129x20_Z64": ((17, 3, 64), (3, 3, 0), 1, 5, 6, 4, 1, 0),
    "das_slab_1_33": ((3, 3, 33), (4, 4, 0), 0, 1, 0, 0, 0, 0),
    "das_slab_32_33": ((3, 3, 33), (4, 4, 0), 0, 1, 0, 0, 0, 0),
    "das_slab_7_1": ((10, 1, 1), (2, 6, 0), 0, 1, 0, 0, 0, 0),
    "gather_slab_1_33": ((5, 5, 33), (3, 3, 0), 1, 1, 5, 5, 0, 0),
    "gather_slab_32_33": ((5, 5, 33), (3, 3, 0), 1, 1, 5, 5, 0, 0),
    "gather_slab_7_1": ((40, 1, 1), (0, 6, 0), 1, 1, 5, 5, 0, 0),
    "staged_slab_1_33": ((5, 5, 33), (3, 3, 0), 1, 1, 5, 5, 0, 0),
    "staged_slab_32_33": ((5, 5, 33), (3, 3, 0), 1, 1, 5, 5, 0, 0),
    "staged_slab_7_1": ((40, 1, 1), (0, 6, 0), 1, 1, 5, 5, 0, 0),
    "staged_real_slab_1_33": ((5, 5, 33), (3, 3, 0), 1, 1, 5, 5, 0, 0),
    "staged_real_slab_32_33": ((5, 5, 33), (3, 3, 0), 1, 1, 5, 5, 0, 0),
    "staged_real_slab_7_1": ((40, 1, 1), (0, 6, 0), 1, 1, 5, 5, 0, 0),
    "staged_cubic_slab_1_33": ((5, 5, 33), (3, 3, 0), 1, 1, 5, 4, 0, 0),
    "staged_cubic_slab_32_33": ((5, 5, 33), (3, 3, 0), 1, 1, 5, 4, 0, 0),
    "staged_cubic_slab_7_1": ((40, 1, 1), (0, 6, 0), 1, 1, 5, 4, 0, 0),
    "paired_slab_1_33": ((13, 5, 33), (3, 3, 0), 1, 5, 5, 5, 2, 0),
    "paired_slab_32_33": ((13, 5, 33), (3, 3, 0), 1, 5, 5, 5, 2, 0),
    "paired_slab_7_1": ((97, 1, 1), (0, 6, 0), 1, 5, 5, 5, 2, 0),
    "hercules_slab_1_33": ((4, 2, 33), (4, 4, 0), 0, 1, 0, 0, 0, 0),
    "hercules_slab_32_33": ((4, 2, 33), (4, 4, 0), 0, 1, 0, 0, 0, 0),
    "hercules_slab_7_1": ((8, 1, 1), (3, 5, 0), 0, 1, 0, 0, 0, 0),
    "staged_slab_row_ends": ((5, 5, 5), (3, 3, 0), 1, 1, 5, 5, 0, 1),
    "burst_walk1_T9": ((1, 1, 9), (4, 4, 0), 0, 1, 0, 0, 0, 0),
    "burst_plane_R33": ((1, 33, 1), (6, 2, 0), 0, 3, 0, 0, 0, 0),
}
