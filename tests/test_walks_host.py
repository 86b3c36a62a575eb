"""tests/walk_cases.py kept honest without a device: under every entry's das path mode and hooks the planner
(beamformer_hip_describe_das) gives the kernel, the tiles and the walk order the entry is listed for; the regimes the table reaches
cover walk_cases.REQUIRED; and the CPU oracle's frame of every entry is fit to judge a walk by -- it passes the comparison against
itself on the first bar, and at least half the voxels of EVERY tile are well above zero, so a tile written from another tile's
position cannot pass for its own.

Tile counts, bands, column groups and z chunks are not reported by the library: they are computed here from the reported fields with
the library's own formulas, each cited where it is used."""
import time

import numpy as np
import pytest

from tests import cases, parity, walk_cases as W

NAMES = [e.name for e in W.ENTRIES]
KERNEL_NAME = {0: "das_kernel", 1: "das_rca_separable_kernel", 2: "das_rca_staged_kernel", 3: "das_factored_kernel", 4: "das_hercules_kernel",
               5: "das_tile_kernel"}
HERCULES_ROWS = 8          # csrc/das_select.cpp:446 kHerculesRows


def ceil_div(a, b):
    return (a + b - 1) // b


def describe(bflib, entry, acq=None):
    """beamformer_hip_describe_das of the entry under its mode, hooks and slab: (path, kernel name, description struct)"""
    acq = acq or entry.make()
    L = bflib.library()
    for name, value in entry.hooks:
        bflib.set_hook(name, value)
    L.beamformer_hip_set_das_path(entry.mode)
    try:
        if entry.slab:
            bflib.describe_das(acq.bp, acq.filters)                    # (the block has to be there before its shard is set)
            assert L.beamformer_hip_set_output_shard(0, *entry.slab), bflib.last_error()
        path, kernel, _, reasons, d = bflib.describe_das(acq.bp, acq.filters)
    finally:
        L.beamformer_hip_set_output_shard(0, 0, 0)
        L.beamformer_hip_set_das_path(0)
        for name, _ in entry.hooks:
            bflib.set_hook(name, None)
    return path, kernel, reasons, d


def launch(entry, d):
    """(tiles, tile extents in voxels, walk order) of the launch the description `d` stands for.  describe_das reports the GENERAL
    kernel's blocks and tile shifts whatever kernel runs (csrc/lib_api.cpp:1554); das_hercules.hip and the row-column kernels have
    tiles of their own, formed here as the planner forms them."""
    size = list(entry.points)
    zcount = entry.slab[1] if entry.slab else max(1, size[2])
    ext = [size[0], size[1], zcount]
    if entry.kernel == "hercules":
        # csrc/das_select.cpp:488-491: 64 lanes along x, kHerculesRows output rows a block, one plane
        return (ceil_div(size[0], 64), ceil_div(size[1], HERCULES_ROWS), zcount), (64, HERCULES_ROWS, 1), int(d.tile_walk)
    if entry.kernel in W.STAGED_FAMILY:
        # csrc/das_select.cpp:316-318 (gather), :436-438 (staged): tiles along u (the receive axis), along v, planes
        u, v = int(d.u_axis), 1 - int(d.u_axis)
        U, V = 1 << int(d.u_shift), 1 << int(d.v_shift)
        extent = [0, 0, 1]
        extent[u], extent[v] = U, V
        return (ceil_div(size[u], U), ceil_div(size[v], V), zcount), tuple(extent), int(d.tile_walk)
    shift = [int(s) for s in d.tile_shift]
    blocks = tuple(int(b) for b in d.blocks)
    assert blocks == tuple(ceil_div(ext[k], 1 << shift[k]) for k in range(3))          # csrc/das_select.cpp:78, :661, :843 blocks_at
    return blocks, tuple(1 << s for s in shift), int(d.tile_walk)


def regimes(entry, d):
    """the regime tags (tests/walk_cases.py) of the launch described by `d`, and the derived counts behind them"""
    tiles, extent, walk = launch(entry, d)
    total = tiles[0] * tiles[1] * tiles[2]
    tags, counts = set(), {"tiles": tiles, "total": total, "walk": walk}
    if entry.kernel in W.STAGED_FAMILY:
        # BfSeparableArgs::depth_major (csrc/das_staged_shared.h:19-29): bit 0 the column walk, bit 1 the STAGED_CHECKED loop, bit 2 planes
        # in chunks of 32 (the global-table forms, csrc/das_select.cpp:430)
        assert walk & 1 and bool(walk & 2) == entry.checked and bool(walk & 4) == (int(d.uniform_tables) != 0), walk
        if walk & 4:
            zchunks = (tiles[2] + 31) >> 5                                              # csrc/das_staged_shared.h:34
            counts.update(zchunks=zchunks, launched=ceil_div(tiles[0] * tiles[1] * zchunks * 32, 8) * 8)
            tags.add(("zchunks", entry.kernel, tuple(entry.points[:2]), tiles[2]))
        else:
            # csrc/bf_kernels.h:311 bf_walk_columns; the gather kernel walks single columns (csrc/das_select.cpp:319)
            counts["walk_columns"] = 1 if entry.kernel == "gather" else 4 if tiles[0] % 4 == 0 else 2 if tiles[0] % 2 == 0 else 1
            tags.add(("xcd", entry.kernel, 1, total))
            tags.add(("columns", entry.kernel) + tiles)
    elif walk == 3:
        # csrc/das_select.cpp:120-128 tile_walk: band_rows; csrc/bf_kernels.h:328-333 bf_plane_walk_blocks: bands, slots per XCD, blocks launched
        assert tiles[2] == 1
        band_rows = max(1, tiles[1] // 32)
        bands = ceil_div(tiles[1], band_rows)
        slots = 2 * ceil_div(bands, 16)
        counts.update(band_rows=band_rows, bands=bands, slots=slots, launched=8 * slots * band_rows * tiles[0],
                      last_band_rows=tiles[1] - (bands - 1) * band_rows)
        tags.add(("bands", entry.kernel, tiles[1]))
    else:
        assert walk in (1, 2), walk
        counts.update(launched=ceil_div(total, 8) * 8, tail=ceil_div(total, 8) * 8 - total)      # csrc/bf_kernels.h:339; the ids of the tail have no tile
        tags.add(("xcd", entry.kernel, walk, total))
    if entry.slab:
        tags.add(("slab", entry.kernel) + tuple(entry.slab))
        if int(d.row_end_planes) > 0:
            tags.add(("slab_row_ends", entry.kernel))
    if entry.burst:
        tags = {("burst", t) for t in tags}
    return tags, counts, extent


@pytest.mark.parametrize("name", NAMES)
def test_the_planner_gives_the_entry_its_kernel_and_regime(name, bflib):
    entry = W.BY_NAME[name]
    acq = entry.make()
    assert acq.voxels <= 250_000 and acq.voxels * acq.bp.channel_count * acq.bp.acquisition_count <= 250_000 * 8 * 6
    assert cases.tolerance(acq) == 1e-4
    path, kernel, reasons, d = describe(bflib, entry, acq)
    assert path == entry.path and kernel == KERNEL_NAME[entry.path], (path, kernel, reasons)
    if entry.path in (0, 3, 5):            # (behind the other kernels the field is the general kernel's, which does not run)
        assert bool(d.split_shift) == entry.kernel.endswith("_split"), int(d.split_shift)
    if entry.kernel in W.STAGED_FAMILY:
        assert int(d.uniform_tables) == {"staged_uniform": 1, "paired": 2}.get(entry.kernel, 0)
        if entry.kernel != "gather":
            assert int(d.threads) == (512 if entry.kernel == "staged_cubic" else 1024)
            assert (int(d.u_shift), int(d.v_shift)) == {"staged_cubic": (5, 4), "staged_uniform": (6, 4)}.get(entry.kernel, (5, 5))
    facts = (tuple(d.blocks), tuple(d.tile_shift), int(d.split_shift), int(d.tile_walk), int(d.u_shift), int(d.v_shift), int(d.uniform_tables),
             int(d.row_end_planes))
    assert facts == W.EXPECTED[name], f"blocks, tile_shift, split_shift, tile_walk, u_shift, v_shift, uniform_tables, row_end_planes: {facts}"
    tags, counts, _ = regimes(entry, d)
    assert set(entry.regime) <= tags, (entry.regime, tags, counts)
    if entry.kernel == "staged" and entry.slab and ("slab_row_ends", "staged") in entry.regime:
        assert 0 < int(d.row_end_planes) < entry.slab[1] and int(d.blocks[2]) == entry.slab[1] - int(d.row_end_planes)      # two parts: the main one keeps the rest
    if entry.burst:
        bflib.library().beamformer_hip_set_das_path(entry.mode)
        try:
            b = bflib.describe_burst(acq.bp, W.BURST_FRAMES, acq.filters)
        finally:
            bflib.library().beamformer_hip_set_das_path(0)
        assert b.burst_kernel and b.min_frames == W.BURST_FRAMES, b.reason


def test_the_table_reaches_every_regime(bflib):
    """one assertion over the whole table: the regimes its entries are listed for -- each checked against the planner above -- are a
    superset of the list, per kernel; and the column walk of every staged kernel meets each tile count along u, v and z"""
    reached = set()
    for entry in W.ENTRIES:
        reached |= set(entry.regime)
    assert not (W.REQUIRED - reached), sorted(W.REQUIRED - reached, key=repr)
    for kernel in W.COLUMN_KERNELS:
        grids = [t[2:] for t in reached if t[0] == "columns" and t[1] == kernel]
        for axis, key in enumerate(("tiles_u", "tiles_v", "tiles_z")):
            assert set(W.COLUMN_VALUES[key]) <= {g[axis] for g in grids}, (kernel, key, sorted(grids))
        assert {4, 2, 1} == {4 if g[0] % 4 == 0 else 2 if g[0] % 2 == 0 else 1 for g in grids}      # csrc/bf_kernels.h:311
    # every staged kernel has an entry under STAGED_CHECKED
    for kernel in ("staged", "staged_real", "staged_cubic", "staged_uniform", "paired"):
        assert any(e.checked for e in W.ENTRIES if e.kernel == kernel), kernel
    # the walk orders left out are the ones written down as unreachable
    for kernel, walks in W.WALKS.items():
        for walk in (0, 1, 2):
            assert walk in walks or ("*", walk) in W.UNREACHABLE or (kernel, walk) in W.UNREACHABLE, (kernel, walk)
    coherency = sum(1 for e in W.ENTRIES if e.cw)
    assert 0.12 * len(W.ENTRIES) <= coherency <= 0.3 * len(W.ENTRIES), (coherency, len(W.ENTRIES))


def test_walk_orders_listed_as_unreachable_are_not_given(bflib):
    """depth on voxel y: the HERCULES and the row-column kernels decline, the general kernel runs"""
    for kernel, points, kw in (("hercules", (64, 17, 3), dict(builder="hercules")), ("staged", (40, 36, 3), {}), ("gather", (40, 36, 3), {})):
        entry = W.Entry("unreachable", kernel, (), points, (-2e-3, 5e-3, -2e-3), (2e-3, 9e-3, 2e-3), depth_on_y=True, **kw)
        path, _, reasons, d = describe(bflib, entry)
        assert path not in (1, 2, 4) and reasons[W.KERNELS[kernel][1]], (kernel, path)


_seen = {}


def oracle_frame(oracle, entry):
    """(acquisition, oracle frame, seconds) of the entry's whole frame; entries that share an acquisition share the frame"""
    key = entry.whole
    if key not in _seen:
        _seen.clear()
        acq = entry.make()
        t0 = time.perf_counter()
        ref, _, flags = parity.reference(oracle, acq)
        _seen[key] = (acq, ref, flags, time.perf_counter() - t0)
    return _seen[key]


@pytest.mark.parametrize("name", NAMES)
def test_the_oracle_frame_can_judge_the_walk(name, bflib, oracle):
    entry = W.BY_NAME[name]
    acq, ref, flags, seconds = oracle_frame(oracle, entry)
    print(f"{name}: oracle (float frame and double twin) {seconds:.3f} s, {acq.voxels} voxels")
    verdict = parity.compare(ref.copy(), ref, acq, flags, label=f"walks/{name}/oracle")
    assert verdict.bar == "first" and verdict.flip_voxels == 0 and verdict.rule == "per-voxel", verdict
    # every tile of the entry's tiling: at least half of its voxels above 1e-3 of the frame maximum
    _, _, _, d = describe(bflib, entry, acq)
    _, _, extent = regimes(entry, d)
    frame = ref[entry.slab[0]: entry.slab[0] + entry.slab[1]] if entry.slab else ref
    assert not np.isnan(ref).any()
    live = np.abs(frame) > 1e-3 * np.abs(ref).max()
    z, y, x = np.indices(frame.shape, sparse=True)
    ny_t, nx_t = ceil_div(frame.shape[1], extent[1]), ceil_div(frame.shape[2], extent[0])
    tile = ((z // extent[2]) * ny_t + y // extent[1]) * nx_t + x // extent[0]
    share = np.bincount(tile.ravel(), weights=live.ravel().astype(np.float64)) / np.bincount(tile.ravel())
    assert share.min() >= 0.5, f"tile {int(share.argmin())} of {share.size}: {share.min():.3f} of its voxels are live"
