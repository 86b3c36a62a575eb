"""The block-wise ensemble filter on the device (beamformer_hip_gram_boxes_last_frames, beamformer_hip_mix_field_last_frames;
csrc/ensemble_blocks.hip) and the loop burst -> lattice_boxes -> gram_boxes -> projector a box -> mix_field.  The grids and the pushes
are the ensemble tests' (tests/ring_frames.py).

Gram boxes: every matrix and every info is compared BIT FOR BIT with beamformer_hip_gram_last_frames on the same frames and the same
box -- that call's own parity is tests/test_gpu_ensemble.py's business.  Field mix: every voxel of every output is compared BIT FOR BIT
(NaN by position) with the definition's lerps, in float32 with an exact fmaf (tests/block_filter_ref.py), applied to corner frames that
beamformer_hip_mix_last_frames itself produced on the device under each node's table; a mix moves "the K newest", so the burst is pushed
again between the calls.  The loop is judged against the float64 reference within the bounds it derives.  Every test prints what it
measured before it asserts."""
import ctypes as C

import numpy as np
import pytest

from ogl_beamforming_amd import lib as bf
from ogl_beamforming_amd import params as P
from tests import block_filter_ref as ref
from tests import ensemble_ref
from tests import planted
from tests.frame_info import newest_info
from tests.frame_ops_table import node_weights
from tests.ring_frames import block, BOXES, check_peaks as check_call, ensemble, GRIDS, region_of, same_as_singles, singles, weights
from tests.scaffold import automatic_path  # noqa: F401

pytestmark = pytest.mark.gpu
D = P.DataKind


@pytest.fixture(autouse=True)
def hooks_cleared(automatic_path, bflib):
    yield
    bflib.set_hook("GRAM_BOXES_BUDGET", None)
    bflib.set_hook("BLEND_SHAPE", None)


# ---- gram boxes ----

def box_list(which):
    """the whole frame, one voxel, the grid's box of odd offsets and extents, two boxes that overlap, and one of them twice"""
    px, py, pz = GRIDS[which][0] if which != "nan" else (24, 1, 40)
    odd = BOXES[which] if which != "nan" else ((1, 0, 3), (21, 1, 35))
    hx, hz = px // 2, pz // 2
    first = ((0, 0, 0), (hx + 2, py, pz))
    second = ((hx - 1, 0, 1), (px - hx + 1, py, pz - 1))
    return [((0, 0, 0), (px, py, pz)), ((px - 1, py - 1, pz - 1), (1, 1, 1)), odd, first, second, odd]


def chunk_words(volume, K):
    """bf_gram_chunk_words (csrc/bf_kernels.h)"""
    words = (volume + 63) // 64
    tiles = (K + 31) // 32
    cap = max(64, 1024 // (tiles * (tiles + 1) // 2))
    return max(4, (words + cap - 1) // cap)


def batches_under(boxes, K, budget):
    """how many batches the boxes make under a budget of partials: 16 KiB a chunk and tile pair, a box that does not fit alone"""
    tiles = (K + 31) // 32
    pairs = tiles * (tiles + 1) // 2
    count, held = 0, None
    for _, (nx, ny, nz) in boxes:
        words = (nx * ny * nz + 63) // 64
        each = chunk_words(nx * ny * nz, K)
        need = (words + each - 1) // each * pairs * 16384
        if held is None or held + need > budget:
            count, held = count + 1, 0
        held += need
    return count


@pytest.mark.parametrize("K", [1, 2, 17, 33, 65])
@pytest.mark.parametrize("which", ["plane", "square", "volume", "real"])
def test_gram_boxes_are_the_single_box_calls(which, K, bflib):
    frames, ids = ensemble(which, K)
    boxes = box_list(which)
    want = singles(K, boxes)
    regions = [region_of(box) for box in boxes]
    got, infos, ms = bflib.gram_boxes_last_frames(K, regions)
    print(f"  {which} K {K}: {len(boxes)} boxes, voxels {[int(i.voxels) for i in infos]}, {ms * 1e3:.1f} us")
    assert got.shape == (len(boxes), K, K) and got.dtype == np.complex128 and ms > 0
    assert int(infos[0].first_frame_id) == ids[0] and int(infos[0].voxels) == frames[0].size
    assert tuple(infos[2].region_first) == boxes[2][0] and tuple(infos[2].region_count) == boxes[2][1]
    same_as_singles(got, infos, want, "one call")
    # the boxes differ (the test would pass on a kernel that reduced box 0 every time otherwise); the repeated box repeats
    assert got[0].tobytes() != got[3].tobytes() and got[2].tobytes() == got[5].tobytes()
    # a permuted list gives the permuted result
    order = [4, 0, 5, 2, 1, 3]
    permuted, permuted_infos, _ = bflib.gram_boxes_last_frames(K, [regions[n] for n in order])
    same_as_singles(permuted, permuted_infos, [want[n] for n in order], "permuted")
    # the same list under a budget that cuts it into three batches or more: the same bytes
    budget = 40000 if K <= 32 else 1
    batches = batches_under(boxes, K, budget)
    print(f"  budget {budget}: {batches} batches")
    assert batches >= 3
    bflib.set_hook("GRAM_BOXES_BUDGET", budget)
    cut, cut_infos, _ = bflib.gram_boxes_last_frames(K, regions)
    bflib.set_hook("GRAM_BOXES_BUDGET", None)
    same_as_singles(cut, cut_infos, want, "three batches or more")
    # the same call again: equal bytes
    again, again_infos, _ = bflib.gram_boxes_last_frames(K, regions)
    assert again.tobytes() == got.tobytes() and [bytes(i) for i in again_infos] == [bytes(i) for i in infos]


def test_gram_boxes_over_the_nan_block(bflib):
    frames, ids = ensemble("nan", 3)
    nan = np.isnan(frames).any(axis=0)
    assert nan.sum() >= 64
    z, x = np.argwhere(nan[:, 0, :])[0]
    boxes = box_list("nan") + [((int(x), 0, int(z)), (1, 1, 1))]
    want = singles(3, boxes)
    got, infos, _ = bflib.gram_boxes_last_frames(3, [region_of(box) for box in boxes])
    print(f"  non-finite voxels a box: {[int(i.non_finite) for i in infos]}")
    same_as_singles(got, infos, want, "nan")
    assert int(infos[0].non_finite) == int(nan.sum()) and (int(infos[-1].voxels), int(infos[-1].non_finite)) == (0, 1) and not got[-1].any()
    assert np.isfinite(got.real).all() and np.isfinite(got.imag).all()
    bflib.set_hook("GRAM_BOXES_BUDGET", 1)
    cut, cut_infos, _ = bflib.gram_boxes_last_frames(3, [region_of(box) for box in boxes])
    same_as_singles(cut, cut_infos, want, "nan, a box a batch")


# ---- field mix ----

LATTICES = {
    "one":     dict(nodes=(1, 1, 1), first=(9, 9, 9), step=(0, 0, 0)),                 # the plain mix: first and step are not read
    "square":  dict(nodes=(3, 1, 4), first=(5, 0, 3), step=(23, 1, 17)),
    "beyond":  dict(nodes=(3, 1, 2), first=(0, 0, 0), step=(20, 1, 9)),                # plane 33 x 1 x 7: x nodes at 0, 20, 40; z nodes at 0, 9
    "volume":  dict(nodes=(2, 2, 3), first=(2, 1, 0), step=(5, 3, 2)),
    "flat":    dict(nodes=(2, 2, 1), first=(3, 0, 0), step=(11, 1, 1)),                # two nodes along y on a grid of one point along y
    "nan":     dict(nodes=(2, 1, 2), first=(5, 0, 7), step=(9, 1, 20)),
}


def corners_by_the_plain_mix(which, K, W):
    """corner frames (Nz, Ny, Nx, M, Z, Y, X) that beamformer_hip_mix_last_frames stored under each node's table, the burst pushed
    afresh for each"""
    acq = block(which)
    Nz, Ny, Nx, M, _ = W.shape
    out = None
    for jz in range(Nz):
        for jy in range(Ny):
            for jx in range(Nx):
                ensemble(which, K)
                bf.mix_last_frames(K, W[jz, jy, jx], timed=False)
                frames = bf.get_last_frames(acq.bp, M).copy()
                if out is None:
                    out = np.empty((Nz, Ny, Nx) + frames.shape, frames.dtype)
                out[jz, jy, jx] = frames
    return out


def same_bits(got, want):
    """bit for bit, NaN by position (payloads are not promised)"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    g, w = got.view(np.float32), want.view(np.float32)
    nan = np.isnan(w)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(np.isnan(g), nan) and np.array_equal(g.view(np.uint32)[~nan], w.view(np.uint32)[~nan])


def field_mix(which, K, W, lattice, tag=0):
    """push the burst, mix it under the field: (outputs (M, Z, Y, X), first id, the sources' ids, device ms)"""
    acq = block(which)
    frames, ids = ensemble(which, K)
    first, ms = bf.mix_field_last_frames(K, W, lattice["first"], lattice["step"], tag=tag)
    return bf.get_last_frames(acq.bp, W.shape[3]).copy(), first, ids, ms


CASES = [("plane", "one", 1, 1), ("square", "square", 17, 17), ("plane", "beyond", 2, 16), ("volume", "volume", 17, 1),
         ("plane", "flat", 65, 17), ("real", "beyond", 17, 16), ("real", "flat", 2, 17), ("volume", "volume", 65, 16), ("plane", "beyond", 1, 17)]


@pytest.mark.parametrize("which,name,K,M", CASES)
def test_field_mix_is_the_blend_of_the_plain_mixes(which, name, K, M, bflib):
    lattice = LATTICES[name]
    real = not GRIDS[which][3]
    W = node_weights(lattice, M, K, 8100 + 10 * K + M, real)
    corners = corners_by_the_plain_mix(which, K, W)
    want = ref.blend(corners, lattice["first"], lattice["step"])
    out, first, ids, ms = field_mix(which, K, W, lattice, tag=5)
    g, w = out.view(np.float32), want.view(np.float32)
    differ = int((g.view(np.uint32) != w.view(np.uint32)).sum())
    blended = [int(ref.segments(GRIDS[which][0][a], lattice["nodes"][a], lattice["first"][a], lattice["step"][a])[3].sum()) for a in range(3)]
    print(f"  {which} lattice {name} {lattice['nodes']} K {K} -> M {M} {'real' if real else 'complex'}: {differ} of {g.size} floats differ, "
          f"voxels blended an axis {blended}, {ms * 1e3:.1f} us")
    assert out.shape == (M,) + corners.shape[4:] and out.dtype == corners.dtype and ms > 0
    assert same_bits(out, want)
    # the corners do differ: a kernel that took one node's table everywhere fails above
    if name != "one":
        assert not same_bits(corners[0, 0, 0], corners[-1, -1, -1]) and not same_bits(out, corners[0, 0, 0])
    else:
        assert same_bits(out, corners[0, 0, 0])
    # a voxel outside the lattice on every interpolated axis: the plain mix's bytes under that corner node
    if name == "square":
        assert same_bits(out[:, :3, :, :5], corners[0, 0, 0][:, :3, :, :5]) and same_bits(out[:, 54:, :, 51:], corners[3, 0, 2][:, 54:, :, 51:])
    # the records: consecutive ids behind the sources, the grid, the kind, the tag, the newest source's block
    assert first == ids[-1] + 1 and int(newest_info(bf.library()).frame_id) == first + M - 1
    source_block = int(bf.frame_info(ids[-1]).parameter_block)
    rows, _ = bf.score_last_frames(M)
    pz, py, px = out.shape[1:]
    for j in range(M):
        info = bf.frame_info(first + j)
        assert (int(info.frame_id), tuple(info.points), int(info.parameter_block)) == (first + j, (px, py, pz), source_block)
        assert int(info.data_kind) == int(D.Float32 if real else D.Float32Complex)
        assert (int(rows[j].frame_id), int(rows[j].image_plane_tag), int(rows[j].parameter_block)) == (first + j, 5, source_block)
    t = P.HipFrameTimings()
    assert bf.library().beamformer_hip_get_last_frame_timings(C.byref(t)) and t.stage_count == 0 and t.das_voxels == 0
    assert same_bits(bf.copy_frame(first + M - 1), out[M - 1])
    # the kernel's two shapes (hook BLEND_SHAPE: 0 the corners outermost, 1 each source loaded once; 1 applies where the lattice has one
    # node along y, elsewhere 0 runs): the same bytes
    for shape in (0, 1):
        bflib.set_hook("BLEND_SHAPE", shape)
        shaped, _, _, _ = field_mix(which, K, W, lattice, tag=5)
        assert same_bits(shaped, want), shape
    bflib.set_hook("BLEND_SHAPE", None)


def test_equal_tables_at_every_node_give_the_plain_mix(bflib):
    lattice = LATTICES["square"]
    K, M = 17, 5
    one = weights(M, K, 8300)
    W = np.broadcast_to(one, (4, 1, 3, M, K)).copy()
    acq = block("square")
    ensemble("square", K)
    bf.mix_last_frames(K, one)
    plain = bf.get_last_frames(acq.bp, M).copy()
    out, _, _, _ = field_mix("square", K, W, lattice)
    assert np.isfinite(plain.view(np.float32)).all()
    print(f"  {int((out.view(np.uint32) != plain.view(np.uint32)).sum())} of {out.view(np.uint32).size} words differ from the plain mix")
    assert same_bits(out, plain)
    # the same call twice: equal bytes
    again, _, _, _ = field_mix("square", K, W, lattice)
    assert again.tobytes() == out.tobytes()


def test_an_output_depends_on_its_own_rows_only(bflib):
    lattice = LATTICES["beyond"]
    K, M = 2, 17
    W = node_weights(lattice, M, K, 8400)
    out, _, _, _ = field_mix("plane", K, W, lattice)
    for j in (0, 7, 15, 16):
        alone, _, _, _ = field_mix("plane", K, W[:, :, :, j:j + 1], lattice)
        assert same_bits(alone[0], out[j]), j
    # and the peaks of the outputs are found as any frame's are
    out, first, ids, _ = field_mix("plane", K, W, lattice)
    thresholds = [0.5 * float(np.abs(f).max()) for f in out]
    rows, peaks, found = check_call(list(out), thresholds, cap=64, what="field mix")
    assert all(r["found"] >= 1 for r in found)


def test_field_mix_over_the_nan_block(bflib):
    lattice = LATTICES["nan"]
    K, M = 3, 2
    W = node_weights(lattice, M, K, 8500)
    corners = corners_by_the_plain_mix("nan", K, W)
    nan = np.isnan(corners.view(np.float32)).any(axis=(0, 1, 2, 3))
    want = ref.blend(corners, lattice["first"], lattice["step"])
    out, _, _, _ = field_mix("nan", K, W, lattice)
    print(f"  {int(np.isnan(out.view(np.float32)).sum())} NaN floats of {out.view(np.float32).size}")
    assert nan.sum() >= 64 and same_bits(out, want)
    for shape in (0, 1):
        bflib.set_hook("BLEND_SHAPE", shape)
        assert same_bits(field_mix("nan", K, W, lattice)[0], want), shape
    bflib.set_hook("BLEND_SHAPE", None)
    # a voxel that is not finite in a source is not finite in every output
    frames, _ = ensemble("nan", K)
    bad = np.isnan(frames).any(axis=0)
    assert np.isnan(out.real[:, bad]).all() and np.isnan(out.imag[:, bad]).all() and np.isfinite(out.real[:, ~bad]).all()


# ---- the loop on planted frames ----

def planted_burst(stack):
    """K planted frames by one burst push: (the acquisition of frame 0, frames (K, Z, Y, X)); frame k IS planted array k"""
    blocks = [planted.block(values, "planted_two_clutter") for values in stack]
    frames = bf.beamform_burst(blocks[0].bp, np.stack([acq.rf for acq in blocks]), blocks[0].filters).copy()
    for k, values in enumerate(stack):
        assert planted.same(frames[k], planted.expected(values)), f"frame {k} of the burst is not planted array {k}"
    return blocks[0], frames


def test_the_block_wise_loop_on_the_two_clutter_ensemble(bflib):
    """burst -> lattice_boxes -> gram_boxes -> projector a box -> mix_field on the planted two-clutter ensemble of the host test, K = 8,
    against the reference within the bounds tests/ensemble_ref.py derives; and the residual clutter on the device shows the gap between
    the global and the block-wise rank-1 filter that tests/test_block_filter_host.py established on the reference"""
    values, parts = ref.two_clutter_ensemble()
    K = values.shape[0]
    points = (values.shape[3], values.shape[2], values.shape[1])
    nodes, first_node, step, half = ref.two_clutter_lattice(points)
    acq, frames = planted_burst(list(values))
    boxes = bflib.lattice_boxes(points, nodes, first_node, step, half)
    want_boxes = ref.lattice_boxes(points, nodes, first_node, step, half)
    assert [(tuple(b.first), tuple(b.count)) for b in boxes] == want_boxes
    grams, infos, _ = bflib.gram_boxes_last_frames(K, boxes)
    W = np.empty((1, 1, 2, K, K), np.complex64)
    for n, (expected, voxels, non_finite, bound) in enumerate(ref.gram_boxes(list(frames), want_boxes)):
        over = np.maximum(np.abs(grams[n].real - expected.real), np.abs(grams[n].imag - expected.imag))
        print(f"  box {n}: {int(infos[n].voxels)} voxels, gram worst error {over.max():.3e} = {float((over / bound).max()):.3f} of its bound")
        assert (int(infos[n].voxels), int(infos[n].non_finite)) == (voxels, non_finite) == (48, 0) and (over <= bound).all()
        W[0, 0, n], eigenvalues = bflib.clutter_projector(grams[n], 1)
        assert eigenvalues[0] > 1e3 * eigenvalues[1] > 0
    first, _ = bflib.mix_field_last_frames(K, W, first_node, step)
    assert first == int(infos[0].first_frame_id) + K
    block_out = bflib.get_last_frames(acq.bp, K).copy()
    expected, bound = ref.mix_field(list(frames), W, first_node, step)
    over = np.maximum(np.abs(block_out.real - expected.real), np.abs(block_out.imag - expected.imag))
    print(f"  block-wise frames: worst error {over.max():.3e}, {float((over / bound).max()):.3f} of its bound")
    assert (over <= bound).all()
    # the global filter on the same frames
    acq, again = planted_burst(list(values))
    assert again.tobytes() == frames.tobytes()
    G, _, _ = bflib.gram_last_frames(K)
    W_global, _ = bflib.clutter_projector(G, 1)
    bflib.mix_last_frames(K, W_global)
    global_out = bflib.get_last_frames(acq.bp, K).copy()
    before, left_global, left_block = ref.clutter_left(frames, parts), ref.clutter_left(global_out, parts), ref.clutter_left(block_out, parts)
    print(f"  clutter energy {before:.4e}; left by the global rank-1 filter {left_global:.4e}, by the two-node block-wise one {left_block:.4e} "
          f"(ratio {left_block / left_global:.3e})")
    assert left_global > 0.2 * before and left_block < 1e-3 * left_global
