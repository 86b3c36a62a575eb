"""The ensemble filter on the device (beamformer_hip_gram_last_frames, beamformer_hip_mix_last_frames; csrc/ensemble.hip) and the loop
burst -> gram -> projector -> mix -> peaks -> views.  Frames are produced by ordinary pushes and downloaded with
beamformer_get_last_frames; the expected values are the numpy reference (tests/ensemble_ref.py) applied to those downloaded arrays --
parity of the frames themselves is other tests' business.

The bars are derived, not measured (tests/ensemble_ref.py returns them with the values).  Gram: the products of widened floats are
exact, a voxel term is one rounding and the running sum V more: (V + 2) 2^-53 sum (|r_j| + |i_j|)(|r_k| + |i_k|), for each of the two
parts of an entry.  Mix: an output float is a float32 fmaf chain of 2K terms: (2K + 2) 2^-24 sum_k (|Wre| + |Wim|)(|re_k| + |im_k|).
Counts, ids, grids, the Hermitian mirror and every zero the definition promises are asked exactly.  Every test prints what it measured
before it asserts."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from ogl_beamforming_amd import configs as cfg
from ogl_beamforming_amd import lib as bf
from ogl_beamforming_amd import params as P
from tests import ensemble_ref as ref
from tests import variants_cases as vc
from tests.test_gpu_frame_metrics import block as metrics_block, newest_info, region_of
from tests.test_gpu_frame_peaks import check_call

pytestmark = pytest.mark.gpu
E = P.LibError
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = P.DataKind
GRIDS = {"plane": ((33, 1, 7), vc.LO, vc.HI, True), "square": ((64, 1, 64), vc.LO, vc.HI, True),
         "volume": ((9, 5, 6), vc.LO3, vc.HI3, True), "real": ((33, 1, 7), vc.LO, vc.HI, False)}
# boxes with odd offsets and odd extents: no multiple of a mask word, rows that are no whole lines
BOXES = {"plane": ((1, 0, 1), (29, 1, 5)), "square": ((3, 0, 5), (57, 1, 51)), "volume": ((1, 1, 1), (7, 3, 5)), "real": ((5, 0, 3), (27, 1, 3))}


@pytest.fixture(autouse=True)
def automatic_path(bflib):
    L = bflib.library()
    L.beamformer_set_global_timeout(0xFFFFFFFF)
    L.beamformer_hip_set_das_path(0)
    yield
    L.beamformer_hip_set_das_path(0)


@functools.lru_cache(maxsize=None)
def block(which):
    """16 channels x 2 plane waves of float32 RF straight into DAS on the grid `which` names; "nan": the coherency-weighted plane of the
    frame metrics tests, which leaves NaN where no term passed"""
    if which == "nan":
        return metrics_block("D")
    points, lo, hi, iq = GRIDS[which]
    return cfg.rca("ensemble_" + which, 16, 2, 256, points, lo, hi, seed=7500, interp=P.InterpolationMode.Linear, demodulate=False,
                   data_kind=D.Float32Complex if iq else D.Float32, angles=np.array([-6.0, 6.0]), kind=P.AcquisitionKind.RCA_TPW)


@functools.lru_cache(maxsize=None)
def rf_frames(which, K):
    acq = block(which)
    rng = np.random.default_rng(7600 + K)
    return rng.normal(0.0, 1.0, (K,) + acq.rf.shape).astype(acq.rf.dtype)


def ensemble(which, K):
    """K frames of the grid by one burst push (one: a single push): (frames (K, Z, Y, X), their ids)"""
    acq, rf = block(which), rf_frames(which, K)
    if K == 1:
        frames = bf.beamform(acq.bp, rf[0], acq.filters).copy()[None]
    else:
        frames = bf.beamform_burst(acq.bp, rf, acq.filters).copy()
    newest = int(newest_info(bf.library()).frame_id)
    return frames, list(range(newest - K + 1, newest + 1))


def check_gram(frames, ids, box=None, what=""):
    K = len(frames)
    real = not np.iscomplexobj(frames)
    G, info, ms = bf.gram_last_frames(K, region_of(box))
    expected, voxels, non_finite, bound = ref.gram(list(frames), box)
    pz, py, px = frames[0].shape
    over = np.maximum(np.abs(G.real - expected.real), np.abs(G.imag - expected.imag))
    worst = float((over / np.maximum(bound, 1e-300)).max()) if voxels else 0.0
    print(f"  {what}: K {K} {(px, py, pz)} {'real' if real else 'complex'} box {box}: voxels {int(info.voxels)} ({voxels}), non-finite "
          f"{int(info.non_finite)} ({non_finite}), worst error {over.max():.3e} = {worst:.3f} of its bound, {ms * 1e3:.1f} us")
    assert G.shape == (K, K) and G.dtype == np.complex128 and ms > 0
    assert (int(info.count), int(info.data_kind)) == (K, int(D.Float32 if real else D.Float32Complex))
    assert tuple(info.points) == (px, py, pz) and int(info.first_frame_id) == ids[0]
    assert tuple(info.region_first) == (tuple(box[0]) if box else (0, 0, 0)) and tuple(info.region_count) == (tuple(box[1]) if box else (px, py, pz))
    assert (int(info.voxels), int(info.non_finite)) == (voxels, non_finite)
    # the mirror: equal real parts bit for bit, opposite imaginary parts, a real diagonal
    assert np.array_equal(G.real.view(np.uint64), G.real.T.copy().view(np.uint64))
    assert np.array_equal(G.imag, -G.imag.T) and not np.diagonal(G).imag.any()
    if real:
        assert not G.imag.any()
    assert (over <= bound).all()
    return G, bound


@pytest.mark.parametrize("K", [1, 2, 3, 17, 65])
@pytest.mark.parametrize("which", ["plane", "square", "volume", "real"])
def test_gram_of_a_burst(which, K, bflib):
    frames, ids = ensemble(which, K)
    assert frames.shape[0] == K and frames.shape[1:] == GRIDS[which][0][::-1] and np.iscomplexobj(frames) == GRIDS[which][3]
    G, _ = check_gram(frames, ids, what=which)
    check_gram(frames, ids, BOXES[which], what=which + " box")
    # the frames are far more than any tolerance apart: a kernel that reads one frame for every row fails above
    if K > 1:
        assert abs(G[0, 1]) < 0.9 * np.sqrt(G[0, 0].real * G[1, 1].real)
    # the same call twice: equal bytes
    again, _, _ = bflib.gram_last_frames(K)
    assert G.tobytes() == again.tobytes()


def test_gram_leaves_out_the_voxels_that_are_not_finite_in_some_frame(bflib):
    frames, ids = ensemble("nan", 3)
    nan = np.isnan(frames).any(axis=0)
    print(f"  {int(nan.sum())} of {nan.size} voxels NaN in some frame")
    assert nan.sum() >= 64 and 4 * (~nan).sum() >= nan.size
    G, _ = check_gram(frames, ids, what="nan")
    assert np.isfinite(G.real).all() and np.isfinite(G.imag).all()
    check_gram(frames, ids, ((1, 0, 3), (21, 1, 35)), what="nan box")
    # a box of NaN voxels only: no voxel, a zero matrix
    z, x = np.argwhere(nan[:, 0, :])[0]
    box = ((int(x), 0, int(z)), (1, 1, 1))
    G, info, _ = bflib.gram_last_frames(3, region_of(box))
    assert (int(info.voxels), int(info.non_finite)) == (0, 1) and not G.any()


def test_gram_of_the_octants_sums_to_the_whole(bflib):
    frames, ids = ensemble("volume", 3)
    whole, bound = check_gram(frames, ids, what="volume")
    total = np.zeros_like(whole)
    for z0, nz in ((0, 3), (3, 3)):
        for y0, ny in ((0, 2), (2, 3)):
            for x0, nx in ((0, 4), (4, 5)):
                part, _, _ = bflib.gram_last_frames(3, region_of(((x0, y0, z0), (nx, ny, nz))))
                total += part
    over = np.maximum(np.abs(total.real - whole.real), np.abs(total.imag - whole.imag))
    print(f"  octants against the whole: worst {over.max():.3e}, {float((over / bound).max()):.3f} of the bound")
    assert (over <= 2 * bound).all()


# ---- mix ----

def weights(M, K, seed, real=False):
    rng = np.random.default_rng(seed)
    if real:
        return rng.standard_normal((M, K)).astype(np.float32).astype(np.complex64)
    return (rng.standard_normal((M, K)) + 1j * rng.standard_normal((M, K))).astype(np.complex64)


def check_mix(which, frames, ids, W, tag=0, what=""):
    """mix the len(frames) newest frames under W and check the outputs and their records; returns (outputs, first id)"""
    acq = block(which)
    K, M = len(frames), W.shape[0]
    real = not np.iscomplexobj(frames)
    source_block = int(bf.frame_info(ids[-1]).parameter_block)
    first, ms = bf.mix_last_frames(K, W, tag=tag)
    out = bf.get_last_frames(acq.bp, M).copy()
    expected, bound = ref.mix(list(frames), W)
    finite = np.isfinite(expected.real) & np.isfinite(expected.imag) if not real else np.isfinite(expected)
    if real:
        over = np.abs(out.astype(np.float64) - expected)
    else:
        over = np.maximum(np.abs(out.real.astype(np.float64) - expected.real), np.abs(out.imag.astype(np.float64) - expected.imag))
    ratio = np.where(finite, over / np.maximum(bound, 1e-300), 0.0)
    print(f"  {what}: K {K} -> M {M} {'real' if real else 'complex'}: worst error {np.where(finite, over, 0).max():.3e} = {ratio.max():.3f} of its bound, "
          f"{int((~finite).sum())} non-finite, {ms * 1e3:.1f} us")
    assert out.shape == (M,) + frames.shape[1:] and out.dtype == frames.dtype and ms > 0
    assert (over[finite] <= bound[finite]).all()
    # a voxel that is not finite in some input is not finite in every output
    got_finite = np.isfinite(out.real) & np.isfinite(out.imag) if not real else np.isfinite(out)
    assert np.array_equal(got_finite, finite)
    # the records: consecutive ids behind the sources, the grid, the kind, the tag, the newest source's block
    assert first == ids[-1] + 1 and int(newest_info(bf.library()).frame_id) == first + M - 1
    rows, _ = bf.score_last_frames(M)
    pz, py, px = frames.shape[1:]
    for j in range(M):
        info = bf.frame_info(first + j)
        assert (int(info.frame_id), tuple(info.points), int(info.parameter_block)) == (first + j, (px, py, pz), source_block)
        assert int(info.data_kind) == int(D.Float32 if real else D.Float32Complex)
        assert (int(rows[j].frame_id), int(rows[j].image_plane_tag), int(rows[j].parameter_block)) == (first + j, tag, source_block)
    # their rows of the timing table: no stages, no DAS voxels
    t = P.HipFrameTimings()
    assert bf.library().beamformer_hip_get_last_frame_timings(C.byref(t)) and t.stage_count == 0 and t.das_voxels == 0
    # a source frame is still served by its id
    assert np.array_equal(bf.copy_frame(ids[0]).view(np.uint32), frames[0].view(np.uint32))
    return out, first


@pytest.mark.parametrize("K,M", [(1, 1), (3, 3), (17, 5), (5, 17), (65, 65)])
def test_mix_of_a_burst(K, M, bflib):
    frames, ids = ensemble("plane", K)
    before = bytes(bflib.last_burst_info()) if K > 1 else None
    out, first = check_mix("plane", frames, ids, weights(M, K, 7700 + K), tag=3, what="plane")
    if K > 1 and M < 32:
        # the newest burst's info is unchanged behind the outputs
        assert bytes(bflib.last_burst_info()) == before
    # the same call twice: two runs of equal bytes (the K newest frames are now the outputs: mix the sources again by pushing them again)
    frames2, ids2 = ensemble("plane", K)
    assert np.array_equal(frames2.view(np.uint32), frames.view(np.uint32))
    again, _ = check_mix("plane", frames2, ids2, weights(M, K, 7700 + K), tag=3, what="plane again")
    assert out.tobytes() == again.tobytes()


def test_mix_of_real_frames(bflib):
    frames, ids = ensemble("real", 5)
    assert frames.dtype == np.float32
    check_mix("real", frames, ids, weights(3, 5, 7801, real=True), what="real")
    # a nonzero imaginary weight on real frames is refused, and nothing changes
    frames, ids = ensemble("real", 5)
    W = weights(3, 5, 7801, real=True)
    W[2, 4] += 1e-30j
    first, ms = C.c_uint32(77), C.c_float(-1.0)
    assert not bflib.library().beamformer_hip_mix_last_frames(5, W.ctypes.data_as(C.POINTER(C.c_float)), 3, 0, C.byref(first), C.byref(ms))
    assert bflib.last_error()[0] == E.InvalidAccess and first.value == 77 and ms.value == -1.0
    assert int(newest_info(bflib.library()).frame_id) == ids[-1]


def test_mix_by_a_permutation_by_zero_and_over_nan_voxels(bflib):
    frames, ids = ensemble("nan", 5)
    nan = np.isnan(frames).any(axis=0)
    assert nan.sum() >= 64
    order = [3, 0, 4, 1, 2]
    out, _ = check_mix("nan", frames, ids, np.eye(5, dtype=np.complex64)[order], what="permutation")
    for j, k in enumerate(order):
        assert np.array_equal(out[j][~nan], frames[k][~nan])                       # by value (-0 may come back +0)
    assert np.isnan(out.real[:, nan]).all() and np.isnan(out.imag[:, nan]).all()  # no weight is skipped: 0 * NaN
    frames, ids = ensemble("nan", 5)
    out, _ = check_mix("nan", frames, ids, np.zeros((2, 5), np.complex64), what="zero")
    assert not out[:, ~nan].any() and np.isnan(out.real[:, nan]).all()


# ---- the loop: burst -> gram -> projector -> mix -> peaks -> views ----

LOOP_POINTS = (32, 1, 48)


@functools.lru_cache(maxsize=None)
def loop_case():
    """8 RF frames a_k R0 + b_k R1 of two seeded float32 RF frames, |a| 100 times |b|: a strong common component (tissue) and a weak one"""
    acq = cfg.rca("ensemble_loop", 16, 2, 256, LOOP_POINTS, vc.LO, vc.HI, seed=7900, interp=P.InterpolationMode.Linear, demodulate=False,
                  data_kind=D.Float32Complex, angles=np.array([-6.0, 6.0]), kind=P.AcquisitionKind.RCA_TPW)
    rng = np.random.default_rng(7901)
    r0, r1 = (rng.normal(0.0, 1.0, acq.rf.shape).astype(np.float32) for _ in range(2))
    a = 10.0 * (1.0 + 0.05 * np.cos(np.arange(8)))
    b = 0.1 * np.array([1, -1, 1, 1, -1, -1, 1, -1], np.float64)
    rf = np.stack([(a[k] * r0 + b[k] * r1).astype(np.float32) for k in range(8)])
    return acq, rf


def test_the_clutter_filter_loop(bflib):
    acq, rf = loop_case()
    burst = bflib.beamform_burst(acq.bp, rf, acq.filters).copy()
    assert burst.shape == (8, 48, 1, 32) and np.iscomplexobj(burst) and np.isfinite(burst.real).all()
    source_energy = [float(r.sum_abs2) for r in bflib.score_last_frames(8)[0]]
    G, info, _ = bflib.gram_last_frames(8)
    W, values = bflib.clutter_projector(G, 1)
    print(f"  eigenvalues {values}")
    assert values[0] > 1e3 * values[1] > 0
    first, _ = bflib.mix_last_frames(8, W)
    assert first == int(info.first_frame_id) + 8
    mixed = bflib.get_last_frames(acq.bp, 8).copy()
    expected, bound = ref.mix(list(burst), W)
    over = np.maximum(np.abs(mixed.real - expected.real), np.abs(mixed.imag - expected.imag))
    print(f"  mixed frames: worst error {over.max():.3e}, {float((over / bound).max()):.3f} of its bound")
    assert (over <= bound).all()
    rows, _ = bflib.score_last_frames(8)
    mixed_energy = [float(r.sum_abs2) for r in rows]
    print(f"  energy: sources {source_energy}, mixed {mixed_energy}")
    assert max(mixed_energy) < min(source_energy)
    thresholds = [0.5 * float(r.max_abs) for r in rows]
    peak_rows, peaks, found = check_call(list(mixed), thresholds, cap=64, what="mixed")
    assert all(r["found"] >= 1 for r in found)
    few = [peaks[int(peak_rows[7].first) + k] for k in range(min(3, int(peak_rows[7].stored)))]
    views = bflib.peaks_to_views(list(acq.bp.das_voxel_transform), LOOP_POINTS, few, (17, 1, 17), (4.0, 0.0, 4.0), use_offsets=True)
    patches = bflib.beamform_burst_views(acq.bp, rf, views, acq.filters)
    assert len(patches) == len(few) and all(len(p) == 8 and p[0].shape == (17, 1, 17) for p in patches)
    assert int(newest_info(bflib.library()).frame_id) - int(bflib.last_burst_views_info().first_frame_id) + 1 == 8 * len(few)


# ---- refusals that need a device ----

def newest_id(L):
    """the newest frame's id; None while the newest push is a tombstone"""
    info = P.HipFrameInfo()
    return int(info.frame_id) if L.beamformer_hip_get_last_frame_info(C.byref(info)) else None


def refused_both(L, K, kind, region=None):
    """both device calls refuse `K` frames with this error kind, write nothing and queue nothing (a region: the Gram call alone)"""
    gram = np.full((K, K), -7.0 - 7.0j, np.complex128)
    untouched = gram.tobytes()
    info = P.HipEnsembleInfo()
    newest = newest_id(L)
    assert not L.beamformer_hip_gram_last_frames(K, None if region is None else C.byref(region), gram.ctypes.data_as(C.POINTER(C.c_double)), C.byref(info), None)
    assert bf.last_error()[0] == kind and gram.tobytes() == untouched and not bytes(info).strip(b"\0")
    if region is None:
        first = C.c_uint32(77)
        W = np.eye(K, dtype=np.complex64)
        assert not L.beamformer_hip_mix_last_frames(K, W.ctypes.data_as(C.POINTER(C.c_float)), K, 0, C.byref(first), None)
        assert bf.last_error()[0] == kind and first.value == 77
    assert newest_id(L) == newest


def test_refusals(bflib):
    L = bflib.library()
    # more frames asked for than were ever queued: a fresh context with two frames
    L.beamformer_hip_shutdown()
    assert L.beamformer_hip_set_devices((C.c_int32 * 1)(0), 1)
    frames, ids = ensemble("plane", 2)
    assert ids == [0, 1]
    refused_both(L, 3, E.InvalidAccess)
    check_gram(frames, ids, what="two frames")
    # a box outside the frames, a zero extent
    for box in (((0, 0, 0), (34, 1, 7)), ((1, 0, 0), (33, 1, 7)), ((0, 0, 7), (1, 1, 1)), ((0, 0, 0), (33, 0, 7)), ((0xFFFFFFFF, 0, 0), (2, 1, 1))):
        refused_both(L, 2, E.InvalidAccess, bflib.frame_region(*box))
    # frames of two grids, frames of two kinds on one grid
    a, b, r = block("plane"), block("square"), block("real")
    bflib.beamform(b.bp, rf_frames("square", 1)[0], b.filters)
    refused_both(L, 2, E.DataSizeMismatch)
    refused_both(L, 3, E.DataSizeMismatch)
    bflib.beamform(a.bp, rf_frames("plane", 1)[0], a.filters)
    bflib.beamform(r.bp, rf_frames("real", 1)[0], r.filters)
    refused_both(L, 2, E.DataSizeMismatch)
    # a tombstone among the K: a variants push that fails at its DAS stage (das path flag 0x2000) leaves three, without any device fault
    acq = metrics_block("A")
    variants = vc.candidates(acq.bp)
    bflib.beamform_variants(acq.bp, acq.rf, variants, acq.filters)
    rf = np.ascontiguousarray(acq.rf)
    L.beamformer_hip_set_das_path(P.HIP_DAS_PATH_FAIL_VIEWS_DAS)
    assert not L.beamformer_hip_push_data_variants_with_compute(rf.ctypes.data_as(C.c_void_p), rf.nbytes, (P.HipDasVariant * 3)(*variants), 3, 0, 0)
    L.beamformer_hip_set_das_path(0)
    refused_both(L, 1, E.InvalidAccess)
    refused_both(L, 4, E.InvalidAccess)
    single = bflib.beamform(acq.bp, acq.rf, acq.filters).copy()
    refused_both(L, 2, E.InvalidAccess)
    check_gram(single[None], [int(newest_info(L).frame_id)], what="behind the tombstones")


def test_several_devices_are_refused(bflib):
    L = bflib.library()
    acq = vc.separable_volume()
    try:
        L.beamformer_hip_shutdown()
        assert L.beamformer_hip_set_devices((C.c_int32 * 2)(0, 0), 2)
        bflib.beamform(acq.bp, acq.rf, acq.filters)
        assert L.beamformer_hip_get_device_count() == 2
        refused_both(L, 1, E.InvalidAccess)
    finally:
        L.beamformer_hip_shutdown()
        assert L.beamformer_hip_set_devices((C.c_int32 * 1)(0), 1)
    frames, ids = ensemble("plane", 2)
    check_gram(frames, ids, what="one device again")


def test_the_ring_a_run_that_wraps_and_one_that_would_reuse_its_sources():
    """a 1 MiB frame ring in a process of its own (the ring is sized once per process): tests/ensemble_wrap_worker.py"""
    env = dict(os.environ, BEAMFORMER_HIP_FRAME_RING_BYTES=str(1 << 20))
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ensemble_wrap_worker.py")], env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "refused" in run.stdout, run.stdout
