"""What the frame-operation tests share: the acquisitions and ensembles that fill the frame ring (built once: the builders are cached and
hold beamformed frames), map placements, and each operation's check of one call against its reference
(tests/*_ref.py).  Imports the reference modules, tests/planted.py and no test module."""
import ctypes as C
import functools

import numpy as np

from ogl_beamforming_amd import configs as cfg
from ogl_beamforming_amd import lib as bf
from ogl_beamforming_amd import params as P
from tests import autocorr_ref
from tests import block_filter_ref
from tests import ensemble_ref
from tests import frame_metrics_ref
from tests import frame_peaks_ref
from tests import frame_quantiles_ref
from tests import localisation_ref
from tests import motion_ref
from tests import planted
from tests import spatial_ref
from tests import track_chains_ref
from tests import track_draw_ref
from tests import tracks_ref
from tests import variants_cases as vc
from tests import warp_ref
from tests.frame_info import newest_info


BOX = ((3, 2, 1), (10, 13, 30))            # 3900 voxels of 16 x 16 x 32: no multiple of a wave or a block, all three gradients cut


@functools.lru_cache(maxsize=None)
def metrics_block(which):
    """the acquisitions of the blocks A .. D, built once"""
    if which == "A":
        return vc.block("linear", iq=True, cw=False)
    if which == "B":
        return vc.block("linear", iq=False, cw=False)
    if which == "C":
        return vc.separable_volume()
    if which == "forces":
        return vc.forces_block()
    points, lo, hi = {"D": ((24, 1, 40), (-6e-3, 0, 0.2e-3), (6e-3, 0, 5.5e-3)),
                      "D3": ((16, 16, 32), (-12e-3, -12e-3, 0.5e-3), (12e-3, 12e-3, 5.5e-3))}[which]
    return cfg.rca("frame_metrics_nan_" + which, 16, 2, 256, points, lo, hi, seed=7300, interp=P.InterpolationMode.Linear, cw=True,
                   demodulate=False, data_kind=P.DataKind.Float32Complex, angles=np.array([-6.0, 6.0]), kind=P.AcquisitionKind.RCA_TPW)


def variants_push(which):
    """a variants push of the block under variants_cases.candidates: (frames (3, Z, Y, X), their ids)"""
    acq = metrics_block(which)
    frames = bf.beamform_variants(acq.bp, acq.rf, vc.candidates(acq.bp), acq.filters).copy()
    newest = int(newest_info(bf.library()).frame_id)
    return frames, [newest - 2, newest - 1, newest]


def region_of(box):
    return None if box is None else bf.frame_region(*box)


def within(got, expected, bar, what):
    print(f"    {what}: {got!r} against {expected!r}, off by {abs(got - expected):.3e} (bar {bar:.3e})")
    assert abs(got - expected) <= bar, what


def check_row(row, frame, box=None, what=""):
    """one row against the reference applied to the downloaded frame"""
    real = not np.iscomplexobj(frame)
    r = frame_metrics_ref.metrics(frame, *(box if box else (None, None)))
    print(f"  {what}: frame {int(row.frame_id)} {tuple(row.points)} {'real' if real else 'complex'} box {r['region_first']} + {r['region_count']}")
    # identity: the record's
    info = bf.frame_info(int(row.frame_id))
    assert tuple(row.points) == tuple(info.points) == r["points"] and row.data_kind == info.data_kind
    assert row.data_kind == int(P.DataKind.Float32 if real else P.DataKind.Float32Complex) and row.parameter_block == info.parameter_block
    assert tuple(row.region_first) == r["region_first"] and tuple(row.region_count) == r["region_count"] and row.reserved == 0
    # counts: exact
    assert (int(row.voxels), int(row.non_finite), [int(n) for n in row.gradient_pairs]) == (r["voxels"], r["non_finite"], r["gradient_pairs"])
    assert row.voxels + row.non_finite == int(np.prod(r["region_count"]))
    # sums
    s2 = r["sum_abs2"]
    for name, bar in (("sum_abs", 1e-6), ("sum_abs2", 2e-6), ("sum_abs4", 4e-6)):
        within(getattr(row, name), r[name], (1e-12 if real else bar) * r[name], name)
    for axis in range(3):
        bar = 1e-12 * r["gradient2"][axis] if real else 2e-6 * np.sqrt(r["gradient2"][axis] * s2) + 1e-12 * s2
        within(row.gradient2[axis], r["gradient2"][axis], bar, f"gradient2[{axis}]")
    # the maximum
    within(float(row.max_abs), r["max_abs"], 3e-7 * r["max_abs"], "max_abs")
    index = tuple(int(v) for v in row.max_index)
    if real or not r["voxels"]:
        assert index == r["max_index"], (index, r["max_index"])
    else:
        local = tuple(i - f for i, f in zip(index, r["region_first"]))
        assert all(0 <= i < c for i, c in zip(local, r["region_count"])), index
        at = float(r["magnitude"][local[2], local[1], local[0]])
        print(f"    max_index {index} (reference {r['max_index']}): reference magnitude there {at!r}")
        assert at >= r["max_abs"] * (1 - 3e-7), (at, r["max_abs"])
    return r


def fraction_of_max(frames, fraction):
    """per frame: `fraction` of its largest finite magnitude, as the float32 the call is given"""
    out = []
    for f in frames:
        m = frame_metrics_ref.magnitude(f)
        out.append(float(np.float32(fraction) * m[np.isfinite(m)].max()))
    return out


CAP = 4096


def ulps(a, b):
    """distance in units in the last place of two arrays of finite non-negative float32"""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def peak_records(row, peaks):
    return np.frombuffer(bytes(peaks), np.dtype(P.HipFramePeak))[int(row.first):int(row.first) + int(row.stored)]


def check_frame(row, peaks, frame, threshold, box=None, cap=CAP, first=None, what=""):
    """one frame's row and records against the reference applied to the downloaded frame"""
    real = not np.iscomplexobj(frame)
    r = frame_peaks_ref.peaks(frame, threshold, *(box if box else (None, None)), cap=cap)
    pz, py, px = frame.shape
    print(f"  {what}: frame {int(row.frame_id)} {(px, py, pz)} {'real' if real else 'complex'} threshold {threshold!r} box {box}: "
          f"found {int(row.found)} ({r['found']}), above {int(row.above_threshold)} ({r['above_threshold']}), stored {int(row.stored)} ({r['stored']})")
    info = bf.frame_info(int(row.frame_id))
    assert tuple(row.points) == tuple(info.points) == (px, py, pz) and row.data_kind == info.data_kind and row.parameter_block == info.parameter_block
    assert row.data_kind == int(P.DataKind.Float32 if real else P.DataKind.Float32Complex)
    assert tuple(row.region_first) == (tuple(box[0]) if box else (0, 0, 0)) and tuple(row.region_count) == (tuple(box[1]) if box else (px, py, pz))
    assert row.threshold == np.float32(threshold)
    assert (int(row.found), int(row.above_threshold), int(row.stored)) == (r["found"], r["above_threshold"], r["stored"])
    if first is not None:
        assert int(row.first) == first
    got = peak_records(row, peaks)
    assert np.array_equal(got["index"], r["index"]), (got["index"][:8], r["index"][:8])
    assert np.array_equal(got["fitted"], r["fitted"])
    if real:
        assert np.array_equal(got["magnitude"].view(np.uint32), r["magnitude"].view(np.uint32))
        assert np.array_equal(got["offset"].view(np.uint32), r["offset"].view(np.uint32))
    elif len(got):
        away = ulps(got["magnitude"], r["magnitude"])
        print(f"    magnitude: {int((away == 0).sum())} of {len(away)} bit-equal, worst {int(away.max())} ulp")
        assert away.max() <= 1, f"magnitude {int(away.max())} ulp from the reference's (bar 1)"
        # den per axis from the reference's magnitudes, for the bar
        m = np.pad(frame_metrics_ref.magnitude(frame), 1, constant_values=np.float32(np.nan)).astype(np.float64)
        x, y, z = (r["index"][:, a].astype(np.int64) + 1 for a in range(3))
        m0 = m[z, y, x]
        for axis, (dz, dy, dx) in enumerate(((0, 0, 1), (0, 1, 0), (1, 0, 0))):
            on = (r["fitted"] >> axis & 1).astype(bool)
            den = (m[z - dz, y - dy, x - dx] + m[z + dz, y + dy, x + dx]) - 2 * m0
            bar = 8 * 2.0 ** -23 * m0[on] / np.abs(den[on]) + 2.0 ** -20
            off = np.abs(got["offset"][on, axis].astype(np.float64) - r["offset"][on, axis].astype(np.float64))
            if on.any():
                print(f"    offset[{axis}]: {int(on.sum())} fitted, worst {off.max():.3e} (its bar {bar[np.argmax(off)]:.3e}), "
                      f"{int((got['offset'][on, axis] == r['offset'][on, axis]).sum())} bit-equal")
            assert (off <= bar).all(), axis
            assert not got["offset"][~on, axis].any()
        assert (np.abs(got["offset"]) <= 0.5).all(), f"offset {float(np.abs(got['offset']).max())!r} (bar 0.5)"
    return r


def check_peaks(frames, thresholds, box=None, cap=CAP, what=""):
    """find the peaks of the len(frames) newest frames and check every frame; thresholds: one number or one a frame"""
    rows, peaks, ms = bf.find_peaks_last_frames(len(frames), thresholds, cap, region_of(box))
    each = [thresholds] * len(frames) if np.ndim(thresholds) == 0 else list(thresholds)
    first, out = 0, []
    for k, frame in enumerate(frames):
        out.append(check_frame(rows[k], peaks, frame, each[k], box, cap, first, what=f"{what} {k}"))
        first += int(rows[k].stored)
    assert len(peaks) == first and ms > 0
    return rows, peaks, out


D = P.DataKind
GRIDS = {"plane": ((33, 1, 7), vc.LO, vc.HI, True), "square": ((64, 1, 64), vc.LO, vc.HI, True),
         "volume": ((9, 5, 6), vc.LO3, vc.HI3, True), "real": ((33, 1, 7), vc.LO, vc.HI, False)}
# boxes with odd offsets and odd extents: no multiple of a mask word, rows that are no whole lines
BOXES = {"plane": ((1, 0, 1), (29, 1, 5)), "square": ((3, 0, 5), (57, 1, 51)), "volume": ((1, 1, 1), (7, 3, 5)), "real": ((5, 0, 3), (27, 1, 3))}


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
    expected, voxels, non_finite, bound = ensemble_ref.gram(list(frames), box)
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
    assert (over <= bound).all(), f"worst error {over.max():.3e} = {worst:.3f} of its bound"
    return G, bound


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
    expected, bound = ensemble_ref.mix(list(frames), W)
    finite = np.isfinite(expected.real) & np.isfinite(expected.imag) if not real else np.isfinite(expected)
    if real:
        over = np.abs(out.astype(np.float64) - expected)
    else:
        over = np.maximum(np.abs(out.real.astype(np.float64) - expected.real), np.abs(out.imag.astype(np.float64) - expected.imag))
    ratio = np.where(finite, over / np.maximum(bound, 1e-300), 0.0)
    print(f"  {what}: K {K} -> M {M} {'real' if real else 'complex'}: worst error {np.where(finite, over, 0).max():.3e} = {ratio.max():.3f} of its bound, "
          f"{int((~finite).sum())} non-finite, {ms * 1e3:.1f} us")
    assert out.shape == (M,) + frames.shape[1:] and out.dtype == frames.dtype and ms > 0
    assert (over[finite] <= bound[finite]).all(), f"worst error {ratio.max():.3f} of its bound"
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


def check_mix_field(which, frames, ids, W, lattice, tag=0, what=""):
    """mix the len(frames) newest frames under the field W (Nz, Ny, Nx, M, K) on `lattice` (nodes, first, step) and check the outputs
    against the float64 reference within its bound, and their ids; returns (outputs, first id)"""
    M = W.shape[3]
    first, ms = bf.mix_field_last_frames(len(frames), W, lattice["first"], lattice["step"], tag=tag)
    out = bf.get_last_frames(block(which).bp, M).copy()
    expected, bound = block_filter_ref.mix_field(list(frames), W, lattice["first"], lattice["step"])
    over = np.abs(out.astype(np.float64) - expected) if not np.iscomplexobj(frames) else \
        np.maximum(np.abs(out.real - expected.real), np.abs(out.imag - expected.imag))
    print(f"  {what}: K {len(frames)} -> M {M}, nodes {lattice['nodes']}: worst error {float((over / np.maximum(bound, 1e-300)).max()):.3f} of its bound, {ms * 1e3:.1f} us")
    assert out.shape == (M,) + frames.shape[1:] and out.dtype == frames.dtype and ms > 0
    assert (over <= bound).all()
    assert first == ids[-1] + 1 and int(newest_info(bf.library()).frame_id) == first + M - 1
    assert np.array_equal(bf.copy_frame(ids[0]).view(np.uint32), frames[0].view(np.uint32))       # a source is still served by its id
    return out, first


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


def parts(a):
    """the floats of an array of frames as (real parts, imaginary parts or None)"""
    return (a.real, a.imag) if np.iscomplexobj(a) else (a, None)


def share_of_bound(got, expected, bound, finite):
    """the worst |got - expected| / bound over the finite voxels of every lag, real and imaginary parts (lag 0's imaginary part, exact
    by definition, is left out): (worst share, every float within its bound)"""
    worst, inside = 0.0, True
    for lag in range(len(got)):
        for which, (g, x) in enumerate(zip(parts(got[lag]), parts(expected[lag]))):
            if g is None or (which == 1 and lag == 0):
                continue
            f = finite[lag]
            over = np.abs(g[f].astype(np.float64) - x[f])
            if over.size:
                worst = max(worst, float((over / np.maximum(bound[lag][f], 1e-300)).max()))
                inside = inside and bool((over <= bound[lag][f]).all())
    return worst, inside


def burst_info_unchanged(after, before):
    """the newest burst's info behind the outputs: what the library keeps -- the route, the ids, the stage kinds -- equal byte for byte.
    The stage times are not kept: every call asks the runtime again for the time between the same two events, and the runtime converts
    device ticks to nanoseconds with a calibration it renews as it runs, so two answers may differ by nanoseconds; they are asked to
    within a microsecond."""
    times = P.HipBurstInfo.stage_ms.offset
    a, b = bytes(after), bytes(before)
    moved = max(abs(x - y) for x, y in zip(list(after.stage_ms) + [after.burst_ms], list(before.stage_ms) + [before.burst_ms]))
    print(f"  burst info behind the outputs: stage times moved by {moved * 1e6:.1f} ns at the most")
    assert a[:times] == b[:times] and len(a) == len(b) == P.HipBurstInfo.burst_ms.offset + 4
    assert moved <= 1e-3, f"stage times moved by {moved:.3e} ms (bar 1e-3)"


def finite_of(a):
    return np.isfinite(a.real) & np.isfinite(a.imag) if np.iscomplexobj(a) else np.isfinite(a)


def check_autocorr(which, frames, ids, W, lags, tag=0, what="", factor=1.0, expected=None):
    """autocorrelate the len(frames) newest frames under W (None: the identity form) and check the outputs and their records; returns
    (outputs, first id).  expected: (values, bound) other than the reference's on `frames`; factor: the multiple of the bound asked."""
    acq = block(which)
    K = len(frames)
    real = not np.iscomplexobj(frames)
    source_block = int(bf.frame_info(ids[-1]).parameter_block)
    first, ms = bf.autocorrelate_last_frames(K, W, lags, tag=tag)
    out = bf.get_last_frames(acq.bp, lags).copy()
    values, bound = expected if expected is not None else autocorr_ref.autocorrelate(list(frames), W, lags)
    finite = finite_of(values)
    worst, inside = share_of_bound(out, values, factor * bound, finite)
    rows = K if W is None else W.shape[0]
    print(f"  {what}: K {K}, rows {rows}{' (identity)' if W is None else ''}, lags {lags}, {'real' if real else 'complex'} {frames.shape[1:]}: "
          f"worst error {worst:.4f} of its bound, {int((~finite).sum())} non-finite, {ms * 1e3:.1f} us")
    assert out.shape == (lags,) + frames.shape[1:] and out.dtype == frames.dtype and ms > 0
    assert inside, f"worst error {worst:.4f} of its bound"
    # a voxel that is not finite in some source is not finite in every output, lag 0's imaginary part included
    assert np.array_equal(finite_of(out), finite)
    if not real:
        assert np.array_equal(np.isfinite(out[0].imag), finite[0])
        assert not out[0].imag.view(np.uint32)[finite[0]].any()                      # exactly +0: no bit set
    assert (out[0].real[finite[0]] >= 0).all()
    # the records: consecutive ids behind the sources, the grid, the kind, the tag, the newest source's block
    assert first == ids[-1] + 1 and int(newest_info(bf.library()).frame_id) == first + lags - 1
    scores, _ = bf.score_last_frames(lags)
    pz, py, px = frames.shape[1:]
    for j in range(lags):
        info = bf.frame_info(first + j)
        assert (int(info.frame_id), tuple(info.points), int(info.parameter_block)) == (first + j, (px, py, pz), source_block)
        assert int(info.data_kind) == int(D.Float32 if real else D.Float32Complex)
        assert (int(scores[j].frame_id), int(scores[j].image_plane_tag), int(scores[j].parameter_block)) == (first + j, tag, source_block)
    # their rows of the timing table: no stages, no DAS voxels
    t = P.HipFrameTimings()
    assert bf.library().beamformer_hip_get_last_frame_timings(C.byref(t)) and t.stage_count == 0 and t.das_voxels == 0
    # a source frame is still served by its id
    assert np.array_equal(bf.copy_frame(ids[0]).view(np.uint32), frames[0].view(np.uint32))
    return out, first


# (K, rows, lags): one row; a ragged tile of three; a tile boundary at row 16 with all three carried rows in use; one full tile; two
# full tiles and one row; more than 64 frames and a ragged fifth tile
AUTOCORR_CASES = [(1, 1, 1), (3, 3, 3), (5, 17, 4), (17, 16, 4), (17, 33, 2), (65, 65, 4)]


def singles(K, boxes):
    return [bf.gram_last_frames(K, region_of(box))[:2] for box in boxes]


def same_as_singles(got, infos, want, what):
    for n, (G, info) in enumerate(want):
        assert got[n].tobytes() == G.tobytes(), f"{what}: the matrix of box {n}"
        assert bytes(infos[n]) == bytes(info), f"{what}: the info of box {n}"


def finer(points, factor=4):
    """the grid `factor` times finer an axis over the same box: voxel i lands on map voxel factor * i"""
    return tuple(factor * (n - 1) + 1 if n > 1 else 1 for n in points)


def map_view(points, lo, hi):
    """the map's grid as a view; an axis without extent (a plane's y) gets one: the map's transform has to be regular"""
    return bf.view(points, lo, tuple(h if h != l else l + 1e-3 for l, h in zip(lo, hi)))


def placement_onto(grid, transform, points):
    return bf.map_placement(list(transform), points, list(grid.das_voxel_transform), list(grid.output_points))


def points_of(frame):
    return frame.shape[::-1]


def run_localise(grid, frames, thresholds, placements, use_offsets=True, box=None, reset=True):
    """reset the map (unless told not to), deposit the len(frames) newest frames, download: (counts, rows, info)"""
    if reset:
        bf.localisation_map_reset(grid.output_points)
    rows, ms = bf.accumulate_peaks_last_frames(len(frames), thresholds, placements, use_offsets, region_of(box))
    assert ms > 0
    counts, info = bf.localisation_map_copy(grid.output_points)
    assert tuple(info.points) == tuple(grid.output_points)
    return counts, rows, info


def check_rows(rows, expected, frames, thresholds, box=None):
    """the rows against the reference's numbers and against find_peaks' rows of the same call"""
    found, _, _ = bf.find_peaks_last_frames(len(frames), thresholds, 16, region_of(box))
    each = [thresholds] * len(frames) if np.ndim(thresholds) == 0 else list(thresholds)
    for k, (row, want, peaks) in enumerate(zip(rows, expected, found)):
        print(f"  frame {int(row.frame_id)} {tuple(row.points)}: found {int(row.found)}, above {int(row.above_threshold)}, "
              f"deposited {int(row.deposited)}, outside {int(row.outside)}")
        assert (int(row.found), int(row.above_threshold)) == (int(peaks.found), int(peaks.above_threshold)) == (want["found"], want["above_threshold"])
        assert (int(row.deposited), int(row.outside)) == (want["deposited"], want["outside"]) and row.deposited + row.outside == row.found
        assert (row.frame_id, row.parameter_block, row.data_kind, row.image_plane_tag) == (peaks.frame_id, peaks.parameter_block, peaks.data_kind, peaks.image_plane_tag)
        assert tuple(row.points) == tuple(peaks.points) == points_of(frames[k]) and tuple(row.reserved) == (0, 0)
        assert tuple(row.region_first) == tuple(peaks.region_first) and tuple(row.region_count) == tuple(peaks.region_count)
        assert row.threshold == np.float32(each[k])


def same_localise(counts, expected):
    assert counts.dtype == expected.dtype == np.uint32 and counts.shape == expected.shape
    assert counts.tobytes() == expected.tobytes(), f"{int((counts != expected).sum())} bins differ"


def binned_records(points, frames_count, thresholds, placements, use_offsets=True, box=None):
    """the reference map of the records find_peaks returns for the newest frames, at the cap of 65536"""
    rows, peaks, _ = bf.find_peaks_last_frames(frames_count, thresholds, P.HIP_MAX_PEAKS_PER_FRAME, region_of(box))
    records = np.frombuffer(bytes(peaks), np.dtype(P.HipFramePeak))
    counts = np.zeros((points[2], points[1], points[0]), np.uint32)
    A = np.asarray(placements, np.float64).reshape(-1, 3, 4)
    numbers = []
    for k, row in enumerate(rows):
        assert row.stored == row.found
        mine = records[int(row.first):int(row.first) + int(row.stored)]
        deposited, outside = localisation_ref.deposit_records(counts, mine["index"], mine["offset"], A[0 if len(A) == 1 else k], use_offsets)
        numbers.append({"found": int(row.found), "above_threshold": int(row.above_threshold), "deposited": deposited, "outside": outside})
    return counts, numbers


FRACTIONS = [0.5, 1.0, 0.05, 0.999, 0.0, 0.5]       # unsorted, with a repeat


def bits(value):
    return int(np.asarray(value, np.float32).view(np.uint32))


def ranked(frames, fractions, box=None, histograms=True):
    """one call over the len(frames) newest frames, every field against the reference applied to the downloaded frames: the
    reference's results, frame by frame"""
    rows, records, tables, ms = bf.quantiles_last_frames(len(frames), fractions, region_of(box), histograms=histograms)
    fractions = [float(f) for f in np.atleast_1d(fractions)]
    K = len(fractions)
    volume = sum(int(np.prod(box[1] if box else f.shape)) * f.itemsize for f in frames)
    print(f"  quantiles of {len(frames)} frames, {K} fractions, box {box}: {volume} bytes of boxes, device {ms:.4f} ms")
    assert ms > 0 and len(records) == len(frames) * K and (tables is not None) == histograms
    expected = []
    for n, frame in enumerate(frames):
        want = frame_quantiles_ref.quantiles(frame, fractions, *(box if box else (None, None)))
        row, real = rows[n], not np.iscomplexobj(frame)
        info = bf.frame_info(int(row.frame_id))
        assert tuple(row.points) == tuple(info.points) == want["points"] and row.data_kind == info.data_kind
        assert row.data_kind == int(P.DataKind.Float32 if real else P.DataKind.Float32Complex)
        assert row.parameter_block == info.parameter_block
        assert tuple(row.region_first) == want["region_first"] and tuple(row.region_count) == want["region_count"]
        assert (int(row.first), int(row.stored), int(row.reserved)) == (n * K, K, 0)
        assert (int(row.voxels), int(row.non_finite)) == (want["voxels"], want["non_finite"]), (n, int(row.voxels), int(row.non_finite))
        assert row.voxels + row.non_finite == int(np.prod(want["region_count"]))
        for k, q in enumerate(want["rows"]):
            got = records[n * K + k]
            print(f"    frame {int(row.frame_id)} f {q['fraction']!r}: rank {int(got.rank)} value {float(got.value)!r} below {int(got.below)} "
                  f"equal {int(got.equal)} threshold {float(got.threshold)!r}  (reference rank {q['rank']} value {float(q['value'])!r})")
            assert got.fraction == q["fraction"] and got.reserved == 0
            assert (int(got.rank), int(got.below), int(got.equal)) == (q["rank"], q["below"], q["equal"]), (n, k)
            assert bits(got.value) == q["value_bits"], (n, k)
            assert bits(got.magnitude) == bits(q["magnitude"]) and bits(got.threshold) == bits(q["threshold"]), (n, k)
            assert got.below <= got.rank < got.below + got.equal or want["voxels"] == 0
        if histograms:
            assert tables.shape == (len(frames), P.HIP_QUANTILE_BINS) and tables[n].tobytes() == want["histogram"].tobytes(), n
            assert int(tables[n].sum(dtype=np.uint64)) == int(row.voxels) and not tables[n, 2040:].any()
        expected.append(want)
    return expected


ENTRY = np.dtype(P.HipShiftCorrelation)
DOUBLES = ("re", "im", "energy_reference", "energy_frame")


def regions_of(boxes):
    return None if boxes is None else [bf.frame_region(*b) for b in boxes]


SEEN = []           # the worst share of its bar of every call checked in this run, for the figure the commit message quotes


def worst_of(table, expected, bars):
    """the largest error of the four doubles as a fraction of its bar (0 where the bar and the error are both 0, inf where the bar alone is)"""
    worst = 0.0
    for name, bar in zip(DOUBLES, (0, 0, 1, 2)):
        over = np.abs(table[name] - expected[name])
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(over > 0, over / bars[..., bar], 0.0)
        worst = max(worst, float(ratio.max()))
    return worst


def check_correlate(frames, ids, reference, window, boxes=None, what=""):
    """one call against the reference applied to the downloaded frames; returns (table, expected, bars)"""
    K = len(frames)
    real = not np.iscomplexobj(frames)
    pz, py, px = frames[0].shape
    table, info, ms = bf.correlate_last_frames(K, reference, window, regions_of(boxes))
    expected, bars = motion_ref.correlate(list(frames), reference, window, boxes)
    R, T = (1 if boxes is None else len(boxes)), int(np.prod([2 * s + 1 for s in window]))
    assert table.shape == expected.shape == (R, K, 2 * window[2] + 1, 2 * window[1] + 1, 2 * window[0] + 1) and table.dtype == ENTRY
    same_terms = np.array_equal(table["terms"], expected["terms"])
    finite = all(np.isfinite(table[name]).all() for name in DOUBLES)
    worst = worst_of(table, expected, bars) if same_terms and finite else float("nan")
    SEEN.append(worst)
    print(f"  {what}: K {K} ref {reference} {(px, py, pz)} {'real' if real else 'complex'} window {window} boxes {boxes}: terms "
          f"{int(table['terms'].sum())} ({int(expected['terms'].sum())}), worst error {worst:.3f} of its bar (the largest of this run so far "
          f"{max(SEEN):.3f}), {ms * 1e3:.1f} us")
    assert same_terms and finite and ms > 0
    assert worst <= 1.0, f"worst error {worst:.3f} of its bar"
    # info, field by field
    assert (int(info.count), int(info.reference), int(info.data_kind), int(info.region_count)) == (K, reference, int(D.Float32 if real else D.Float32Complex), R)
    assert tuple(info.points) == (px, py, pz) and tuple(info.max_shift) == tuple(window) and int(info.shifts) == T
    assert (int(info.first_frame_id), int(info.reference_frame_id), int(info.reserved)) == (ids[0], ids[reference], 0)
    # an entry without terms is 40 zero bytes; real frames have no imaginary part
    empty = table["terms"] == 0
    assert not table[empty].tobytes().strip(b"\0")
    if real:
        assert not table["im"].any()
    return table, expected, bars


SPATIAL_ZERO, NORMALISED = int(P.HipSpatialMode.Zero), int(P.HipSpatialMode.Normalised)
ROWS = (273, 3, 5)
COLUMN = (1, 5, 9)                 # one x point: the y axis is the contiguous one, and spatial_row_kernel runs it


@functools.lru_cache(maxsize=None)
def spatial_block_of(which):
    if which not in ("rows", "column"):
        return block(which)
    return cfg.rca("spatial_" + which, 16, 2, 256, ROWS if which == "rows" else COLUMN, vc.LO3, vc.HI3, seed=7500, interp=P.InterpolationMode.Linear, demodulate=False,
                   data_kind=D.Float32Complex, angles=np.array([-6.0, 6.0]), kind=P.AcquisitionKind.RCA_TPW)


def finite_parts(a):
    return (np.isfinite(a.real), np.isfinite(a.imag)) if np.iscomplexobj(a) else (np.isfinite(a),)


def check_convolve(which, frames, ids, taps, mode=SPATIAL_ZERO, tag=0, what=""):
    """filter the len(frames) newest frames and check the outputs and their records; returns (outputs, first id)"""
    acq = spatial_block_of(which)
    K = len(frames)
    real = not np.iscomplexobj(frames)
    source_block = int(bf.frame_info(ids[-1]).parameter_block)
    first, ms = bf.convolve_last_frames(K, taps, mode, tag=tag)
    out = bf.get_last_frames(acq.bp, K).copy()
    assert out.shape == frames.shape and out.dtype == frames.dtype and ms > 0
    worst, inside, masks, holes = 0.0, True, True, 0
    for n in range(K):
        values, bound = spatial_ref.convolve(frames[n], taps, mode)
        w, i = spatial_ref.share_of_bound(out[n], values, bound)
        worst, inside = max(worst, w), inside and i
        # finite exactly where the reference is: Zero mode, where no voxel under the taps is not finite; Normalised, where D > 0
        masks = masks and all(np.array_equal(g, x) for g, x in zip(finite_parts(out[n]), finite_parts(values)))
        holes += int((~finite_parts(values)[0]).sum())
    counts = [0 if h is None else len(h) for h in taps]
    print(f"  {what}: K {K}, taps {counts}, mode {mode}, {'real' if real else 'complex'} {frames.shape[1:]}: worst error {worst:.4f} of its bound, "
          f"{holes} real parts not finite, {ms * 1e3:.1f} us")
    assert inside and masks, f"worst error {worst:.4f} of its bound, masks equal: {masks}"
    # the records: consecutive ids behind the sources, the grid, the kind, the tag, the newest source's block
    assert first == ids[-1] + 1 and int(newest_info(bf.library()).frame_id) == first + K - 1
    scores, _ = bf.score_last_frames(K)
    pz, py, px = frames.shape[1:]
    for j in range(K):
        info = bf.frame_info(first + j)
        assert (int(info.frame_id), tuple(info.points), int(info.parameter_block)) == (first + j, (px, py, pz), source_block)
        assert int(info.data_kind) == int(D.Float32 if real else D.Float32Complex)
        assert (int(scores[j].frame_id), int(scores[j].image_plane_tag), int(scores[j].parameter_block)) == (first + j, tag, source_block)
    # their rows of the timing table: no stages, no DAS voxels
    t = P.HipFrameTimings()
    assert bf.library().beamformer_hip_get_last_frame_timings(C.byref(t)) and t.stage_count == 0 and t.das_voxels == 0
    # a source frame is still served by its id
    assert np.array_equal(bf.copy_frame(ids[0]).view(np.uint32), frames[0].view(np.uint32))
    return out, first


LINEAR, CUBIC = int(P.HipWarpInterpolation.Linear), int(P.HipWarpInterpolation.Cubic)
WARP_ZERO, CLAMP = int(P.HipWarpEdge.Zero), int(P.HipWarpEdge.Clamp)
DEEP, WIDE = (37, 19, 11), (96, 1, 96)
OWN = {"deep": (DEEP, vc.LO3, vc.HI3), "wide": (WIDE, vc.LO, vc.HI)}


@functools.lru_cache(maxsize=None)
def warp_block_of(which):
    if which not in OWN:
        return block(which)
    points, lo, hi = OWN[which]
    return cfg.rca("warp_" + which, 16, 2, 256, points, lo, hi, seed=7500, interp=P.InterpolationMode.Linear, demodulate=False,
                   data_kind=D.Float32Complex, angles=np.array([-6.0, 6.0]), kind=P.AcquisitionKind.RCA_TPW)


def warp_call(K, case, rotations=None, interpolation=LINEAR, edge=WARP_ZERO, tag=0):
    return bf.warp_last_frames(K, case["field"], case["nodes"], case["node_first"], case["node_step"], rotations, interpolation, edge, tag=tag)


def warp_reference(frames, case, rotations, interpolation, edge):
    return [warp_ref.warp(frames[n], case["field"][n], case["nodes"], case["node_first"], case["node_step"],
                     None if rotations is None else rotations[n], interpolation, edge) for n in range(len(frames))]


def check_warp(which, frames, ids, case, rotations=None, interpolation=LINEAR, edge=WARP_ZERO, tag=0, what="", same_masks=False):
    """warp the len(frames) newest frames and check the outputs and their records; returns (outputs, first id, worst share, compared share)"""
    acq = warp_block_of(which)
    K = len(frames)
    real = not np.iscomplexobj(frames)
    source_block = int(bf.frame_info(ids[-1]).parameter_block)
    first, ms = warp_call(K, case, rotations, interpolation, edge, tag)
    out = bf.get_last_frames(acq.bp, K).copy()
    assert out.shape == frames.shape and out.dtype == frames.dtype and ms > 0
    worst, inside, compared, total = 0.0, True, 0, 0
    for n, (values, bound) in enumerate(warp_reference(frames, case, rotations, interpolation, edge)):
        w, i = warp_ref.share_of_bound(out[n], values, bound)
        worst, inside = max(worst, w), inside and i
        for got, x in zip(*[(a.real, a.imag) if np.iscomplexobj(values) else (a,) for a in (out[n], values)]):
            compared, total = compared + int(np.isfinite(x).sum()), total + x.size
            if same_masks:                # the positions are float32 numbers: the device's support is the reference's, voxel for voxel
                assert np.array_equal(np.isfinite(got), np.isfinite(x))
    share = compared / total
    print(f"  {what}: K {K}, nodes {case['nodes']}, interpolation {interpolation}, edge {edge}, {'real' if real else 'complex'} {frames.shape[1:]}: "
          f"worst error {worst:.4f} of its bound, {share:.4f} of the floats compared, {ms * 1e3:.1f} us")
    assert inside, f"worst error {worst:.4f} of its bound"
    # the records: consecutive ids behind the sources, the grid, the kind, the tag, the newest source's block
    assert first == ids[-1] + 1 and int(newest_info(bf.library()).frame_id) == first + K - 1
    scores, _ = bf.score_last_frames(K)
    pz, py, px = frames.shape[1:]
    for j in range(K):
        info = bf.frame_info(first + j)
        assert (int(info.frame_id), tuple(info.points), int(info.parameter_block)) == (first + j, (px, py, pz), source_block)
        assert int(info.data_kind) == int(D.Float32 if real else D.Float32Complex)
        assert (int(scores[j].frame_id), int(scores[j].image_plane_tag), int(scores[j].parameter_block)) == (first + j, tag, source_block)
    t = P.HipFrameTimings()
    assert bf.library().beamformer_hip_get_last_frame_timings(C.byref(t)) and t.stage_count == 0 and t.das_voxels == 0
    assert np.array_equal(bf.copy_frame(ids[0]).view(np.uint32), frames[0].view(np.uint32))       # a source is still served by its id
    return out, first, worst, share


def pair(count, thresholds, placements, reach, cap=CAP, use_offsets=True, deposit=False, box=None):
    rows, pairs, ms = bf.pair_peaks_last_frames(count, thresholds, placements, reach, cap, use_offsets, deposit, region_of(box))
    assert ms > 0
    return rows, np.frombuffer(bytes(pairs), tracks_ref.PAIR)


def expected_pair_rows(numbers, count, thresholds, cap, box=None):
    """the rows the call owes: the reference's numbers, and find_peaks' ids and counts of the same frames"""
    found, _, _ = bf.find_peaks_last_frames(count, thresholds, cap, region_of(box))
    levels = tracks_ref.each(np.asarray(thresholds, np.float32), count)
    rows = (P.HipPeakPairs * len(numbers))()
    for n, (row, want) in enumerate(zip(rows, numbers)):
        for k in range(2):
            peaks = found[n + k]
            row.frame_id[k], row.threshold[k], row.peaks[k], row.found[k] = peaks.frame_id, float(levels[n + k]), peaks.stored, peaks.found
            assert int(peaks.stored) == want["peaks"][k] and ("found" not in want or int(peaks.found) == want["found"][k])
            row.unplaced[k], row.unpaired[k] = want["unplaced"][k], want["unpaired"][k]
        row.first, row.pairs, row.deposited, row.outside = want["first"], want["pairs"], want["deposited"], want["outside"]
    return rows


def same_pairs_call(rows, got, want, numbers, count, thresholds, cap=CAP, box=None):
    """the packed records and the rows, byte for byte"""
    print("  " + ", ".join(f"pair {n}: {w['peaks']} peaks, {w['pairs']} pairs, unpaired {w['unpaired']}, unplaced {w['unplaced']}, "
                           f"deposited {w['deposited']}, outside {w['outside']}" for n, w in enumerate(numbers)))
    assert got.tobytes() == want.tobytes(), f"{len(got)} records against {len(want)}"
    assert bytes(rows) == bytes(expected_pair_rows(numbers, count, thresholds, cap, box))
    for row in rows:
        assert row.deposited + row.outside in (0, row.pairs) and row.peaks[0] - row.unplaced[0] - row.pairs == row.unpaired[0]


def same_map(points, counts, sums):
    got_counts, got_sums, info = bf.track_map_copy(points)
    assert tuple(info.points) == tuple(points) and got_counts.dtype == np.uint32 and got_sums.dtype == np.int64
    assert got_counts.tobytes() == counts.tobytes(), f"{int((got_counts != counts).sum())} counts differ"
    assert got_sums.tobytes() == sums.tobytes(), f"{int((got_sums != sums).sum())} sums differ"
    return info


def peak_lists(count, thresholds, cap=CAP, box=None):
    """the find_peaks records of the `count` newest frames: [(index, offset)] for the reference (complex frames)"""
    rows, peaks, _ = bf.find_peaks_last_frames(count, thresholds, cap, region_of(box))
    records = np.frombuffer(bytes(peaks), np.dtype(P.HipFramePeak))
    return [(records[int(r.first):int(r.first) + int(r.stored)]["index"], records[int(r.first):int(r.first) + int(r.stored)]["offset"]) for r in rows]


def planted_push(values):
    """one planted frame by a single push: (the downloaded frame, its id) -- and it IS what was planted"""
    acq = planted.block(values)
    frame = bf.beamform(acq.bp, acq.rf, acq.filters).copy()
    assert planted.same(frame, planted.expected(values)), "the DAS kernel changed a planted value"
    return frame, int(newest_info(bf.library()).frame_id)


def planted_burst(stack):
    """K planted frames by one burst push (one: a single push): (frames (K, Z, Y, X), ids); frame k is planted array k"""
    if len(stack) == 1:
        frame, frame_id = planted_push(stack[0])
        return frame[None], [frame_id]
    blocks = [planted.block(values) for values in stack]
    frames = bf.beamform_burst(blocks[0].bp, np.stack([acq.rf for acq in blocks]), blocks[0].filters).copy()
    for k, values in enumerate(stack):
        assert planted.same(frames[k], planted.expected(values)), f"frame {k} of the burst is not planted array {k}"
    newest = int(newest_info(bf.library()).frame_id)
    return frames, list(range(newest - len(stack) + 1, newest + 1))


def track(count, thresholds, placements, reach, min_length, cap=CAP, use_offsets=True, deposit=0, box=None):
    rows, tracks, points, ms = bf.track_peaks_last_frames(count, thresholds, placements, reach, cap, min_length, use_offsets, deposit, region_of(box))
    assert ms > 0
    return rows, np.frombuffer(bytes(tracks), track_chains_ref.TRACK), np.frombuffer(bytes(points), track_chains_ref.POINT)


def expected_track_rows(numbers, count, thresholds, cap, box=None):
    """the rows the call owes: the reference's numbers, and find_peaks' ids and counts of the same frames"""
    found, _, _ = bf.find_peaks_last_frames(count, thresholds, cap, region_of(box))
    levels = tracks_ref.each(np.asarray(thresholds, np.float32), count)
    rows = (P.HipTrackedFrame * count)()
    for row, want, peaks, level in zip(rows, numbers, found, levels):
        row.frame_id, row.threshold, row.peaks, row.found, row.unplaced = peaks.frame_id, float(level), peaks.stored, peaks.found, want["unplaced"]
        assert int(peaks.stored) == want["peaks"] and ("found" not in want or int(peaks.found) == want["found"])
        for name in track_chains_ref.COUNTERS:
            setattr(row, name, want[name])
    return rows


def same_tracks_call(got, want, count, thresholds, cap=CAP, box=None):
    """the tracks, the points and the rows, byte for byte"""
    rows, tracks, points = got
    print(f"  {len(want['tracks'])} of {len(want['lengths'])} tracks kept, {len(want['points'])} points; lengths {sorted(want['lengths'])[-12:]}")
    assert tracks.tobytes() == want["tracks"].tobytes(), f"{len(tracks)} tracks against {len(want['tracks'])}"
    assert points.tobytes() == want["points"].tobytes(), f"{len(points)} points against {len(want['points'])}"
    assert bytes(rows) == bytes(expected_track_rows(want["rows"], count, thresholds, cap, box))


def fresh_maps(field):
    """both maps of the device reset to `field`, and the reference's: (density, counts, sums)"""
    bf.localisation_map_reset(field)
    bf.track_map_reset(field)
    return (np.zeros(field[::-1], np.uint32),) + tracks_ref.empty_map(field)


def same_maps(field, density, counts, sums):
    got, info = bf.localisation_map_copy(field)
    assert got.tobytes() == density.tobytes(), f"{int((got != density).sum())} bins of the localisation map differ"
    return info, same_map(field, counts, sums)


POINTS, LINKS = P.HIP_TRACK_DEPOSIT_POINTS, P.HIP_TRACK_DEPOSIT_LINKS


def draw(count, thresholds, placements, reach, min_length, smooth, cap=CAP, use_offsets=True, deposit=0, box=None):
    rows, ms = bf.draw_tracks_last_frames(count, thresholds, placements, reach, cap, min_length, smooth, use_offsets, deposit, region_of(box))
    assert ms > 0
    return rows


def expected_drawn_rows(numbers, count, thresholds, cap, box=None):
    """the rows the call owes: the reference's numbers, and find_peaks' ids and counts of the same frames"""
    found, _, _ = bf.find_peaks_last_frames(count, thresholds, cap, region_of(box))
    levels = tracks_ref.each(np.asarray(thresholds, np.float32), count)
    rows = (P.HipDrawnFrame * count)()
    for row, want, peaks, level in zip(rows, numbers, found, levels):
        row.frame_id, row.threshold, row.peaks, row.found, row.unplaced = peaks.frame_id, float(level), peaks.stored, peaks.found, want["unplaced"]
        assert int(peaks.stored) == want["peaks"] and ("found" not in want or int(peaks.found) == want["found"])
        for name in track_draw_ref.COUNTERS:
            setattr(row, name, want[name])
    return rows


def same_rows(rows, want, count, thresholds, cap=CAP, box=None):
    owed = expected_drawn_rows(want["rows"], count, thresholds, cap, box)
    if bytes(rows) != bytes(owed):
        for n, (a, b) in enumerate(zip(rows, owed)):
            print(n, [(name, getattr(a, name), getattr(b, name)) for name, _ in P.HipDrawnFrame._fields_ if getattr(a, name) != getattr(b, name)])
    assert bytes(rows) == bytes(owed)


def fresh_point_and_track_maps(point_field, track_field):
    """both maps of the device reset, and the reference's: (density, counts, sums)"""
    bf.localisation_map_reset(point_field)
    bf.track_map_reset(track_field)
    return (np.zeros(point_field[::-1], np.uint32),) + tracks_ref.empty_map(track_field)


def same_point_and_track_maps(point_field, track_field, density, counts, sums):
    got, info = bf.localisation_map_copy(point_field)
    assert got.tobytes() == density.tobytes(), f"{int((got != density).sum())} bins of the localisation map differ"
    return info, same_map(track_field, counts, sums)


def same_infos(point_info, link_info, calls, rows, deposit):
    """the maps' totals after `calls` equal calls on fresh maps"""
    total = track_draw_ref.totals(rows)
    drawn = total["samples"] - total["repeats"]
    assert (point_info.calls, int(point_info.deposited), int(point_info.outside)) == \
        ((calls, calls * total["points_deposited"], calls * total["points_outside"]) if deposit & POINTS else (0, 0, 0))
    assert (link_info.calls, int(link_info.pairs), int(link_info.deposited), int(link_info.outside)) == \
        ((calls, calls * drawn, calls * total["links_deposited"], calls * total["links_outside"]) if deposit & LINKS else (0, 0, 0, 0))
    assert int(link_info.pairs) == int(link_info.deposited) + int(link_info.outside)
