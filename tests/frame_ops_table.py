"""The frame operations as one table.  csrc/frame_ops.cpp takes every operation's source frames through a few shared functions
(newest_ensemble_frames, frames_once_a_box, queue_frames_of_newest): what holds for one operation of a family holds for all of it, and
tests/test_gpu_frame_ops_contract.py, tests/test_frame_ops_contract_host.py and tests/frame_run_wrap_worker.py ask it of all,
parametrised over OPS.  A FrameOp record says everything those need to treat the operations alike.

OPS holds the two families whose frames are of one grid and one kind: `ensemble`, the three calls that read the newest frames through
newest_ensemble_frames (gram, and through frames_once_a_box gram_boxes and correlate), and `produce`, the five that queue frames made
of them through queue_frames_of_newest.  tests/test_frame_ops_contract_host.py reads from csrc/frame_ops.cpp which declared functions
take these paths and holds OPS to exactly those.  The calls on newest_boxed_frames alone and the two map producers are no part of this
table: their rules differ (mixed grids are served, maps hold state) and their modules hold their own tests.

A plain module: it imports no test module, and nothing while it is imported that needs a device or the oracle."""
import ctypes as C
import dataclasses

import numpy as np

from ogl_beamforming_amd import lib as bf
from ogl_beamforming_amd import params as P
from tests import autocorr_ref
from tests import block_filter_ref
from tests import ensemble_ref
from tests import spatial_ref
from tests import warp_ref
from tests.frame_info import newest_id, newest_info
from tests.ring_frames import (block, check_autocorr, check_convolve, check_correlate, check_gram, check_mix, check_mix_field, check_warp, NORMALISED, rf_frames,
                               same_as_singles, singles, weights)

E = P.LibError
FLOATS = C.POINTER(C.c_float)
U3, F3 = C.c_uint32 * 3, C.c_float * 3
CUBIC, CLAMP = int(P.HipWarpInterpolation.Cubic), int(P.HipWarpEdge.Clamp)


@dataclasses.dataclass(frozen=True)
class Row:
    """one malformed call: what differs from the good arguments of FrameOp.bare (made when asked for: some need arrays), the error
    kind, whether it is decided before a device is needed, and the frames present when a live device is asked: K of the grid `which`"""
    what: str
    change: object
    error: object
    host: bool
    which: str = "plane"
    K: int = 3
    counterpart: object = None     # (frames, ids): the check of the nearest good call, on K fresh frames of the grid


@dataclasses.dataclass(frozen=True)
class Run:
    """one good call through the Python helper: its sources, the frames it queues, the call (timed) -> (first id, device ms), and
    judge(outputs, sources) -> the worst error as a share of the reference's bound, asserted to be inside it"""
    K: int
    outputs: int
    call: object
    judge: object


@dataclasses.dataclass(frozen=True)
class FrameOp:
    name: str                      # the pytest id
    symbol: str                    # the ABI call
    helper: object                 # lib.py's
    family: str                    # ensemble (newest_ensemble_frames) or produce (queue_frames_of_newest): its entry path in frame_ops.cpp
    count_cap: int                 # the largest `count` the ABI takes
    bare: object                   # (count, sized=None, null=False, **change) -> (call(L), untouched()): the bare ABI call with good
    #                                arguments for `sized or count` frames, its outputs prefilled with sentinels (null: no outputs)
    good_call: object              # (which, frames, ids, what): the operation's check_* of tests/ring_frames.py on the newest frames
    malformed: tuple               # the operation's own Rows
    plain: object = None           # readers: K -> what the helper returns for good arguments
    run: object = None             # produce: (K, rng) -> Run: a small good call whose outputs the reference judges
    ring_runs: object = None       # produce: (rng, W) -> (Run of 2 outputs, [change of bare(32)], Run on 14 sources): tests/frame_run_wrap_worker.py
    takes_region: bool = False
    box_lists: object = None       # takes_region: box -> the `boxes` of bare() that put this one box where the call could overlook it
    forms: object = lambda count: [{}]       # the changes of bare() under which the call takes another way to the shared function


def sentinels(null):
    """the outputs every producer has, prefilled: (first id, device ms) as the ABI takes them, and untouched()"""
    first, ms = C.c_uint32(77), C.c_float(-1.0)
    return (None, None) if null else (C.byref(first), C.byref(ms)), lambda: first.value == 77 and ms.value == -1.0


def pointer(a, dtype):
    """(the array kept alive, its float pointer) -- None stays None"""
    if a is None:
        return None, None
    a = np.ascontiguousarray(a, dtype)
    return a, a.ctypes.data_as(FLOATS)


def refused(L, op, count, kind, **change):
    """the bare call refuses with this error kind, writes nothing and queues nothing: every output keeps its sentinel, the newest id and
    the newest record's bytes stay, and the frame pushed next takes the next id where it would have lain (the ring's next offset is
    unchanged).  The strictest of the copies this replaces; that push leaves one complex plane frame behind.  While the newest push is a
    tombstone (or several devices are in use) there is no newest record to compare: the call is then held to the error kind, the
    sentinels and the id alone, and nothing is pushed."""
    call, untouched = op.bare(count, **change)
    newest = newest_id(L)
    before = bytes(newest_info(L)) if newest is not None and L.beamformer_hip_get_device_count() == 1 else None
    assert not call(L)
    assert bf.last_error()[0] == kind, (op.name, bf.last_error(), kind, change)
    assert untouched(), (op.name, change)
    assert newest_id(L) == newest
    if before is not None:
        assert bytes(newest_info(L)) == before
        old = newest_info(L)
        acq = block("plane")
        bf.beamform(acq.bp, rf_frames("plane", 1)[0], acq.filters)
        new = newest_info(L)
        assert int(new.frame_id) == int(old.frame_id) + 1
        assert int(new.device_pointer) == int(old.device_pointer) + (int(old.size_bytes) + 63) // 64 * 64


def share(out, expected, bound):
    """the worst |out - expected| / bound, real and imaginary parts, asserted inside the bound"""
    parts = [(out.real, expected.real), (out.imag, expected.imag)] if np.iscomplexobj(expected) else [(out, expected)]
    worst = max(float((np.abs(g.astype(np.float64) - x) / np.maximum(bound, 1e-300)).max()) for g, x in parts)
    assert worst <= 1.0, f"worst error {worst:.4f} of its bound"
    return worst


def framewise(module, out, sources, reference):
    """the worst share of the operations that make one output a source, by the reference module's own share_of_bound:
    reference(frame, n) -> (values, bound)"""
    worst = 0.0
    for n, (got, frame) in enumerate(zip(out, sources)):
        w, inside = module.share_of_bound(got, *reference(frame, n))
        assert inside, w
        worst = max(worst, w)
    return worst


def imaginary_on_real(table):
    """the real table with an imaginary part of 1e-30 in its last float: refused where the frames are real, so not without a device"""
    table = table.astype(np.complex64)
    table.reshape(-1)[-1] += 1e-30j
    return table


# ---- mix ----

def bare_mix(count, sized=None, null=False, weights=None):
    W, w = pointer(np.eye(sized or count, dtype=np.complex64) if weights is None else weights, np.complex64)
    outputs, untouched = sentinels(null)
    return (lambda L: L.beamformer_hip_mix_last_frames(count, w, W.shape[0], 0, *outputs)), untouched


def run_mix(K, W):
    return Run(K, len(W), lambda timed=True: bf.mix_last_frames(K, W, timed=timed),
               lambda out, sources: share(out, *ensemble_ref.mix(list(sources), W)))


MIX = FrameOp(
    name="mix", symbol="beamformer_hip_mix_last_frames", helper=bf.mix_last_frames, family="produce", count_cap=P.HIP_MAX_ENSEMBLE_FRAMES,
    bare=bare_mix,
    good_call=lambda which, frames, ids, what: check_mix(which, frames, ids, weights(2, len(frames), 7700 + len(frames), not np.iscomplexobj(frames)), what=what),
    run=lambda K, rng: run_mix(K, weights(2, K, 7710)),
    # one row of the 32 newest would lie on the oldest of them; 33 rows are a run the ring cannot hold at all
    ring_runs=lambda rng, W: (run_mix(15, W[:2, :15]), [dict(weights=np.ones((1, 32))), dict(weights=np.ones((33, 32)))], run_mix(14, W[:14, :14])),
    malformed=(Row("an imaginary weight on real frames", lambda: dict(weights=imaginary_on_real(weights(3, 5, 7801, real=True))),
                   E.InvalidAccess, host=False, which="real", K=5),),
    )


# ---- mix_field ----

ONE = dict(nodes=(1, 1, 1), first=(9, 9, 9), step=(0, 0, 0))           # the plain mix: first and step are not read
BEYOND = dict(nodes=(3, 1, 2), first=(0, 0, 0), step=(20, 1, 9))       # plane 33 x 1 x 7: x nodes at 0, 20, 40; z nodes at 0, 9
WRAP = dict(nodes=(3, 1, 2), first=(4, 0, 10), step=(25, 1, 40))       # the worker's 64 x 1 x 64


def node_weights(lattice, M, K, seed, real=False):
    nx, ny, nz = lattice["nodes"]
    return np.stack([weights(M, K, seed + n, real) for n in range(nx * ny * nz)]).reshape(nz, ny, nx, M, K)


def bare_mix_field(count, sized=None, null=False, weights=None, lattice=ONE, **lattice_change):
    lattice = dict(lattice, **lattice_change)
    W, w = pointer(np.ones((1, 1, 1, 1, sized or count)) if weights is None else weights, np.complex64)
    outputs, untouched = sentinels(null)
    return (lambda L: L.beamformer_hip_mix_field_last_frames(count, w, U3(*lattice["nodes"]), U3(*lattice["first"]), U3(*lattice["step"]),
                                                             W.shape[3], 0, *outputs)), untouched


def run_mix_field(K, W, lattice):
    return Run(K, W.shape[3], lambda timed=True: bf.mix_field_last_frames(K, W, lattice["first"], lattice["step"], timed=timed),
               lambda out, sources: share(out, *block_filter_ref.mix_field(list(sources), W, lattice["first"], lattice["step"])))


MIX_FIELD = FrameOp(
    name="mix_field", symbol="beamformer_hip_mix_field_last_frames", helper=bf.mix_field_last_frames, family="produce",
    count_cap=P.HIP_MAX_ENSEMBLE_FRAMES, bare=bare_mix_field,
    good_call=lambda which, frames, ids, what: check_mix_field(which, frames, ids, node_weights(BEYOND, 2, len(frames), 8700, not np.iscomplexobj(frames)), BEYOND, what=what),
    run=lambda K, rng: run_mix_field(K, node_weights(WRAP, 2, K, 8710), WRAP),
    ring_runs=lambda rng, W: (run_mix_field(15, node_weights(WRAP, 2, 15, 8720), WRAP),
                              [dict(), dict(weights=node_weights(WRAP, 1, 32, 8730), lattice=WRAP)],
                              run_mix_field(14, node_weights(WRAP, 14, 14, 8740), WRAP)),
    malformed=(
        Row("a step of 0 between nodes", lambda: dict(weights=node_weights(BEYOND, 2, 2, 8600), lattice=BEYOND, step=(0, 1, 9)), E.InvalidAccess, host=True, K=2),
        Row("no node along an axis", lambda: dict(weights=node_weights(BEYOND, 2, 2, 8600), lattice=BEYOND, nodes=(0, 1, 2)), E.BufferOverflow, host=True, K=2),
        Row("a NaN weight", lambda: dict(weights=np.where(np.arange(24).reshape(2, 1, 3, 2, 2) == 6, np.nan, node_weights(BEYOND, 2, 2, 8600)), lattice=BEYOND),
            E.InvalidAccess, host=True, K=2),
        Row("an imaginary weight on real frames, at the last node's last row",
            lambda: dict(weights=imaginary_on_real(node_weights(BEYOND, 2, 3, 8601, real=True)), lattice=BEYOND), E.InvalidAccess, host=False, which="real",
            counterpart=lambda frames, ids: check_mix_field("real", frames, ids, node_weights(BEYOND, 2, 3, 8601, real=True), BEYOND, what="without it"))),
    )


# ---- autocorrelate ----

def bare_autocorrelate(count, sized=None, null=False, weights=None, rows=None, lags=1):
    W, w = pointer(weights, np.complex64)
    outputs, untouched = sentinels(null)
    rows = rows if rows is not None else (sized or count) if W is None else W.shape[0]
    return (lambda L: L.beamformer_hip_autocorrelate_last_frames(count, w, rows, lags, 0, *outputs)), untouched


def run_autocorrelate(K, W, lags):
    def judge(out, sources):
        assert not out[0].imag.any()                                    # lag 0's imaginary part is 0 exactly
        return share(out, *autocorr_ref.autocorrelate(list(sources), W, lags))
    return Run(K, lags, lambda timed=True: bf.autocorrelate_last_frames(K, W, lags, timed=timed), judge)


AUTOCORRELATE = FrameOp(
    name="autocorrelate", symbol="beamformer_hip_autocorrelate_last_frames", helper=bf.autocorrelate_last_frames, family="produce",
    count_cap=P.HIP_MAX_ENSEMBLE_FRAMES, bare=bare_autocorrelate,
    good_call=lambda which, frames, ids, what: check_autocorr(which, frames, ids, None, min(2, len(frames)), what=what),
    run=lambda K, rng: run_autocorrelate(K, weights(4, K, 8710), 2),
    # a run of lags is at most four frames: it meets its own sources only by wrapping
    ring_runs=lambda rng, W: (run_autocorrelate(15, W[:15, :15], 2), [dict(), dict(weights=np.ones((1, 32)))], run_autocorrelate(14, None, 4)),
    malformed=(
        Row("more lags than rows", lambda: dict(weights=weights(2, 3, 8700), lags=3), E.InvalidAccess, host=True),
        Row("more lags than rows, the identity form", lambda: dict(lags=4), E.InvalidAccess, host=True),
        Row("more lags than BEAMFORMER_HIP_MAX_LAGS", lambda: dict(lags=P.HIP_MAX_LAGS + 1), E.InvalidAccess, host=True, K=5),
        Row("no lag", lambda: dict(lags=0), E.InvalidAccess, host=True),
        Row("the identity form with rows != count", lambda: dict(rows=2), E.InvalidAccess, host=True),
        Row("an imaginary weight on real frames", lambda: dict(weights=imaginary_on_real(weights(3, 5, 8501, real=True)), lags=2),
            E.InvalidAccess, host=False, which="real", K=5)),
    forms=lambda count: [{}, dict(weights=np.ones((1, count)))])


# ---- convolve ----

THIRDS = np.full(3, 1 / 3, np.float32)


def bare_convolve(count, sized=None, null=False, taps=(THIRDS, None, THIRDS), mode=0):
    arrays = [pointer(h, np.float32) for h in taps]
    pointers = (FLOATS * 3)(*[p for _, p in arrays])
    counts = U3(*[0 if a is None else len(a) for a, _ in arrays])
    outputs, untouched = sentinels(null)

    def call(L, keep=arrays):            # (the taps live as long as the call does)
        return L.beamformer_hip_convolve_last_frames(count, pointers, counts, mode, 0, *outputs)
    return call, untouched


def run_convolve(K, taps, mode):
    return Run(K, K, lambda timed=True: bf.convolve_last_frames(K, taps, mode, timed=timed),
               lambda out, sources: framewise(spatial_ref, out, sources, lambda frame, n: spatial_ref.convolve(frame, taps, mode)))


def convolve_ring_runs(rng, W):
    """the 14 newest under three passes in Normalised mode, whose scratch (a run and two D fields) is the library's own"""
    taps = [rng.uniform(0.1, 1.0, n).astype(np.float32) for n in (9, 3, 5)]
    return run_convolve(2, [taps[0], None, taps[2]], 0), [dict(taps=taps), dict(taps=taps, mode=NORMALISED)], run_convolve(14, taps, NORMALISED)


CONVOLVE = FrameOp(
    name="convolve", symbol="beamformer_hip_convolve_last_frames", helper=bf.convolve_last_frames, family="produce", count_cap=P.HIP_MAX_ENSEMBLE_FRAMES,
    bare=bare_convolve,
    good_call=lambda which, frames, ids, what: check_convolve(which, frames, ids, [THIRDS, None, THIRDS], NORMALISED, what=what),
    run=lambda K, rng: run_convolve(K, [THIRDS, None, THIRDS], 0),
    ring_runs=convolve_ring_runs,
    malformed=(Row("a negative tap in Normalised mode; Zero mode takes it", lambda: dict(taps=(np.array([0.5, -0.25, 0.5], np.float32), None, None), mode=NORMALISED),
                   E.InvalidAccess, host=True,
                   counterpart=lambda frames, ids: check_convolve("plane", frames, ids, [np.array([0.5, -0.25, 0.5], np.float32), None, None], 0, what="the same taps, zero mode")),),
    forms=lambda count: [{}, dict(mode=NORMALISED)])


# ---- warp ----

def bare_warp(count, sized=None, null=False, field=None, nodes=(1, 1, 1), node_first=(0, 0, 0), node_step=(1, 1, 1), rotations=None, interpolation=0, edge=0):
    d, field_pointer = pointer(np.zeros((sized or count, 1, 1, 1, 3)) if field is None else field, np.float32)
    r, rotation_pointer = pointer(rotations, np.complex64)
    outputs, untouched = sentinels(null)

    def call(L, keep=(d, r)):            # (the field and the rotations live as long as the call does)
        return L.beamformer_hip_warp_last_frames(count, field_pointer, U3(*nodes), F3(*node_first), F3(*node_step), rotation_pointer, interpolation, edge, 0, *outputs)
    return call, untouched


def run_warp(K, field, interpolation=0, edge=0, **lattice):
    return Run(K, K, lambda timed=True: bf.warp_last_frames(K, field, interpolation=interpolation, edge=edge, timed=timed, **lattice),
               lambda out, sources: framewise(warp_ref, out, sources, lambda frame, n: warp_ref.warp(frame, field[n], interpolation=interpolation, edge=edge, **lattice)))


def warp_ring_runs(rng, W):
    shifts = (rng.integers(-20, 21, (32, 3)) / 8.0).astype(np.float32)
    field = rng.uniform(-2.0, 2.0, (14, 2, 1, 3, 3)).astype(np.float32)
    lattice = dict(nodes=(3, 1, 2), node_first=(4.5, 0, 10), node_step=(25.25, 1, 40))
    return (run_warp(2, shifts[:2], interpolation=CUBIC), [dict(field=shifts), dict(field=shifts, interpolation=CUBIC, edge=CLAMP)],
            run_warp(14, field, edge=CLAMP, **lattice))


WARP = FrameOp(
    name="warp", symbol="beamformer_hip_warp_last_frames", helper=bf.warp_last_frames, family="produce", count_cap=P.HIP_MAX_ENSEMBLE_FRAMES,
    bare=bare_warp,
    good_call=lambda which, frames, ids, what: check_warp(which, frames, ids, dict(field=np.zeros((len(frames), 1, 1, 1, 3), np.float32), nodes=(1, 1, 1),
                                                                                   node_first=(0, 0, 0), node_step=(1, 1, 1)), what=what),
    run=lambda K, rng: run_warp(K, np.array([[0.5, 0, -1.25], [-2.125, 0, 0.375], [1, 0, 1]], np.float32)[:K]),
    ring_runs=warp_ring_runs,
    malformed=(Row("an imaginary rotation on real frames; real factors run", lambda: dict(rotations=[1, 1 + 1e-30j, 1]), E.InvalidAccess, host=False, which="real",
                   counterpart=lambda frames, ids: check_warp("real", frames, ids, dict(field=np.zeros((3, 1, 1, 1, 3), np.float32), nodes=(1, 1, 1), node_first=(0, 0, 0),
                                                                                        node_step=(1, 1, 1)), np.array([1, -2, 0.5], np.complex64), what="real factors")),),
    )


# ---- the ensemble readers: gram, gram_boxes, correlate ----

GOOD_BOX = ((1, 0, 1), (5, 1, 3))                  # inside every grid of tests/ring_frames.py GRIDS
WINDOW = (1, 0, 1)


def regions(boxes):
    """(the ctypes array of at least one region, kept alive; how many)"""
    return (P.HipFrameRegion * max(1, len(boxes)))(*[bf.frame_region(*box) for box in boxes]), len(boxes)


def reader_outputs(null, values, info):
    """a reader's outputs prefilled -- the numbers -7, the info's bytes 0x5A, the device time -1 --: (pointers, untouched())"""
    C.memset(C.byref(info), 0x5A, C.sizeof(info))
    ms = C.c_float(-1.0)
    before = values.tobytes()
    untouched = lambda: values.tobytes() == before and bytes(info) == b"\x5A" * C.sizeof(info) and ms.value == -1.0
    return (None, None, None) if null else (values.ctypes.data_as(C.c_void_p), info, C.byref(ms)), untouched


def bare_gram(count, sized=None, null=False, boxes=None):
    K = min(sized or count, 64)
    (gram, info, ms), untouched = reader_outputs(null, np.full((K, K), -7.0 - 7.0j, np.complex128), P.HipEnsembleInfo())
    array = regions(boxes)[0] if boxes else None
    return (lambda L: L.beamformer_hip_gram_last_frames(count, array, C.cast(gram, C.POINTER(C.c_double)), C.byref(info) if info else None, ms)), untouched


def bare_gram_boxes(count, sized=None, null=False, boxes=(GOOD_BOX,)):
    K = min(sized or count, 64)
    array, B = regions(boxes)
    (grams, infos, ms), untouched = reader_outputs(null, np.full((min(max(1, B), 4), K, K), -7.0 - 7.0j, np.complex128), (P.HipEnsembleInfo * max(1, B))())
    return (lambda L: L.beamformer_hip_gram_boxes_last_frames(count, array, B, C.cast(grams, C.POINTER(C.c_double)), infos, ms)), untouched


def bare_correlate(count, sized=None, null=False, boxes=None, reference=0, window=WINDOW):
    array, R = regions(boxes) if boxes else (None, 0)
    room = max(1, R) * (sized or count) * int(np.prod([2 * s + 1 for s in window]))
    (table, info, ms), untouched = reader_outputs(null, np.full(min(room, 1 << 16) * 5, -7.0, np.float64), P.HipCorrelationInfo())
    return (lambda L: L.beamformer_hip_correlate_last_frames(count, reference, array, R, U3(*window), C.cast(table, C.POINTER(P.HipShiftCorrelation)),
                                                             C.byref(info) if info else None, ms)), untouched


def good_gram_boxes(which, frames, ids, what):
    got, infos, _ = bf.gram_boxes_last_frames(len(frames), [bf.frame_region(*GOOD_BOX)])
    same_as_singles(got, infos, singles(len(frames), [GOOD_BOX]), what)
    check_gram(frames, ids, GOOD_BOX, what=what)


def the_entry_cap_is_legal_one_region_below(frames, ids):
    """17 frames x 1089 shifts x 56 regions = 1036728 entries are served, every region's table the single region's"""
    whole = ((0, 0, 0), frames[0].shape[::-1])
    many, info, ms = bf.correlate_last_frames(17, 0, (16, 0, 16), [bf.frame_region(*whole)] * 56)
    single, _, _ = check_correlate(frames, ids, 0, (16, 0, 16), [whole], what="behind the cap")
    print(f"  56 regions x 17 frames x 1089 shifts: {ms * 1e3:.1f} us")
    assert many.shape[0] == 56 and int(info.region_count) == 56 and all(many[r].tobytes() == single[0].tobytes() for r in (0, 1, 55))


PLANE = ((0, 0, 0), (33, 1, 7))
GRAM = FrameOp(
    name="gram", symbol="beamformer_hip_gram_last_frames", helper=bf.gram_last_frames, family="ensemble", count_cap=P.HIP_MAX_ENSEMBLE_FRAMES,
    bare=bare_gram, good_call=lambda which, frames, ids, what: check_gram(frames, ids, what=what), malformed=(),
    plain=lambda K: bf.gram_last_frames(K), takes_region=True, box_lists=lambda box: [[box]])
GRAM_BOXES = FrameOp(
    name="gram_boxes", symbol="beamformer_hip_gram_boxes_last_frames", helper=bf.gram_boxes_last_frames, family="ensemble",
    count_cap=P.HIP_MAX_ENSEMBLE_FRAMES, bare=bare_gram_boxes, good_call=good_gram_boxes,
    malformed=(Row("no box", lambda: dict(boxes=()), E.BufferOverflow, host=True, K=2),
               Row("more boxes than the call takes", lambda: dict(boxes=(GOOD_BOX,) * 1025), E.BufferOverflow, host=True, K=2)),
    plain=lambda K: bf.gram_boxes_last_frames(K, [bf.frame_region(*GOOD_BOX)]), takes_region=True,
    box_lists=lambda box: [[GOOD_BOX, box, GOOD_BOX], [GOOD_BOX, GOOD_BOX, box]])
CORRELATE = FrameOp(
    name="correlate", symbol="beamformer_hip_correlate_last_frames", helper=bf.correlate_last_frames, family="ensemble",
    count_cap=P.HIP_MAX_ENSEMBLE_FRAMES, bare=bare_correlate,
    good_call=lambda which, frames, ids, what: check_correlate(frames, ids, len(frames) - 1, WINDOW, None, what=what),
    malformed=(Row("a reference that is not one of the frames", lambda: dict(reference=2), E.InvalidAccess, host=True, K=2),
               # 17 frames x 1089 shifts x 57 regions = 1055241 > 2^20
               Row("one region over the entry cap", lambda: dict(window=(16, 0, 16), boxes=(PLANE,) * 57), E.BufferOverflow, host=True, K=17),
               Row("256 regions over the entry cap", lambda: dict(window=(16, 0, 16), boxes=(PLANE,) * 256), E.BufferOverflow, host=True, K=17,
                   counterpart=the_entry_cap_is_legal_one_region_below)),
    plain=lambda K: bf.correlate_last_frames(K, 0, WINDOW), takes_region=True, box_lists=lambda box: [[box], [PLANE, box]])


OPS = (GRAM, GRAM_BOXES, CORRELATE, MIX, MIX_FIELD, AUTOCORRELATE, CONVOLVE, WARP)
IDS = [op.name for op in OPS]
PRODUCE = [op for op in OPS if op.family == "produce"]
