"""The comparison every DAS parity test and the fuzz use: a frame of the library against the CPU oracle's frame of the same
input (oracle/), with the tolerances of DESIGN.md 4.  A plain module -- no pytest marker, no device, and the product library is
not loaded by importing it -- so that the CPU tests of the comparison itself (tests/test_compare.py) and the tools can use it.

Linear and cubic interpolation, per voxel:
  flip set F   the valid voxels at which the float oracle is more than 1.5 tol of the frame maximum from its double-precision twin
               (the truth) and which hold a term within float rounding of an end of its RF row (the oracle marks them: its
               ambiguity buffer): there the oracle's own float and double builds took different sides of a step -- sample_rf's
               range test at a row end -- and a whole tap separates them.  On F the frame must meet the FIRST bar against the float
               oracle: the kernels decide row-end terms exactly as the oracle's float build does.
  first bar    |gpu - oracle| <= tol * max|oracle|.
  second bar   only for voxels off F over the first: |gpu - truth| <= oracle_off + tol * max|oracle|, oracle_off the largest
               |oracle - truth| over the valid voxels off F (<= 1.5 tol unless the float oracle's rounding alone, with no row end
               involved, exceeds that somewhere on the frame: at most 2.5 tol in all, or the oracle's own error + tol).
A compared sub-grid (no truth frame of its shape) keeps the first bar only.  Nearest interpolation has a rule of its own (the
oracle's per-voxel ambiguity budget)."""
import atexit
import dataclasses
import json
import os
import sys
import weakref

import numpy as np

from ogl_beamforming_amd import params as P
from tests import cases

FLIP_FACTOR = 1.5           # |oracle_f32 - truth| above FLIP_FACTOR * tol * scale: the voxel is in the flip set F


@dataclasses.dataclass
class Verdict:
    """what compare() found: the largest error against the float oracle (relative to the frame maximum), which bar the frame
    needed ("first": every voxel within tol of the oracle; "second": some voxel off F passed only against the truth), the size
    of the flip set, the voxels that used the second bar and the largest (|gpu - truth| - oracle_off) / scale among them
    (None when none did)"""
    max_rel_err: float
    bar: str
    flip_voxels: int
    second_bar_voxels: int
    worst_excess: float = None
    rule: str = "per-voxel"     # "per-voxel" (linear, cubic), "first-only" (a sub-grid: no truth frame), "nearest"


LOG = []                    # every compare() call: {"test": test id or label, "das_path": DAS path or None, **Verdict}
_TRUTH = {}                 # id(oracle frame) -> (weak reference to it, its double-precision twin, row-end marks): reference() computed them at once


def reference(oracle, acq):
    """(frame, pairs, flags) of the oracle; for nearest interpolation flags carries the per-voxel
    ambiguity budget of taps that sit within 2^-10 of a rounding boundary (oracle/oracle.h).  For linear and cubic interpolation
    the same oracle call computes the frame's double-precision twin and marks the voxels with a term at a row end, which compare()
    then takes (truth_frame, row_end_marks)."""
    nearest = acq.bp.interpolation_mode == int(P.InterpolationMode.Nearest)
    flags = {}
    truth = None if nearest else {}
    ref, pairs = oracle.beamform(acq.bp, acq.rf, acq.filters, flags=flags, truth=truth)
    if truth is not None:
        for key in [k for k, (alive, _, _) in _TRUTH.items() if alive() is None]:
            del _TRUTH[key]
        _TRUTH[id(ref)] = (weakref.ref(ref), truth["frame"], flags["near_half"])
    return ref, pairs, flags if nearest else None


def _twin(acq, shape, ref):
    """(double-precision twin, row-end marks) of the oracle frame `ref`, or (None, None) when the compared frame is a sub-grid"""
    if ref is not None and id(ref) in _TRUTH:
        alive, exact, marks = _TRUTH[id(ref)]
        if alive() is ref:
            return (exact, marks) if exact.shape == tuple(shape) else (None, None)
    from oracle import binding
    truth, flags = {}, {}
    binding.beamform(acq.bp, acq.rf, acq.filters, truth=truth, flags=flags)
    return (truth["frame"], flags["near_half"]) if truth["frame"].shape == tuple(shape) else (None, None)


def truth_frame(acq, shape, ref=None):
    """the oracle's frame with every DAS stage in double precision (oracle.beamform(truth=...)); None when the compared frame is a
    sub-grid of it (those comparisons keep the first bar only).  ref: the oracle frame reference() returned, whose twin it kept."""
    return _twin(acq, shape, ref)[0]


def row_end_marks(acq, shape, ref=None):
    """linear / cubic interpolation: the voxels of the oracle's frame that hold a term within float rounding of an end of its RF row
    (oracle.beamform(flags=...)["near_half"]); None for a sub-grid"""
    return _twin(acq, shape, ref)[1]


def _record(verdict, label, path):
    if label is None:
        label = os.environ.get("PYTEST_CURRENT_TEST", "").rsplit(" (", 1)[0] or None
    LOG.append({"test": label, "das_path": path, **dataclasses.asdict(verdict)})
    return verdict


def compare(gpu, ref, acq, flags=None, *, path=None, label=None):
    """asserts that the library's frame `gpu` is the oracle's `ref` within the rules above; returns the Verdict and appends it to
    LOG with `label` (default: the running test's id) and `path` (the DAS path that computed the frame, when the caller knows it)"""
    assert gpu.shape == ref.shape and gpu.dtype == ref.dtype
    nan_gpu, nan_ref = np.isnan(gpu), np.isnan(ref)
    assert np.array_equal(nan_gpu, nan_ref), "NaN positions (coherency weighting with zero incoherent sum) differ"
    ok = ~nan_ref
    scale = np.max(np.abs(ref[ok])) if ok.any() else 1.0
    assert scale > 0, "oracle image is empty: the case does not exercise the path"
    tol = cases.tolerance(acq)
    if acq.bp.interpolation_mode == int(P.InterpolationMode.Nearest):
        # A sample index within float rounding of k + 1/2 may pick the other tap.  The oracle reports, per
        # voxel, how far such flips can move the coherent sum (flags["budget"], zero where no tap is near a
        # boundary): without coherency weighting EVERY voxel must agree within tolerance + budget; with it
        # (a quotient of two sums the flips both touch) the voxels that hold no such tap must meet SURVEY
        # 8c's bar: fewer than 1e-3 of them off by more than 1e-3.
        assert flags is not None, "nearest interpolation is compared against the oracle's ambiguity budget"
        err = np.abs(gpu - ref)
        if not acq.bp.coherency_weighting:
            slack = tol * scale + 1.01 * flags["budget"]
            assert (err[ok] <= slack[ok]).all(), f"nearest: max excess {np.max(err[ok] - slack[ok]):.3e} over tolerance + tap ambiguity"
        clean = ok & ~flags["near_half"]
        if clean.any():
            bad = float(np.mean(err[clean] > max(tol, 1e-3) * scale))
            assert bad < 1e-3, f"nearest: mismatch fraction {bad:.2e} on the {int(clean.sum())} voxels without boundary taps"
        # no systematic offset hiding under the budget: the median voxel agrees ten times better than the bar -- or, where float rounding
        # of the phase alone is that large (round 4's fuzz draw general/1001: 12 terms at 96 turns, the float oracle itself 1.1e-5 from
        # its double twin at the median voxel), the GPU's median distance to that truth is the oracle's own plus the same allowance
        median_bar = 1e-5 if tol <= 1e-4 else tol
        bar = "first"
        if not np.median(err[ok]) / scale < median_bar:
            exact = truth_frame(acq, ref.shape, ref)
            assert exact is not None, f"nearest: median error {np.median(err[ok]) / scale:.3e} >= {median_bar:.0e}"
            gpu_off, oracle_off = np.median(np.abs(gpu[ok] - exact[ok])) / scale, np.median(np.abs(ref[ok] - exact[ok])) / scale
            assert gpu_off <= oracle_off + median_bar, (f"nearest: median error {np.median(err[ok]) / scale:.3e} >= {median_bar:.0e} and the GPU's median distance to the "
                                                        f"double-precision truth {gpu_off:.3e} exceeds the float oracle's {oracle_off:.3e} by more than that")
            bar = "second"
        return _record(Verdict(float(err[ok].max() / scale), bar, 0, 0, None, "nearest"), label, path)
    err = np.abs(gpu - ref) / scale
    over = ok & (err > tol)
    max_rel = float(err[ok].max()) if ok.any() else 0.0
    exact, marks = _twin(acq, ref.shape, ref)
    if exact is None:
        assert not over.any(), f"max relative error {max_rel:.3e} > {tol:.0e}"
        return _record(Verdict(max_rel, "first", 0, 0, None, "first-only"), label, path)
    # The flip set: voxels at which the float oracle took the other side of a step than its double twin (a tap kept by one and
    # dropped by the other at a row end).  The kernels decide those terms in the float oracle's own arithmetic, so on
    # F the first bar against the float oracle holds -- a kernel that lands on the truth there decided the term differently.  (A voxel
    # with no term at a row end is not in F whatever its error: on 1e-4 frames with coherency weighting the float oracle's rounding
    # alone reaches 1.5 tol at single voxels -- draw_paired 14 -- and a kernel's own rounding there is no flip.)
    oracle_err = np.where(ok, np.abs(ref.astype(exact.dtype) - exact), 0.0)
    flip = ok & marks & (oracle_err > FLIP_FACTOR * tol * scale)
    bad_flip = over & flip
    assert not bad_flip.any(), (f"max relative error {max_rel:.3e} > {tol:.0e} on {int(bad_flip.sum())} of the {int(flip.sum())} voxels where the float oracle "
                                f"and its double twin disagree by a step (up to {err[bad_flip].max():.3e}): a row-end term was decided otherwise than "
                                f"the float oracle decides it")
    # Second bar, for the voxels off F over the first: two float32 evaluations of one sum of white-noise taps differ by the rounding of a
    # 2000-sample index on every tap, and neither is the truth.  The oracle's double-precision twin is (the same loops in
    # double on the same float32 DAS input).  Such a voxel passes only if the GPU is no further from that truth than the float ORACLE
    # gets from it anywhere off F on this frame, plus the bar -- never because another kernel of the library lands on the same value.
    # (Per voxel the two float errors are independent draws of one distribution -- asking the GPU to stay within the bar of the
    # oracle's error AT THE SAME VOXEL fails whenever the oracle was lucky there: 2 of round 4's 33 regression draws by 8 %.  The
    # maximum of the oracle's own error off F is the size of that distribution; on F it is a whole tap and no allowance.)
    second = over & ~flip
    rest = ok & ~flip
    oracle_off = float(oracle_err[rest].max()) if rest.any() else 0.0
    worst = None
    if second.any():
        excess = (np.abs(gpu[second].astype(exact.dtype) - exact[second]) - oracle_off) / scale
        worst = float(excess.max())
        assert (excess <= tol).all(), (f"max relative error {max_rel:.3e} > {tol:.0e}, and on {int((excess > tol).sum())} of {int(second.sum())} such voxels the GPU is "
                                       f"further from the double-precision truth than the float oracle ever is off the flip set on this frame "
                                       f"({oracle_off / scale:.3e}) by {worst:.3e} > {tol:.0e}")
    return _record(Verdict(max_rel, "second" if second.any() else "first", int(flip.sum()), int(second.sum()), worst), label, path)


def summary():
    """one line on LOG: how many comparisons needed the second bar, on how many voxels, and the flip sets' total size"""
    second = [e for e in LOG if e["bar"] == "second"]
    worst = max((e["worst_excess"] for e in second if e["worst_excess"] is not None), default=None)
    return (f"compare(): {len(LOG)} frames, {len(second)} needed the second bar ({sum(e['second_bar_voxels'] for e in second)} voxels"
            + (f", worst excess {worst:.2e}" if worst is not None else "") + f"), {sum(e['flip_voxels'] for e in LOG)} flip-set voxels in all")


@atexit.register
def _report():
    """at the end of a run that compared frames: the summary line on stderr, and LOG as JSON where BF_PARITY_LOG names a file"""
    if not LOG:
        return
    print(summary(), file=sys.stderr)
    where = os.environ.get("BF_PARITY_LOG")
    if where:
        second = [e for e in LOG if e["bar"] == "second"]
        with open(where, "w") as f:
            json.dump({"frames": len(LOG), "second_bar_frames": len(second), "flip_voxels": sum(e["flip_voxels"] for e in LOG),
                       "second_bar_voxels": sum(e["second_bar_voxels"] for e in second), "second_bar": second,
                       "with_flip_voxels": [e for e in LOG if e["flip_voxels"] and e["bar"] != "second"]}, f, indent=1)
