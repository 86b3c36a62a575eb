"""The parity comparison itself (tests/parity.py compare()) on the CPU: synthetic "GPU" frames built from the oracle's float frame and
its double-precision twin, each with a known verdict.  The frames are draws of the separable generator whose RF rows end inside the
image (tests/test_gpu_random.py ROW_END_SEPARABLE): on 241, 254, 259, 361 and 398 the float oracle and its twin keep or drop a row-end
term differently at one or two voxels -- a whole tap -- and the frame-wide rule of round 4 took that tap as its allowance everywhere.
96 has no such voxel."""
import functools

import numpy as np
import pytest

from tests import cases, draws, parity

FLIP_SEEDS = [241, 254, 259, 361, 398]
NO_FLIP_SEED = 96


@functools.lru_cache(maxsize=None)
def frames(seed):
    """(acq, float oracle frame, flags, its double twin computed on its own, valid mask, scale, tol, flip set)"""
    from oracle import binding
    acq = draws.draw_separable(seed)
    ref, _, flags = parity.reference(binding, acq)
    truth = {}
    again, _ = binding.beamform(acq.bp, acq.rf, acq.filters, truth=truth)
    assert np.array_equal(again, ref, equal_nan=True)
    exact = truth["frame"]
    ok = ~np.isnan(ref)
    scale = float(np.abs(ref[ok]).max())
    tol = cases.tolerance(acq)
    flip = ok & (np.abs(ref.astype(exact.dtype) - exact) > 1.5 * tol * scale)
    return acq, ref, flags, exact, ok, scale, tol, flip


def old_rule_accepts(gpu, ref, exact, ok, scale, tol):
    """round 4's rule (a copy): a voxel over the first bar passes if the GPU is within max_frame |oracle - truth| + tol * scale of the
    truth, the maximum taken over EVERY valid voxel"""
    err = np.abs(gpu - ref)
    if err[ok].max() <= tol * scale:
        return True
    over = ok & (err > tol * scale)
    oracle_off = np.abs(ref[ok].astype(exact.dtype) - exact[ok]).max()
    excess = (np.abs(gpu[over].astype(exact.dtype) - exact[over]) - oracle_off) / scale
    return bool((excess <= tol).all())


def unit(z):
    """z / |z| (complex or real), 1 where z is 0"""
    m = np.abs(z)
    return np.where(m > 0, z / np.where(m > 0, m, 1), 1)


def tap(seed):
    """one whole tap of this frame: the float oracle's distance from the truth at its worst flip voxel"""
    _, ref, _, exact, _, _, _, flip = frames(seed)
    return float(np.abs(ref[flip].astype(exact.dtype) - exact[flip]).max())


def quiet_voxel(seed):
    """a valid voxel off the flip set at which the float oracle is within 0.5 tol of the truth (the error class must be caught
    anywhere, so: a voxel at which nothing excuses it)"""
    _, ref, _, exact, ok, scale, tol, flip = frames(seed)
    e = np.where(ok & ~flip, np.abs(ref.astype(exact.dtype) - exact), np.inf)
    cands = np.argwhere(e <= 0.5 * tol * scale)
    assert len(cands)
    return tuple(cands[len(cands) // 2])


@pytest.mark.parametrize("seed", FLIP_SEEDS + [NO_FLIP_SEED])
def test_the_float_oracle_passes_on_the_first_bar(seed):
    acq, ref, flags, exact, ok, scale, tol, flip = frames(seed)
    v = parity.compare(ref.copy(), ref, acq, flags, label=f"separable/{seed}")
    assert v.bar == "first" and v.max_rel_err == 0.0 and v.second_bar_voxels == 0 and v.worst_excess is None
    assert v.flip_voxels == int(flip.sum())
    assert (1 <= v.flip_voxels <= 2) if seed in FLIP_SEEDS else v.flip_voxels == 0
    assert parity.LOG[-1]["test"] == f"separable/{seed}" and parity.LOG[-1]["flip_voxels"] == v.flip_voxels


@pytest.mark.parametrize("seed", FLIP_SEEDS)
def test_a_whole_tap_off_the_flip_set_is_rejected(seed):
    """the float oracle plus one tap (the size of the frame's own flip) at a voxel off F: round 4's rule took the flip as the allowance
    of every voxel and accepted the frame; the per-voxel rule does not"""
    acq, ref, flags, exact, ok, scale, tol, flip = frames(seed)
    size = tap(seed)
    assert size > 6 * tol * scale                              # the gap: an allowance of more than six times the bar
    at = quiet_voxel(seed)
    gpu = ref.copy()
    gpu[at] += (size * unit(ref[at] - exact[at])).astype(ref.dtype)
    assert old_rule_accepts(gpu, ref, exact, ok, scale, tol)
    with pytest.raises(AssertionError, match="further from the double-precision truth"):
        parity.compare(gpu, ref, acq, flags)


@pytest.mark.parametrize("seed", FLIP_SEEDS)
def test_the_truth_on_the_flip_set_is_rejected(seed):
    """at a voxel of F the frame must be the float oracle's (row-end terms decided bit for bit as the oracle's float
    build decides them): a kernel that lands on the double truth there -- one tap from the oracle -- decided the term otherwise"""
    acq, ref, flags, exact, ok, scale, tol, flip = frames(seed)
    for at in map(tuple, np.argwhere(flip)):
        gpu = ref.copy()
        gpu[at] = exact[at]
        assert old_rule_accepts(gpu, ref, exact, ok, scale, tol)
        with pytest.raises(AssertionError, match="disagree by a step"):
            parity.compare(gpu, ref, acq, flags)


@pytest.mark.parametrize("seed", FLIP_SEEDS + [NO_FLIP_SEED])
def test_noise_under_the_bar_passes_on_the_first_bar(seed):
    acq, ref, flags, exact, ok, scale, tol, flip = frames(seed)
    rng = np.random.default_rng(seed)
    if np.iscomplexobj(ref):
        noise = np.exp(2j * np.pi * rng.random(ref.shape))
    else:
        noise = rng.choice([-1.0, 1.0], ref.shape)
    gpu = (ref + 0.9 * tol * scale * noise).astype(ref.dtype)
    v = parity.compare(gpu, ref, acq, flags)
    assert v.bar == "first" and v.second_bar_voxels == 0 and 0.85 * tol < v.max_rel_err <= tol
    assert v.flip_voxels == int(flip.sum())


@pytest.mark.parametrize("seed", [361, NO_FLIP_SEED])
def test_a_frame_closer_to_the_truth_passes_on_the_second_bar(seed):
    """1.2 tol from the float oracle, towards the truth, at the voxels off F where the oracle is at least 0.3 tol from the truth: within
    oracle_off + tol of the truth there, so the second bar takes exactly those voxels (the float32 frames with a 1e-4 bar, where the
    oracle's own error is of the bar's size)"""
    acq, ref, flags, exact, ok, scale, tol, flip = frames(seed)
    e = np.where(ok & ~flip, np.abs(ref.astype(exact.dtype) - exact), 0.0)
    moved = e >= 0.3 * tol * scale
    assert moved.sum() >= 3
    gpu = ref.copy()
    gpu[moved] = (ref[moved] + 1.2 * tol * scale * unit(exact[moved] - ref[moved])).astype(ref.dtype)
    assert (np.abs(gpu[moved] - ref[moved]) > tol * scale).all()
    v = parity.compare(gpu, ref, acq, flags)
    assert v.bar == "second" and v.second_bar_voxels == int(moved.sum()) and v.flip_voxels == int(flip.sum())
    assert v.worst_excess is not None and v.worst_excess <= tol
    # the same frame pushed 1.2 tol AWAY from the truth at those voxels is refused
    gpu[moved] = (ref[moved] - 1.2 * tol * scale * unit(exact[moved] - ref[moved])).astype(ref.dtype)
    with pytest.raises(AssertionError, match="further from the double-precision truth"):
        parity.compare(gpu, ref, acq, flags)


def test_the_twin_bar_sees_what_the_pipeline_bar_cannot():
    """rca_staged_auto (Int16 + Demodulate: 2e-3) and its DAS-only twin (tests/twins.py: 1e-4): the same error of 5e-4 of the frame
    maximum, planted at one valid voxel with no row-end mark, passes on the original and is refused on the twin"""
    from oracle import binding
    from tests import twins
    acq = cases.make("rca_staged_auto")
    twin, ref, _, _ = twins.oracle_twin(binding, acq)
    twin_ref, _, twin_flags = parity.reference(binding, twin)
    assert np.array_equal(twins.bits(twin_ref), twins.bits(ref))
    assert cases.tolerance(acq) == 2e-3 and cases.tolerance(twin) == 1e-4
    ok = ~np.isnan(ref)
    scale = float(np.abs(ref[ok]).max())
    marks = parity.row_end_marks(twin, twin_ref.shape, twin_ref)
    cands = np.argwhere(ok & ~marks)
    at = tuple(cands[len(cands) // 2])
    planted = ref.copy()
    planted[at] += ref.dtype.type(5e-4 * scale)
    v = parity.compare(planted, ref, acq, None)
    assert v.bar == "first" and 4e-4 < v.max_rel_err < 6e-4
    planted_twin = twin_ref.copy()
    planted_twin[at] += twin_ref.dtype.type(5e-4 * scale)
    with pytest.raises(AssertionError, match="further from the double-precision truth"):
        parity.compare(planted_twin, twin_ref, twin, twin_flags)


def test_the_flips_are_at_row_ends_and_rounding_alone_is_not_a_flip():
    """the oracle marks the voxels that hold a term within float rounding of an end of its RF row: every voxel of the row-end draws at
    which it is more than 1.5 tol from its twin is one of them.  On draw_paired 14 (Int16Complex with coherency weighting, 1e-4 bar, no row
    ends in the image) the float oracle's rounding alone reaches 1.55 tol at one voxel: that voxel is no flip, and a frame 1.05 tol from the
    oracle there -- as the paired kernel's own rounding lands -- passes on the second bar"""
    from oracle import binding
    for seed in FLIP_SEEDS:
        acq, ref, flags, exact, ok, scale, tol, flip = frames(seed)
        assert (parity.row_end_marks(acq, ref.shape, ref) >= flip).all()
    acq = draws.draw_paired(14)
    ref, _, flags = parity.reference(binding, acq)
    exact = parity.truth_frame(acq, ref.shape, ref)
    ok = ~np.isnan(ref)
    scale, tol = float(np.abs(ref[ok]).max()), cases.tolerance(acq)
    e = np.where(ok, np.abs(ref.astype(exact.dtype) - exact), 0.0)
    at = np.unravel_index(np.argmax(e), e.shape)
    assert e[at] > 1.5 * tol * scale and not parity.row_end_marks(acq, ref.shape, ref).any()
    gpu = ref.copy()
    gpu[at] = (ref[at] + 1.05 * tol * scale * unit(exact[at] - ref[at])).astype(ref.dtype)
    v = parity.compare(gpu, ref, acq, flags)
    assert v.flip_voxels == 0 and v.bar == "second" and v.second_bar_voxels == 1
