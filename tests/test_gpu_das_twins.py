"""The DAS kernels at 1e-4 on IQ data: every binary16-staged case is pushed as it stands -- judged at 2e-3 of the frame
maximum by the parity tests -- and again as its DAS-only twin (tests/twins.py): the DAS input the library itself produced, pushed as
Float32 / Float32Complex RF with the plan's DAS arguments and no stage in front of DAS.  On every route the suite already drives these
cases through (the case lists and das path modes of tests/test_gpu_parity.py, the Int16-only generators of tests/draws.py):
  (a) same route   beamformer_hip_describe_das describes the same launch for the twin as for the original, and the same kernel ran;
  (b) same frame   the twin's frame is the original's, bit for bit: DAS depends on its arguments and its input's bits alone;
  (c) parity       the twin's frame against the oracle's frame of the twin by the unchanged compare(): 1e-4.
Every twin is pushed with the SCRATCH_POISON hook set.  The oracle runs once per case: the DAS input does not depend on the das path."""
import ctypes as C

import numpy as np
import pytest

from ogl_beamforming_amd import params as P
from tests import cases, draws, parity, twins
from tests.das_kernel_cases import FACTORED, HERCULES, SEPARABLE, STAGED, TILE
from tests.das_push import last_timings

pytestmark = pytest.mark.gpu

F16_STAGED = sorted(n for n in cases.CASES if twins.is_f16_staged(cases.make(n)))


def staged_only(names):
    """a (case, route) pair is left out only where the original is not binary16-staged (its parity test already holds it to 1e-4)"""
    return sorted(n for n in names if n in F16_STAGED)


_TWINS = {}                 # case key -> (twin, the oracle's frame of the twin, flags): built from the first push of the case
STAGED_TWIN_RUNS = []       # (seed, uniform_tables) of the separable draws whose twin ran the LDS-staged kernel
TILE_TWIN_RUNS = []         # (seed, staged chunks, gathered chunks) of the tile draws whose twin ran das_tile.hip


class EmptyImage(Exception):
    pass


def push(bflib, acq, mode):
    """(frame, timings, route as described, DAS input) of one push under das path `mode` (hooks as the caller set them)"""
    L = bflib.library()
    L.beamformer_hip_set_das_path(mode)
    try:
        route = twins.route(bflib.describe_das(acq.bp, acq.filters)[4])
        frame = np.asarray(bflib.beamform(acq.bp, acq.rf, acq.filters)).copy()
        t = last_timings(bflib)
        das_in = bflib.das_input(acq.bp)
        plan = P.HipPlan()
        assert L.beamformer_hip_describe_plan(0, C.byref(plan)), bflib.last_error()
    finally:
        L.beamformer_hip_set_das_path(0)
    return frame, t, route, das_in, plan


def check_twin(bflib, oracle, hooks, key, acq, mode, set_hooks=(), skip_empty=False):
    """(a), (b) and (c) for `acq` under das path `mode` with the hooks `set_hooks` ((name, value) pairs) on both pushes; returns
    (verdict, the twin push's timings, the described route)"""
    assert twins.is_f16_staged(acq)
    for name, value in set_hooks:
        hooks.set(name, value)
    hooks.clear("SCRATCH_POISON")
    frame, t, route, das_in, plan = push(bflib, acq, mode)
    assert not np.isnan(das_in).any(), "the original's DAS input holds NaN"
    if key not in _TWINS:
        twin = twins.das_twin(acq, das_in, plan.das_samples, plan.das_sampling_frequency, plan.das_time_offset)
        assert cases.tolerance(twin) == 1e-4
        _TWINS[key] = (twin,) + tuple(parity.reference(oracle, twin)[i] for i in (0, 2))
    twin, ref, flags = _TWINS[key]
    assert np.array_equal(twins.bits(das_in), twins.bits(twin.rf.reshape(das_in.shape))), "the DAS input depends on the das path or the hooks"
    ok = ~np.isnan(ref)
    if skip_empty and (not ok.any() or np.max(np.abs(ref[ok])) == 0):
        raise EmptyImage
    hooks.set("SCRATCH_POISON")
    try:
        twin_frame, twin_t, twin_route, twin_in, twin_plan = push(bflib, twin, mode)
    finally:
        hooks.clear("SCRATCH_POISON")
    # (a) same route
    assert twin_route == route, {k: (route[k], twin_route[k]) for k in route if route[k] != twin_route[k]}
    assert int(twin_t.das_path) == int(t.das_path) and int(twin_t.das_row_end_planes) == int(t.das_row_end_planes), \
        (int(t.das_path), int(twin_t.das_path), int(t.das_row_end_planes), int(twin_t.das_row_end_planes))
    assert int(twin_plan.stages[0].kind) == int(P.ShaderKind.DAS), "a stage ran before the twin's DAS"
    assert np.array_equal(twins.bits(twin_in), twins.bits(das_in)), "the twin's DAS stage did not read the original's DAS input"
    # (b) same frame
    assert twin_frame.dtype == frame.dtype and twin_frame.shape == frame.shape
    diff = twins.bits(twin_frame) != twins.bits(frame)
    assert not diff.any(), (f"{int(diff.sum())} scalars of the twin's frame differ from the original's in their bits (DAS path {int(t.das_path)}): the DAS stage "
                            f"depends on something besides its arguments and its input")
    # (c) parity at 1e-4
    try:
        v = parity.compare(twin_frame, ref, twin, flags, path=int(twin_t.das_path))
    finally:
        scale = float(np.abs(ref[ok]).max()) if ok.any() else 1.0
        err = float(np.abs(twin_frame - ref)[ok].max() / scale) if ok.any() and scale > 0 else 0.0
        print(f"{key} mode {mode:#x} {dict(set_hooks)} DAS path {int(twin_t.das_path)}: max_rel_err {err:.3e}", end="")
    print(f", bar {v.bar} ({v.rule}; {v.second_bar_voxels} second-bar voxels, {v.flip_voxels} flip-set voxels)")
    return v, twin_t, route


# ------------------------------------------------------------------------------------------------ named cases

@pytest.mark.parametrize("name", F16_STAGED)
def test_twin_on_the_automatic_path(name, bflib, oracle, hooks):
    acq = cases.make(name)
    _, t, _ = check_twin(bflib, oracle, hooks, name, acq, 0)
    if name in cases.EXPECTED_AUTOMATIC:
        assert int(t.das_path) == cases.EXPECTED_AUTOMATIC[name]


@pytest.mark.parametrize("name", staged_only(SEPARABLE))
def test_twin_on_the_general_kernel_on_separable_geometry(name, bflib, oracle, hooks):
    _, t, _ = check_twin(bflib, oracle, hooks, name, cases.make(name), 1)
    assert int(t.das_path) == 0


@pytest.mark.parametrize("name", staged_only(STAGED))
def test_twin_on_the_gather_kernel_where_the_staged_kernel_applies(name, bflib, oracle, hooks):
    acq = cases.make(name)
    _, t, _ = check_twin(bflib, oracle, hooks, name, acq, 2)
    assert int(t.das_path) in (1, 3)
    if acq.bp.interpolation_mode == int(P.InterpolationMode.Linear):
        assert int(t.das_path) == 1


@pytest.mark.parametrize("name", staged_only(SEPARABLE))
def test_twin_on_the_lds_staged_kernel(name, bflib, oracle, hooks):
    _, t, _ = check_twin(bflib, oracle, hooks, name, cases.make(name), 3)
    assert int(t.das_path) == (2 if name in STAGED and name not in cases.ROW_END_EVERY_PLANE else 1)


@pytest.mark.parametrize("name", staged_only(STAGED))
def test_twin_on_the_lds_staged_kernel_checked_loop_everywhere(name, bflib, oracle, hooks):
    _, t, _ = check_twin(bflib, oracle, hooks, name, cases.make(name), 3, (("STAGED_CHECKED", "1"),))
    assert int(t.das_path) == (1 if name in cases.ROW_END_EVERY_PLANE else 2)
    assert int(t.staged_window_violations) == 0, "a term left its staged window: plan_staged's bound is wrong"


@pytest.mark.parametrize("tables", ["uniform", "lds"])
@pytest.mark.parametrize("shape", ["6,4,5", "6,4,6"])
@pytest.mark.parametrize("name", staged_only(["rca_staged_fine", "rca_staged_fine_vls_short_rows", "rca_staged_auto"]))
def test_twin_on_the_lds_staged_kernel_uniform_and_lds_tables(name, shape, tables, bflib, oracle, hooks):
    """64 x 16 tiles: the wave-uniform form (transmit tables in global memory, scalar loads) and, with STAGED_NOUNIFORM, the LDS-table form"""
    set_hooks = (("STAGED_SHAPE", shape),) + ((("STAGED_NOUNIFORM", "1"),) if tables == "lds" else ())
    _, t, route = check_twin(bflib, oracle, hooks, name, cases.make(name), 3, set_hooks)
    if int(t.das_path) == 2:
        assert route["uniform_tables"] == (1 if tables == "uniform" else 0)
    if name == "rca_staged_fine":
        assert int(t.das_path) == 2


@pytest.mark.parametrize("name", staged_only(HERCULES))
def test_twin_on_the_hercules_aligned_kernel(name, bflib, oracle, hooks):
    _, t, _ = check_twin(bflib, oracle, hooks, name, cases.make(name), 6)
    assert int(t.das_path) == 4


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("name", staged_only(FACTORED))
def test_twin_on_the_factored_kernel(name, split, bflib, oracle, hooks):
    _, t, _ = check_twin(bflib, oracle, hooks, name, cases.make(name), 0x04 if split else 0x14)
    assert int(t.das_path) == 3


@pytest.mark.parametrize("name", staged_only(TILE))
def test_twin_on_the_block_staged_kernel(name, bflib, oracle, hooks):
    _, t, _ = check_twin(bflib, oracle, hooks, name, cases.make(name), 0x14 | 0x100)
    assert int(t.das_path) == 5 and int(t.tile_staged_chunks) + int(t.tile_gather_chunks) > 0


@pytest.mark.parametrize("name", F16_STAGED)
def test_twin_on_the_general_kernel_without_channel_split(name, bflib, oracle, hooks):
    _, t, _ = check_twin(bflib, oracle, hooks, name, cases.make(name), 0x11)
    assert int(t.das_path) == 0


def test_every_route_has_its_cases():
    """the case lists above are those of tests/test_gpu_parity.py less the cases that are not binary16-staged: none may be empty by accident"""
    assert len(F16_STAGED) == 50
    assert len(staged_only(SEPARABLE)) >= 13 and len(staged_only(STAGED)) >= 11 and len(staged_only(HERCULES)) >= 12
    assert len(staged_only(FACTORED)) >= 20 and len(staged_only(TILE)) >= 10
    assert {"hercules_plane_xz", "hercules_plane_yz", "hercules_wide_cubic_cw"} <= set(staged_only(HERCULES))       # the prepared-copy path on Int16 input


# ------------------------------------------------------------------------------------------------ the Int16-only generators

SEPARABLE_SEEDS = [s for s in range(32) if twins.is_f16_staged(draws.draw_separable(s))]     # (the real-sample draws go straight into DAS: 1e-4 already)


@pytest.mark.parametrize("seed", SEPARABLE_SEEDS)
def test_twin_of_a_random_separable_acquisition(seed, bflib, oracle, hooks):
    acq = draws.draw_separable(seed)
    try:
        _, t, route = check_twin(bflib, oracle, hooks, f"separable/{seed}", acq, 0, skip_empty=True)
    except EmptyImage:
        pytest.skip("empty image")
    if int(t.das_path) == 2:
        _, t, _ = check_twin(bflib, oracle, hooks, f"separable/{seed}", acq, 0, (("STAGED_CHECKED", "1"),))
        assert int(t.das_path) == 2 and int(t.staged_window_violations) == 0, "a term left its staged window: plan_staged's bound is wrong"
        STAGED_TWIN_RUNS.append((seed, route["uniform_tables"]))


@pytest.mark.parametrize("seed", range(32))
def test_twin_of_a_random_acquisition_on_the_block_staged_kernel(seed, bflib, oracle, hooks):
    acq = draws.draw_tile(seed)
    try:
        _, t, _ = check_twin(bflib, oracle, hooks, f"tile/{seed}", acq, 0x10 | 0x100, skip_empty=True)
    except EmptyImage:
        pytest.skip("empty image")
    if int(t.das_path) == 5:
        TILE_TWIN_RUNS.append((seed, int(t.tile_staged_chunks), int(t.tile_gather_chunks)))


def test_twin_draws_reach_the_staged_and_block_staged_kernels():
    """the counts tests/test_gpu_random.py requires of the same seeds"""
    print(f"staged twin draws: {len(STAGED_TWIN_RUNS)}: {STAGED_TWIN_RUNS}")
    print(f"block-staged twin draws: {len(TILE_TWIN_RUNS)}: {TILE_TWIN_RUNS}")
    assert len(STAGED_TWIN_RUNS) >= 12, STAGED_TWIN_RUNS
    assert len(TILE_TWIN_RUNS) >= 20, TILE_TWIN_RUNS


def test_worst_twin_error_per_das_path():
    """what DESIGN.md 4 quotes: the largest max_rel_err of the twin runs of this module per DAS path, and how many needed the second bar"""
    mine = [e for e in parity.LOG if e["test"] and "test_gpu_das_twins" in e["test"]]
    assert mine, "reports the twin runs of this module: run it with them"
    for path in sorted({e["das_path"] for e in mine}):
        rows = [e for e in mine if e["das_path"] == path]
        worst = max(rows, key=lambda e: e["max_rel_err"])
        second = [e for e in rows if e["bar"] == "second"]
        excess = max((e["worst_excess"] for e in second if e["worst_excess"] is not None), default=None)
        print(f"DAS path {path} ({P.DasPath(path).name}): {len(rows)} twin frames, worst max_rel_err {worst['max_rel_err']:.3e} ({worst['test']}), "
              f"{len(second)} on the second bar" + (f" (worst excess {excess:.2e})" if excess is not None else ""))
