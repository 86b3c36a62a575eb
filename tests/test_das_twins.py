"""The DAS-only twins (tests/twins.py) on the CPU: for every binary16-staged named case the twin built from the oracle's own DAS-input
capture has the original's DAS plan and the original's frame, bit for bit, and is judged at 1e-4; the oracle alone stays within
compare()'s rules on it; and the library's kernel selection (beamformer_hip_describe_das: needs no device) routes the twin as it routes
the original under every das path mode the GPU tests use."""
import functools

import numpy as np
import pytest

from tests import cases, draws, parity, twins

F16_STAGED = sorted(n for n in cases.CASES if twins.is_f16_staged(cases.make(n)))
# every das path mode tests/test_gpu_das_twins.py pushes under
MODES = (0, 1, 2, 3, 6, 0x04, 0x14, 0x14 | 0x100, 0x11, 0x10 | 0x100)


def test_the_binary16_staged_cases_are_the_ones_counted():
    assert len(cases.CASES) == 68 and len(F16_STAGED) == 50
    for name in ("config1_small", "config2_small", "config3_small", "config4_small", "config5_small", "rca_staged_auto", "tile_tpw",
                 "harness_tpw_small", "hercules_plane_yz", "hercules_real"):
        assert name in F16_STAGED


@functools.lru_cache(maxsize=None)
def built(name):
    """(original, twin from the oracle's capture and plan, the oracle's frame of the original)"""
    from oracle import binding
    acq = cases.make(name)
    twin, ref, _, _ = twins.oracle_twin(binding, acq)
    return acq, twin, ref


@pytest.mark.parametrize("name", F16_STAGED)
def test_the_twin_is_exact(name, oracle):
    acq, twin, ref = built(name)
    plan, twin_plan = oracle.plan(acq.bp, acq.filters), oracle.plan(twin.bp, twin.filters)
    for field, _ in twins.PLAN_FIELDS:
        a, b = getattr(plan, field), getattr(twin_plan, field)
        if hasattr(a, "__len__"):
            a, b = list(a), list(b)
        assert a == b, (field, a, b)
    assert [int(s.kind) for s in twin_plan.stages[:twin_plan.stage_count]][0] == 3          # DAS first: no stage runs before it
    assert cases.tolerance(acq) == 2e-3 and cases.tolerance(twin) == 1e-4
    captured = {}
    twin_ref, _ = oracle.beamform(twin.bp, twin.rf, twin.filters, das_input=captured)
    assert twin_ref.dtype == ref.dtype and np.array_equal(twins.bits(twin_ref), twins.bits(ref)), "the oracle's frame of the twin is not its frame of the original"
    assert np.array_equal(twins.bits(captured["data"]), twins.bits(twin.rf.reshape(captured["data"].shape))), "the twin's DAS input is not its RF"


@pytest.mark.parametrize("name", F16_STAGED)
def test_the_oracle_alone_meets_the_rule_on_the_twin(name, oracle):
    """the float oracle is up to 1.3e-4 of the frame maximum from its double twin on these frames: over the 1e-4 bar, which is
    what compare()'s second bar exists for -- the reference itself must pass, with an empty flip set"""
    _, twin, _ = built(name)
    ref, _, flags = parity.reference(oracle, twin)
    v = parity.compare(ref.copy(), ref, twin, flags, path=-1)
    assert v.max_rel_err == 0.0 and v.bar == "first" and v.flip_voxels == 0


def zero_twin(oracle, acq):
    """the twin with an all-zero DAS input: the kernel selection reads parameters only"""
    plan = oracle.plan(acq.bp, acq.filters)
    shape = (int(acq.bp.channel_count), int(acq.bp.acquisition_count), int(plan.input_sample_count))
    return twins.das_twin(acq, np.zeros(shape, np.complex64 if plan.iq_pipeline else np.float32), plan.input_sample_count,
                          plan.das_sampling_frequency, plan.das_time_offset)


def assert_same_plan_and_route(oracle, acq, twin, modes, hook_settings=((),)):
    import ctypes as C

    from ogl_beamforming_amd import lib, params as P
    L = lib.library()
    try:
        for hooks in hook_settings:
            for hook, value in hooks:
                lib.set_hook(hook, value)
            for mode in modes:
                L.beamformer_hip_set_das_path(mode)
                seen = []
                for which in (acq, twin):
                    d = lib.describe_das(which.bp, which.filters)[4]
                    plan = P.HipPlan()
                    assert L.beamformer_hip_describe_plan(0, C.byref(plan)), lib.last_error()
                    seen.append((twins.route(d), plan))
                (route, plan), (twin_route, twin_plan) = seen
                assert route == twin_route, (acq.name, hex(mode), hooks, {k: (route[k], twin_route[k]) for k in route if route[k] != twin_route[k]})
                for _, field in twins.PLAN_FIELDS:
                    if field is None:
                        continue
                    a, b = getattr(plan, field), getattr(twin_plan, field)
                    if hasattr(a, "__len__"):
                        a, b = list(a), list(b)
                    assert a == b, (acq.name, field, a, b)
                assert [int(s.kind) for s in twin_plan.stages[:twin_plan.stage_count]][0] == 3
            for hook, _ in hooks:
                lib.set_hook(hook, None)
    finally:
        L.beamformer_hip_set_das_path(0)
        for hooks in hook_settings:
            for hook, _ in hooks:
                lib.set_hook(hook, None)


STAGED_HOOKS = ((), (("STAGED_CHECKED", "1"),), (("STAGED_SHAPE", "6,4,5"),), (("STAGED_SHAPE", "6,4,6"),),
                (("STAGED_SHAPE", "6,4,5"), ("STAGED_NOUNIFORM", "1")), (("STAGED_SHAPE", "6,4,6"), ("STAGED_NOUNIFORM", "1")))


@pytest.mark.parametrize("name", F16_STAGED)
def test_the_library_routes_the_twin_as_the_original(name, oracle):
    """the library's plan of the twin agrees with its plan of the original in the DAS fields, and beamformer_hip_describe_das describes
    the same launch for both under every mode and staged-kernel hook of the GPU twin tests: a twin is not silently re-routed"""
    acq = cases.make(name)
    twin = zero_twin(oracle, acq)
    assert_same_plan_and_route(oracle, acq, twin, MODES)
    assert_same_plan_and_route(oracle, acq, twin, (3,), STAGED_HOOKS[1:])


@pytest.mark.parametrize("generator,modes", [(draws.draw_separable, (0,)), (draws.draw_tile, (0x10 | 0x100,))], ids=["separable", "tile"])
def test_the_library_routes_the_twins_of_the_int16_draws_as_the_originals(generator, modes, oracle):
    checked = 0
    for seed in range(32):
        acq = generator(seed)
        if not twins.is_f16_staged(acq):         # (the separable generator's real-sample draws: Int16 straight into DAS, already at 1e-4)
            continue
        assert_same_plan_and_route(oracle, acq, zero_twin(oracle, acq), modes, STAGED_HOOKS[:2])
        checked += 1
    assert checked >= 20, checked
