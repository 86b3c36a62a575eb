"""The pre-DAS pipeline matrix on the device (tests/pipeline_cases.py: the curated list and the kept random draws).  Every pipeline
first passes the host extent audit -- no stage writes past its inter-stage buffer -- and is then pushed with SCRATCH_POISON set:
  1. the DAS input against the oracle's, element by element: bit-identical where every stage is exact, else inside the propagated
     forward-error bound of tests/test_gpu_stages.py (stage_bounds; an Int16 store adds 1 in the stored unit); err / bar is printed;
  2. the frame: compare() with cases.tolerance, unchanged -- or, where a stage stored Int16 inexactly, within
     tol x max|oracle| + C x A x max(DAS-input bar): apodization and linear weights lie in [0, 1], at most C x A terms a voxel;
  3. the poisoned frame equals an unpoisoned push bit for bit (an element read without having been written shows as NaN in 1.).
Then: a filter slot replaced between two pushes, a long chain around a one-stage plan (order independence), long chains inside a burst,
and under frame graphs.  The last test prints the worst err / bar by stage and store kind."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from ogl_beamforming_amd import configs as cfg
from ogl_beamforming_amd import params as P
from tests import cases
from tests import pipeline_cases as pc
from tests import stage_checks as stages
from tests.das_push import compare, noise_frames

pytestmark = pytest.mark.gpu

S = P.ShaderKind
DK = P.DataKind
as_bits = stages.as_bits
# (stage, store kind) -> (largest err / bar at the DAS input of any pipeline that HOLDS such a stage, its name): the ratio is measured
# once per pipeline, behind all of its stages -- the table says which kinds of stage lie on the worst pipelines, not what each adds
WORST = {}


def inexact_int16_store(plan):
    return any(int(plan.stages[i].kind) in pc.PRE_DAS and (int(plan.stages[i].out_kind) >> 1) == 0 for i in range(plan.stage_count))


def run_pipeline(bflib, oracle, hooks, acq, reference=None):
    plan = stages.plan_of(bflib, acq)
    pc.audit(plan, acq.bp)
    ref, flags, ref_in = reference if reference is not None else stages.oracle_run(oracle, acq)
    gpu, gpu_in = stages.push(bflib, acq, hooks, poison=True)
    verdict, ratio = stages.check_das_input(bflib, oracle, acq, gpu_in, ref_in, acq.name)
    for i in range(plan.stage_count):
        st = plan.stages[i]
        if int(st.kind) in pc.PRE_DAS:
            key = (S(int(st.kind)).name, DK(int(st.out_kind)).name)
            if ratio >= WORST.get(key, (-1.0, ""))[0]:
                WORST[key] = (ratio, acq.name)
    if verdict == "bound" and inexact_int16_store(plan):
        _, _, bar = stages.stage_bounds(bflib, oracle, acq, plan)
        ok = ~np.isnan(ref)
        assert np.array_equal(np.isnan(gpu), ~ok)
        scale = float(np.abs(ref[ok]).max())
        assert scale > 0, "oracle image is empty: the case does not exercise the path"
        allowed = cases.tolerance(acq) * scale + int(acq.bp.channel_count) * int(acq.bp.acquisition_count) * float(bar.max())
        err = float(np.abs(gpu[ok] - ref[ok]).max())
        print(f"{acq.name}: frame max error {err:.3e}, allowed {allowed:.3e} (max|oracle| {scale:.3e})")
        assert err <= allowed
    else:
        compare(gpu, ref, acq, flags)
    clean, clean_in = stages.push(bflib, acq, hooks, poison=False)
    assert np.array_equal(as_bits(gpu_in), as_bits(clean_in)), "the DAS input depends on what the scratch buffers held"
    diff = as_bits(gpu) != as_bits(clean)
    assert not diff.any(), f"{int(diff.sum())} frame scalars differ from the unpoisoned push (unwritten voxels keep 0xFFFFFFFF)"
    return gpu, gpu_in, verdict


@pytest.mark.parametrize("name", sorted(pc.BY_NAME))
def test_curated_pipeline(name, bflib, oracle, hooks):
    run_pipeline(bflib, oracle, hooks, pc.build(pc.BY_NAME[name]))


@pytest.mark.parametrize("seed", list(pc.RANDOM_SEEDS))
def test_random_pipeline(seed, bflib, oracle, hooks):
    k = pc.kept(bflib, oracle, pc.draw_pipeline(seed))
    if isinstance(k, str):
        print(f"draw{seed:02d} DROPPED, nothing ran: {k}")  # (tests/test_pipelines_host.py bounds how many)
        return
    acq, ref, flags, ref_in = k
    run_pipeline(bflib, oracle, hooks, acq, (ref, flags, ref_in))


# ------------------------------------------------------------------------------------------------ slot replacement

def test_a_replaced_filter_slot_is_what_the_next_push_reads(bflib, oracle, hooks):
    """slot 1 holds the chirp for the first push and a 21-tap Kaiser for the second; nothing else is pushed in between"""
    L = bflib.library()
    acq = pc.build(pc.BY_NAME["f32_demod_filter"])
    assert 1 in acq.bp.compute_stage_parameters[:2]
    _, first_in = stages.push(bflib, acq, hooks, poison=True)
    stages.check_das_input(bflib, oracle, acq, first_in, stages.oracle_run(oracle, acq)[2], "before the replacement")
    replaced = list(acq.filters)
    replaced[1] = cfg.kaiser_filter(pc.FS / 2, pc.FD / 2, length=21, beta=4.0)
    assert L.beamformer_create_filter(C.byref(replaced[1]), 1, 0)
    rf = np.ascontiguousarray(acq.rf)
    assert L.beamformer_push_data_with_compute(rf.ctypes.data_as(C.c_void_p), rf.nbytes, 0, 0), bflib.last_error()
    second_in = bflib.das_input(acq.bp)
    after = dataclasses.replace(acq, filters=replaced)
    assert not np.array_equal(as_bits(first_in), as_bits(second_in))
    stages.check_das_input(bflib, oracle, after, second_in, stages.oracle_run(oracle, after)[2], "after the replacement")


# ------------------------------------------------------------------------------------------------ order independence

def test_a_long_chain_does_not_depend_on_the_plan_before_it(bflib, hooks):
    hooks.clear("SCRATCH_POISON")
    chain = pc.build(pc.BY_NAME["f32_decode_filter_decode_filter_filter"])
    assert sum(int(stages.plan_of(bflib, chain).stages[i].kind) in pc.PRE_DAS for i in range(6)) == 6
    first, first_in = stages.push(bflib, chain)
    stages.push(bflib, pc.build(pc.BY_NAME["i16_filter"]))
    again, again_in = stages.push(bflib, chain)
    assert np.array_equal(as_bits(first_in), as_bits(again_in)), "the DAS input depends on what ran before it"
    assert np.array_equal(as_bits(first), as_bits(again)), "the frame depends on what ran before it"


# ------------------------------------------------------------------------------------------------ bursts

@pytest.mark.parametrize("name", pc.LONG_CHAINS)
def test_long_chain_in_a_burst(name, bflib, hooks):
    acq = pc.build(pc.BY_NAME[name])
    pc.audit(stages.plan_of(bflib, acq), acq.bp)
    rf = noise_frames(acq, 3, 9900 + pc.LONG_CHAINS.index(name))
    if rf.dtype.kind == "i":
        rf = (rf // 8).astype(rf.dtype)
    _, inputs, _ = stages.push_burst(bflib, hooks, acq, rf, 0)
    for k in range(3):
        stages.nan_free(acq, inputs[k], f"{name} burst frame {k}")
        _, one_in = stages.push(bflib, dataclasses.replace(acq, rf=rf[k]), hooks, poison=True)
        assert np.array_equal(as_bits(inputs[k]), as_bits(one_in)), \
            f"{name}: burst frame {k}'s DAS input is not its single push's: {stages.first_difference(inputs[k], one_in)}"


# ------------------------------------------------------------------------------------------------ frame graphs

def test_long_chain_under_frame_graphs(bflib, hooks):
    hooks.clear("SCRATCH_POISON")
    L = bflib.library()
    acq = pc.build(pc.BY_NAME["i16_demod_filter_decode_filter_decode"])
    direct, direct_in = stages.push(bflib, acq)
    rf = np.ascontiguousarray(acq.rf)
    replayed0, replayed, built = C.c_uint64(), C.c_uint64(), C.c_uint64()
    L.beamformer_hip_frame_graph_counts(C.byref(replayed0), C.byref(built))
    try:
        L.beamformer_hip_enable_frame_graphs(1)
        for _ in range(3):                                   # (a plan's first frame never runs from a graph)
            assert L.beamformer_push_data_with_compute(rf.ctypes.data_as(C.c_void_p), rf.nbytes, 0, 0), bflib.last_error()
        graphed, graphed_in = bflib.get_last_frame(acq.bp), bflib.das_input(acq.bp)
    finally:
        L.beamformer_hip_enable_frame_graphs(0)
    L.beamformer_hip_frame_graph_counts(C.byref(replayed), C.byref(built))
    assert replayed.value > replayed0.value, "no frame ran from a graph"
    assert np.array_equal(as_bits(direct_in), as_bits(graphed_in))
    assert np.array_equal(as_bits(direct), as_bits(graphed))


# ------------------------------------------------------------------------------------------------ the table

def test_zz_worst_ratio_by_stage_and_store_kind():
    """prints what the tests above measured (run after them), per (stage, store kind) the worst DAS-input err / bar over the pipelines
    that hold such a stage; asserts nothing new: every pipeline has met its bar"""
    for (stage, kind), (ratio, name) in sorted(WORST.items()):
        print(f"worst err/bar of a pipeline with  {stage:<10} storing {kind:<15} {ratio:.3e}  ({name})")
        assert ratio <= 1.0
