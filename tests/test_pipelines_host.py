"""The pipeline matrix of tests/pipeline_cases.py without a device: the extent audit (no stage in front of DAS writes past the
inter-stage buffer the executor allocates; the figures of the overrun this closed), what the matrix covers, how many random draws
are dropped, and the teeth of the error model (a stage that read the wrong filter slot does not pass under the bar)."""
import ctypes as C

import numpy as np
import pytest

from ogl_beamforming_amd import params as P
from tests import pipeline_cases as pc
from tests import stage_checks as stages

S = P.ShaderKind
DK = P.DataKind


def describe(bflib, acq):
    bflib.library().beamformer_reserve_parameter_blocks(1)
    return stages.plan_of(bflib, acq)


# ------------------------------------------------------------------------------------------------ the extent audit

@pytest.mark.parametrize("D, demodulate_writes, parent_buffer", [(1, 129024, 65536), (2, 128000, 32768)])
def test_scratch_holds_what_demodulate_writes_between_two_filters(D, demodulate_writes, parent_buffer, bflib):
    """Float32 {Demodulate, Filter, DAS}, 8 channels, 4 transmits, 512 samples: the Demodulate stage keeps the root's strides
    [1, S A, S] = [1, 2048, 512], now counted in complex elements, and writes up to byte (S / (2 D) - 1 + 2048 x 7 + 512 x 3 + 1) x 8.
    The parent commit allocated channels x transmits x das_samples x 8 bytes (+ 64) for it."""
    p = pc.BY_NAME["f32_demod_filter" if D == 1 else "f32_demod_filter_D2"]
    assert (p.kind, p.A, p.S, p.D) == (int(DK.Float32), 4, 512, D) and pc.CHANNELS == 8
    acq = pc.build(p)
    plan = describe(bflib, acq)
    extents, allocated = pc.audit(plan, acq.bp)
    assert [S(k).name for _, k, _ in extents] == ["Demodulate", "Filter"]
    assert extents[0][2] == demodulate_writes
    assert pc.CHANNELS * p.A * int(plan.das_samples) * 8 == parent_buffer < demodulate_writes <= allocated
    assert allocated <= pc.CHANNELS * p.A * p.S * 8, "the write extent of a stage in front of DAS is bounded by channels x transmits x S x 8"
    # (a burst's frames lie round_up(intermediate_bytes, 64) + 64 bytes apart in its stage buffers, csrc/executor.cpp; no describe call
    # reports that stride, so it is exercised on the device only: tests/test_gpu_pipelines.py test_long_chain_in_a_burst)


@pytest.mark.parametrize("name", sorted(pc.BY_NAME))
def test_audit_curated(name, bflib):
    acq = pc.build(pc.BY_NAME[name])
    extents, allocated = pc.audit(describe(bflib, acq), acq.bp)
    assert extents and max(e for _, _, e in extents) == allocated, "the buffers are as large as the largest write extent, no larger"


def test_audit_random_draws(bflib):
    for seed in pc.RANDOM_SEEDS:
        acq = pc.build(pc.draw_pipeline(seed))
        plan = P.HipPlan()
        L = bflib.library()
        L.beamformer_reserve_parameter_blocks(1)
        for slot, fp in enumerate(acq.filters):
            assert L.beamformer_create_filter(C.byref(fp), slot, 0)
        assert L.beamformer_push_simple_parameters(C.byref(acq.bp)), seed
        if L.beamformer_hip_describe_plan(0, C.byref(plan)):
            pc.audit(plan, acq.bp)


# ------------------------------------------------------------------------------------------------ the random draws

@pytest.fixture(scope="module")
def draws(bflib, oracle):
    return {seed: pc.kept(bflib, oracle, pc.draw_pipeline(seed)) for seed in pc.RANDOM_SEEDS}


@pytest.mark.parametrize("name", sorted(pc.BY_NAME))
def test_curated_pipeline_stands_above_its_bar(name, bflib, oracle):
    """more than half of the live DAS-input elements of the oracle exceed their bar: where the bar exceeds the signal, an all-zero
    DAS input would pass the element-wise check"""
    acq = pc.build(pc.BY_NAME[name])
    share = pc.signal_share(bflib, oracle, acq, stages.oracle_run(oracle, acq)[2])
    print(f"{name}: |oracle| > bar on {100 * share:.1f} % of the live DAS-input elements")
    assert share > pc.SIGNAL_SHARE


def test_few_random_draws_are_dropped(draws):
    dropped = {seed: why for seed, why in draws.items() if isinstance(why, str)}
    print(f"dropped {len(dropped)} of {len(draws)}: {dropped}")
    assert len(draws) == 96 and len(dropped) <= 12, dropped
    for seed, k in draws.items():
        if not isinstance(k, str):
            assert not np.isnan(k[3]).any() and not np.isnan(k[1]).all(), seed


# ------------------------------------------------------------------------------------------------ coverage

I16, I16C, F32, F32C, F16, F16C = "Int16", "Int16Complex", "Float32", "Float32Complex", "Float16", "Float16Complex"
ANY = None
# (stage, in kind, out kind, in layout, out layout, taps) with ANY as a wildcard: what the matrix must reach, by category
REQUIRED = {
    "Demodulate stores Int16Complex": ("Demodulate", I16C, I16C, ANY, ANY, ANY),
    "Filter stores Int16Complex": ("Filter", I16C, I16C, ANY, ANY, ANY),
    "Filter stores Int16": ("Filter", I16, I16, ANY, ANY, ANY),
    "Demodulate stores Float16Complex": ("Demodulate", F16C, F16C, ANY, ANY, ANY),
    "Filter stores Float16Complex": ("Filter", F16C, F16C, ANY, ANY, ANY),
    "Filter stores Float16": ("Filter", F16, F16, ANY, ANY, ANY),
    "Filter without demodulation on Int16": ("Filter", I16, F32, "das", "das", ANY),
    "Filter without demodulation on Int16Complex": ("Filter", I16C, F32C, "das", "das", ANY),
    "Filter without demodulation on Float32Complex": ("Filter", F32C, F32C, "das", "das", ANY),
    "Filter without demodulation on Float16": ("Filter", F16, F32, "das", "das", ANY),
    "complex chirp taps on real Float32 samples": ("Filter", F32, ANY, ANY, ANY, "complex"),
    "complex chirp taps on real Int16 samples": ("Filter", I16, ANY, ANY, ANY, "complex"),
    "complex chirp taps in a Demodulate": ("Demodulate", ANY, ANY, ANY, ANY, "complex"),
    "Filter feeding Decode, complex (the transposing form without demodulation)": ("Filter", F32C, F32C, "root", "decode", ANY),
    "Filter feeding Decode from Int16Complex": ("Filter", I16C, F16C, "root", "decode", ANY),
    "second Demodulate feeding Decode": ("Demodulate", F32C, F32C, "root", "decode", ANY),
    "second Demodulate feeding Decode, binary16": ("Demodulate", F16C, F16C, "root", "decode", ANY),
    "Filter feeding Decode, real Float32 (never transposes)": ("Filter", F32, F32, "decode", "decode", ANY),
    "Filter feeding Decode, real Int16": ("Filter", I16, I16, "decode", "decode", ANY),
    "Filter feeding Decode, real Float16": ("Filter", F16, F16, "decode", "decode", ANY),
    "Decode output stays in decode layout, Float32": ("Decode", F32, F32, "decode", "decode", ""),
    "Decode output stays in decode layout, Float32Complex": ("Decode", F32C, F32C, "decode", "decode", ""),
    "Decode output stays in decode layout, Float16": ("Decode", F16, F16, "decode", "decode", ""),
    "Decode Int16 -> Int16": ("Decode", I16, I16, "decode", "decode", ""),
    "Decode Float16Complex -> Float16Complex": ("Decode", F16C, F16C, "decode", "decode", ""),
    "Demodulate reading decode layout": ("Demodulate", F32C, F32C, "decode", "das", ANY),
    "Filter reading decode layout, complex": ("Filter", F32C, F32C, "decode", "decode", ANY),
    "Reshape Int16 -> Int16 into decode layout": ("Reshape", I16, I16, "das", "decode", ""),
    "Reshape Float16 -> Float16 into decode layout": ("Reshape", F16, F16, "das", "decode", ""),
    "Reshape Float32 -> Float32 into decode layout": ("Reshape", F32, F32, "das", "decode", ""),
    "Reshape Float16Complex -> Float16Complex into decode layout": ("Reshape", F16C, F16C, "das", "decode", ""),
    "Reshape Float32Complex -> Float32Complex into decode layout": ("Reshape", F32C, F32C, "das", "decode", ""),
    "Reshape of demodulated kinds from the root layout (reads past the RF)": ("Reshape", F32C, F32C, "root", "decode", ""),
}


def matches(sig, want):
    return all(w is ANY or w == s for s, w in zip(sig, want))


def test_pipeline_matrix_covers_the_issue(oracle, draws):
    """the signatures the curated list and the kept draws reach with the oracle's planner, against the written list"""
    reached, slot_values, lengths, transmits_into_decode = set(), set(), set(), set()
    curated = [(p, pc.build(p)) for p in pc.CURATED]
    random = [(pc.draw_pipeline(seed), k[0]) for seed, k in draws.items() if not isinstance(k, str)]
    curated_lengths = set()
    for index, (p, acq) in enumerate(curated + random):
        sigs, slots = pc.signatures(oracle, acq)
        reached.update(sigs)
        slot_values.update(slots)
        lengths.add(len(sigs))
        if index < len(curated):
            curated_lengths.add(len(sigs))
        for sig in sigs:
            if sig[0] in ("Filter", "Demodulate") and sig[4] == "decode" and sig[1].endswith("Complex"):
                transmits_into_decode.add(p.A)
    missing = [what for what, want in REQUIRED.items() if not any(matches(sig, want) for sig in reached)]
    assert not missing, missing
    assert slot_values >= set(pc.SLOT_VALUES), slot_values
    assert curated_lengths >= {1, 2, 3, 4, 5, 6}, curated_lengths
    assert 20 in transmits_into_decode, "A = 20: a ragged block of 16 transmits in the transposing filter"
    assert {p.A for p, _ in curated + random} >= set(pc.TRANSMITS) and {p.D for p, _ in curated + random} >= set(pc.DECIMATIONS)
    assert {p.S for p in pc.CURATED} >= {512, 1001} and sum(p.S == 1001 for p in pc.CURATED) == 2
    assert 35 <= len(pc.CURATED) <= 45
    named = named_case_signatures(oracle)
    print(f"{len(reached)} stage signatures, {len(reached - named)} of them beyond the named cases' {len(named)}")
    assert len(reached - named) >= 40


def named_case_signatures(oracle):
    from tests import cases
    out = set()
    for name in cases.CASES:
        acq = cases.make(name)
        filters = list(acq.filters) + [None] * (P.FILTER_SLOTS - len(acq.filters))
        acq.filters = [f if f is not None else acq.filters[0] if acq.filters else pc.filters()[0] for f in filters]
        out.update(pc.signatures(oracle, acq)[0])
    return out


# ------------------------------------------------------------------------------------------------ teeth

TWO_SLOTS = [p.name for p in pc.CURATED
             if len({s % P.FILTER_SLOTS for s, st in zip(p.slots, p.stages) if st in (int(S.Filter), int(S.Demodulate))}) >= 2]


@pytest.mark.parametrize("name", TWO_SLOTS)
def test_a_wrong_filter_slot_does_not_pass_under_the_bar(name, bflib, oracle):
    """the oracle's DAS input with the filters of the pipeline's first two distinct slots exchanged lies outside the element-wise
    bar on more than 1 % of the elements: a bar that a wrong slot passes under is not a bar"""
    p = pc.BY_NAME[name]
    used = []
    for s, st in zip(p.slots, p.stages):
        if st in (int(S.Filter), int(S.Demodulate)) and s % P.FILTER_SLOTS not in used:
            used.append(s % P.FILTER_SLOTS)
    acq = pc.build(p)
    exact, mag, bar = stages.stage_bounds(bflib, oracle, acq, describe(bflib, acq))
    assert not exact
    right = stages.oracle_run(oracle, acq)[2]
    wrong = stages.oracle_run(oracle, pc.build(p, swap=(used[0], used[1])))[2]
    if np.iscomplexobj(right):
        err = np.maximum(np.abs(right.real.astype(np.float64) - wrong.real), np.abs(right.imag.astype(np.float64) - wrong.imag))
    else:
        err = np.abs(right.astype(np.float64) - wrong)
    fraction = float(np.mean(err > bar))
    print(f"{name}: slots {used[0]} and {used[1]} exchanged: {100 * fraction:.1f} % of the DAS input outside the bar")
    assert fraction > 0.01
