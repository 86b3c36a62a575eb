"""Element-wise parity of the stages in front of DAS (ingest, channel map, A1S2, Reshape, Decode, Filter / Demodulate, Hilbert): every
case pushes through the C ABI with the SCRATCH_POISON hook set (both intermediate buffers and the ring slot are 0xFF bytes --
NaN -- when the frame starts), reads back what the DAS stage read (beamformer_hip_copy_das_input) and compares it element by
element with the oracle's capture of the same buffer; then the frame with test_gpu_parity.compare.  A frame-level bar dilutes
a wrong sample by C x A before it sees it; these bars are per element.

Bars:
  * bit-identical (uint32 view) wherever the arithmetic is exact: ingest, channel map, A1S2, Reshape, int/f16 -> f32
    conversion, and Int16 RF decoded before any filter (integer partial sums below 2^24, one identical division);
  * elsewhere |gpu - oracle| <= bar, a forward-error bound propagated stage by stage in float64 from the stage's input
    magnitudes (stage_bounds below).  Each case prints its largest err / bar.  Every Filter / Demodulate stage takes its taps from
    its own filter slot (the oracle's plan names it); an Int16 store adds 1 in the stored unit (I16_STORE).
tests/pipeline_cases.py and tests/test_gpu_pipelines.py carry the same bars to the pipelines these cases never plan."""

import numpy as np
import pytest

from ogl_beamforming_amd import configs as cfg
from tests import cases
from tests.das_push import compare
from tests.stage_checks import (DECIMATION_CASES, DECODE_KINDS, DK, F16C_STAGES, FD, FS, KINDS, PITCH, S, as_bits, check_das_input, decimation_case,
                                decode_order_case, deepest_sample, float16_complex_case, oracle_run, plan_of, push, ragged_case, run_case)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ geometry


def test_decimation_matrix_covers_the_issue():
    covered = {(v[1], v[0]) for v in DECIMATION_CASES.values()}
    assert covered >= {(k, d) for k in KINDS for d in (2, 3, 4, 8)}
    assert {v[2] for v in DECIMATION_CASES.values()} >= {7, 36, 101}
    assert {v[3] for v in DECIMATION_CASES.values() if v[4]} >= {12, 16, 20}


@pytest.mark.parametrize("name", sorted(DECIMATION_CASES))
def test_decimation(name, bflib, oracle, hooks):
    D, kind, L, A, decode, chirp = DECIMATION_CASES[name]
    acq = decimation_case(D, kind, L, A, decode, seed=300 + sorted(DECIMATION_CASES).index(name), chirp=chirp)
    plan = plan_of(bflib, acq)
    Sd = int(plan.das_samples)
    assert Sd == acq.bp.sample_count // (2 * D)
    reach = deepest_sample(acq, plan)
    assert Sd // D <= reach < Sd - 2, f"the image reaches sample {reach:.1f}: not in the filter's tail [{Sd // D}, {Sd})"
    _, ref_in, _ = run_case(bflib, oracle, hooks, acq)
    assert not ref_in[:, :, Sd // D:].any(), "the oracle's tail is not zero"


# ------------------------------------------------------------------------------------------------ ragged rows


@pytest.mark.parametrize("demod", [True, False], ids=["demodulate", "decode"])
@pytest.mark.parametrize("S_", [130, 200, 1000, 1001])
def test_ragged_rows(S_, demod, bflib, oracle, hooks):
    """sample counts that are not a multiple of 128 (64 after demodulation): a ragged last 64-sample group in Filter and
    Decode, and with 1001 an odd row, whose half-element row start truncates (filter.glsl:81-87)"""
    acq = ragged_case(S_, demod, seed=400 + S_ + demod)
    run_case(bflib, oracle, hooks, acq, modes=(0,) if demod else (0, 0x20))


# ------------------------------------------------------------------------------------------------ decode orders


@pytest.mark.parametrize("kind", DECODE_KINDS, ids=[k.name for k in DECODE_KINDS])
@pytest.mark.parametrize("A", [2, 20, 24, 40, 128])
def test_decode_orders(A, kind, bflib, oracle, hooks):
    """FWHT base 20 (A = 20, 40), base 12 x 2 (24), the dense kernel's i0 + k < T guard (A = 2), 66 KiB of dynamic LDS (128
    complex) -- against the oracle, and the Walsh-Hadamard form against the forced-dense one (0x20)"""
    acq = decode_order_case(A, kind)
    _, ref_in, results = run_case(bflib, oracle, hooks, acq, modes=(0, 0x20))
    (fast_frame, fast_in, (bar_fast, _)), (dense_frame, dense_in, (bar_dense, _)) = results
    if kind == DK.Int16:
        assert bar_fast == bar_dense == "bit-identical"
        assert np.array_equal(as_bits(fast_in), as_bits(dense_in))
        assert np.array_equal(as_bits(fast_frame), as_bits(dense_frame))


# ------------------------------------------------------------------------------------------------ raw Float16Complex


@pytest.mark.parametrize("pipeline", sorted(F16C_STAGES))
def test_float16_complex_rf(pipeline, bflib, oracle, hooks):
    """raw Float16Complex RF: converted by a Reshape, decoded, or through a complex matched-chirp filter"""
    run_case(bflib, oracle, hooks, float16_complex_case(pipeline))


# ------------------------------------------------------------------------------------------------ every named case

@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_named_case_das_input_and_write_coverage(name, bflib, oracle, hooks):
    """the DAS input against the oracle (ingest with channel shuffle, raw padding and A1S2 included), and the poisoned frame
    bit-identical to an unpoisoned push: every voxel of the frame is written by some kernel"""
    acq = cases.make(name)
    poisoned = run_case(bflib, oracle, hooks, acq)[2][0][0]
    clean, _ = push(bflib, acq, hooks, poison=False)
    diff = as_bits(poisoned) != as_bits(clean)
    assert not diff.any(), f"{int(diff.sum())} frame scalars differ from the unpoisoned push (unwritten voxels keep 0xFFFFFFFF)"


# ------------------------------------------------------------------------------------------------ order independence

def test_decimation_tail_does_not_depend_on_earlier_frames(bflib, oracle, hooks):
    """without the hook: a D = 2 frame after a large-amplitude D = 1 frame of a bigger plan (both scratch buffers dirty) equals
    the same D = 2 frame pushed first after a fresh start, and the oracle"""
    hooks.clear("SCRATCH_POISON")
    acq = decimation_case(2, DK.Int16, 36, 16, True, seed=700)
    ref, flags, ref_in = oracle_run(oracle, acq)
    bflib.library().beamformer_hip_shutdown()
    first, first_in = push(bflib, acq)
    dirty = cfg.rca("dirty", 32, 16, 4096, (16, 1, 24), (-2e-3, 0, 5e-3), (2e-3, 0, 40e-3), seed=701, data_kind=DK.Float32,
                    stages=(S.Demodulate, S.Decode, S.DAS), decode=1, fs=FS, fd=FD, pitch=PITCH, angles=np.linspace(-5, 5, 16))
    dirty.rf = (dirty.rf * np.float32(1e6)).astype(np.float32)
    push(bflib, dirty)
    again, again_in = push(bflib, acq)
    check_das_input(bflib, oracle, acq, again_in, ref_in, "after a dirty frame")
    compare(again, ref, acq, flags)
    assert np.array_equal(as_bits(first_in), as_bits(again_in)), "the DAS input depends on what ran before it"
    assert np.array_equal(as_bits(first), as_bits(again)), "the frame depends on what ran before it"
