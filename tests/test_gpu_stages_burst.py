"""Element-wise parity of the stages in front of DAS inside a burst (beamformer_hip_push_data_burst_with_compute): every stage kernel
carries a frame dimension there -- ingest and Decode on grid z, Reshape on grid y, Filter and Hilbert on blockIdx.y = frame * channels +
channel with per-frame byte strides, in launches of 65535 // channels frames -- and tests/test_gpu_burst.py sees that code only through
the finished frame, which dilutes a wrong sample by channels x transmits.  Here what the DAS stage read for EVERY frame of the burst
(beamformer_hip_copy_das_input_frame) is judged, on the cases of tests/test_gpu_stages.py and tests/test_hilbert.py.

One burst of n = 5 independent noise frames with the SCRATCH_POISON hook set; for every frame k:
  1. no NaN in the DAS input;
  2. the DAS input equals, bit for bit, the DAS input of a single push of RF k: the kernels and the arithmetic are the same, only the
     frame offset differs;
  3. the DAS input meets tests/test_gpu_stages.py's element-wise bar against the oracle's capture for RF k (bit-identical where the
     arithmetic is exact, else inside the propagated forward-error bound -- nothing new);
  4. the frame meets compare() against the oracle; on the per-frame route (the single push's DAS kernel, free of floating-point
     atomics, on the same input bits) it is also bit-identical to the single push's frame, on the burst kernel within the tolerance
     tests/das_push.py's check_burst uses;
  5. the poisoned burst's frames equal an unpoisoned burst's, bit for bit.

The chunk boundary (tests/burst_chunk_cases.py): three bursts of 257 frames of 256 channels, built from four distinct RF frames, whose
frames 255 and 256 run in the stages' second launch.  Each case prints its largest err / bar as the single-push tests do."""
import dataclasses

import numpy as np
import pytest

from ogl_beamforming_amd import params as P
from tests import burst_chunk_cases, cases
from tests import stage_checks as stages
from tests.das_push import close_to_single_push, compare, noise_frames, same_bits
from tests.stage_checks import hilbert  # noqa: F401  (the fixture that enables the stage in the library and the oracle)
from tests.stage_checks import first_difference, nan_free, push_burst

pytestmark = pytest.mark.gpu

DK = P.DataKind
N = 5
as_bits = stages.as_bits


def burst_case(bflib, oracle, hooks, acq, modes=(0,), seed=0, each_reference=None):
    """one burst of N noise frames of acq's shape per DAS path mode, every frame judged by the five bars of the module docstring;
    each_reference(k, acq_k, ref_in): a check of the caller's on the oracle's capture of frame k.  Returns {mode: [DAS inputs]}."""
    rf = noise_frames(acq, N, 8000 + seed)
    of_frame = [dataclasses.replace(acq, rf=rf[k]) for k in range(N)]
    references = [stages.oracle_run(oracle, a) for a in of_frame]
    inputs_of = {}
    for mode in modes:
        frames, inputs, route = push_burst(bflib, hooks, acq, rf, mode)
        inputs_of[mode] = inputs
        clean = push_burst(bflib, hooks, acq, rf, mode, poison=False)[0]
        per_frame_route = not route.burst_kernel
        worst, bars = 0.0, set()
        for k in range(N):
            label = f"{acq.name} mode {mode:#x} burst frame {k}"
            nan_free(acq, inputs[k], label)
            one, one_in = stages.push(bflib, of_frame[k], hooks, poison=True, mode=mode)
            assert np.array_equal(as_bits(inputs[k]), as_bits(one_in)), \
                f"{label}: the DAS input is not the single push's bit for bit: {first_difference(inputs[k], one_in)}"
            ref, flags, ref_in = references[k]
            if each_reference:
                each_reference(k, of_frame[k], ref_in)
            bar, ratio = stages.check_das_input(bflib, oracle, of_frame[k], inputs[k], ref_in, label)
            bars.add(bar)
            worst = max(worst, ratio)
            compare(frames[k], ref, of_frame[k], flags, label=label)
            if per_frame_route:
                assert same_bits(frames[k], one), f"{label}: per-frame route, but the frame is not the single push's: {first_difference(frames[k], one)}"
            else:
                close_to_single_push(oracle, acq, rf[k], one, frames[k], k)
            assert same_bits(frames[k], clean[k]), (f"{label}: {first_difference(frames[k], clean[k])} from the unpoisoned burst "
                                                    f"(unwritten voxels keep 0xFFFFFFFF)")
        print(f"{acq.name} mode {mode:#x}: burst of {N} on the {'per-frame route' if per_frame_route else 'burst kernel'}, DAS inputs "
              f"{'/'.join(sorted(bars))}, equal to their single pushes bit for bit; burst max err/bar {worst:.3e}")
    return inputs_of


def test_a_single_push_and_a_views_push_hold_one_rf_frame(bflib, hooks):
    """beamformer_hip_copy_das_input_frame outside a burst: frame 0 is what beamformer_hip_copy_das_input serves, frame 1 is refused"""
    acq = stages.ragged_case(130, True, seed=530)
    _, newest = stages.push(bflib, acq, hooks, poison=True)
    views = [bflib.view_of(acq.bp), bflib.view_of(acq.bp)]
    for push in (None, lambda: bflib.beamform_views(acq.bp, acq.rf, views, acq.filters)):
        if push:
            push()
            assert np.array_equal(as_bits(bflib.das_input(acq.bp)), as_bits(newest))
        assert np.array_equal(as_bits(bflib.das_input(acq.bp, 0)), as_bits(newest))
        with pytest.raises(bflib.BeamformerError) as refused:
            bflib.das_input(acq.bp, 1)
        assert refused.value.kind == P.LibError.InvalidAccess


# ------------------------------------------------------------------------------------------------ decimation

@pytest.mark.parametrize("name", sorted(stages.DECIMATION_CASES))
def test_decimation(name, bflib, oracle, hooks):
    """the zero tail of a decimated row meets the neighbouring frame's data"""
    D, kind, L, A, decode, chirp = stages.DECIMATION_CASES[name]
    index = sorted(stages.DECIMATION_CASES).index(name)
    acq = stages.decimation_case(D, kind, L, A, decode, seed=300 + index, chirp=chirp)

    def reaches_the_tail(k, acq_k, ref_in):
        plan = stages.plan_of(bflib, acq_k)
        Sd = int(plan.das_samples)
        assert Sd == acq_k.bp.sample_count // (2 * D)
        reach = stages.deepest_sample(acq_k, plan)
        assert Sd // D <= reach < Sd - 2, f"frame {k}: the image reaches sample {reach:.1f}: not in the filter's tail [{Sd // D}, {Sd})"
        assert not ref_in[:, :, Sd // D:].any(), f"frame {k}: the oracle's tail is not zero"

    burst_case(bflib, oracle, hooks, acq, seed=index, each_reference=reaches_the_tail)


# ------------------------------------------------------------------------------------------------ ragged rows

@pytest.mark.parametrize("demod", [True, False], ids=["demodulate", "decode"])
@pytest.mark.parametrize("S_", [130, 1001])
def test_ragged_rows(S_, demod, bflib, oracle, hooks):
    acq = stages.ragged_case(S_, demod, seed=400 + S_ + demod)
    burst_case(bflib, oracle, hooks, acq, modes=(0,) if demod else (0, 0x20), seed=100 + S_ + demod)


# ------------------------------------------------------------------------------------------------ decode orders

@pytest.mark.parametrize("kind", stages.DECODE_KINDS, ids=[k.name for k in stages.DECODE_KINDS])
@pytest.mark.parametrize("A", [2, 20, 24, 128])
def test_decode_orders(A, kind, bflib, oracle, hooks):
    """FWHT bases 20 and 12 x 2, the dense kernel's guard (A = 2), 66 KiB of dynamic LDS (128 complex), and the forced dense form"""
    acq = stages.decode_order_case(A, kind)
    inputs_of = burst_case(bflib, oracle, hooks, acq, modes=(0, 0x20), seed=200 + A)
    if kind == DK.Int16:
        for k, (fast, dense) in enumerate(zip(inputs_of[0], inputs_of[0x20])):
            assert np.array_equal(as_bits(fast), as_bits(dense)), f"frame {k}: the Walsh-Hadamard and the dense decode differ"


# ------------------------------------------------------------------------------------------------ raw Float16Complex

@pytest.mark.parametrize("pipeline", sorted(stages.F16C_STAGES))
def test_float16_complex_rf(pipeline, bflib, oracle, hooks):
    burst_case(bflib, oracle, hooks, stages.float16_complex_case(pipeline), seed=300 + len(pipeline))


# ------------------------------------------------------------------------------------------------ Hilbert

@pytest.mark.parametrize("name", sorted(stages.acquisitions()) + [f"ragged_{n}" for n in stages.RAGGED_SAMPLES])
def test_hilbert_stage(name, bflib, oracle, hooks, hilbert):  # noqa: F811
    acq = stages.ragged_acquisition(int(name[7:])) if name.startswith("ragged_") else stages.acquisitions()[name]
    burst_case(bflib, oracle, hooks, acq, seed=400 + len(name))


# ------------------------------------------------------------------------------------------------ named cases

# ingest with work to do in a burst (channel shuffle and raw padding, A1S2, complex Int16), and the remaining stage forms
NAMED = ["rca_shuffled_padded", "rca_a1s2", "rca_i16_complex_in",
         "config5_literal_order", "hercules_wide_cw", "hercules_chirp", "forces_filter_f32", "hercules_demod_decode_cw"]


@pytest.mark.parametrize("name", NAMED)
def test_named_case(name, bflib, oracle, hooks):
    burst_case(bflib, oracle, hooks, cases.make(name), seed=500 + NAMED.index(name))


# ------------------------------------------------------------------------------------------------ the chunk boundary

@pytest.mark.parametrize("name", sorted(burst_chunk_cases.CASES))
def test_chunk_boundary(name, bflib, oracle, hooks, request):
    """257 frames of 256 channels: frames 255 and 256 run in the second launch of every filter-shaped stage, on in + in_frame_bytes * 255"""
    if name in burst_chunk_cases.NEEDS_HILBERT:
        request.getfixturevalue("hilbert")
    bc = burst_chunk_cases
    acq = bc.CASES[name]()
    assert acq.bp.channel_count == bc.CHANNELS and tuple(acq.bp.output_points[:3]) == bc.POINTS
    sources = noise_frames(acq, bc.SOURCES, 9300 + sorted(bc.CASES).index(name))
    source_of = bc.assignment(9400 + sorted(bc.CASES).index(name))
    rf = np.ascontiguousarray(sources[source_of])
    assert rf.shape[0] == bc.FRAMES and rf.nbytes <= 70e6

    frames, inputs, route = push_burst(bflib, hooks, acq, rf, 0)
    assert route.stage_launches == 2, "the burst did not cross a chunk of the stages' launches"

    of_source = [dataclasses.replace(acq, rf=sources[j]) for j in range(bc.SOURCES)]
    worst = 0.0
    for j in range(bc.SOURCES):
        label = f"{acq.name} source {j}"
        one, one_in = stages.push(bflib, of_source[j], hooks, poison=True)
        nan_free(acq, one_in, label)
        mine = np.flatnonzero(source_of == j)
        for k in mine:
            assert np.array_equal(as_bits(inputs[k]), as_bits(one_in)), \
                (f"{acq.name}: the DAS input of frame {k} (launch {k // bc.CHUNK}) is not the single push's of its RF (source {j}) bit for "
                 f"bit: {first_difference(inputs[k], one_in)}")
            assert same_bits(frames[k], frames[mine[0]]), f"{acq.name}: frames {mine[0]} and {k} hold the same RF and differ"
        ref, flags, ref_in = stages.oracle_run(oracle, of_source[j])
        worst = max(worst, stages.check_das_input(bflib, oracle, of_source[j], one_in, ref_in, label)[1])
        compare(frames[mine[-1]], ref, of_source[j], flags, label=f"{label} frame {mine[-1]}")
    print(f"{acq.name}: {bc.FRAMES} frames in {route.stage_launches} stage launches on the "
          f"{'burst kernel' if route.burst_kernel else 'per-frame route'}: every DAS input equals its single push bit for bit; max err/bar {worst:.3e}")
