"""DAS-only twins of the binary16-staged acquisitions.  DAS is a pure function of its arguments and of the bits of its
input, so an acquisition whose stages before DAS go through binary16 -- judged at 2e-3 of the frame maximum (tests/cases.py
tolerance()) -- has a twin that hands the DAS stage the same arguments and the same input with no stage in front of it: its RF IS the
DAS input, float32 or complex64, and tolerance() gives it 1e-4.  The library's frame of the twin must be its frame of the original,
bit for bit, and that frame is then judged against the oracle's frame of the twin by the unchanged compare().
A plain module: no pytest marker, no device, and the product library is not loaded by importing it."""
import ctypes as C

import numpy as np

from ogl_beamforming_amd import configs as cfg
from ogl_beamforming_amd import params as P
from tests import cases

# beamformer_hip_describe_das fields a twin must share with its original (tests/test_gpu_das_twins.py, tests/test_das_twins.py)
ROUTE_FIELDS = ("path", "tile_shift", "blocks", "split_shift", "tile_walk", "row_end_planes", "row_ends", "row_end_path", "u_axis", "u_shift",
                "v_shift", "window_samples", "uniform_tables", "lds_bytes", "threads", "channel_chunk", "hercules_prepared_copy",
                "tile_window_samples")
# plan fields a twin must share with its original: (the oracle's OraclePlan name, the library's HipPlan name or None)
PLAN_FIELDS = (("das_sampling_frequency", "das_sampling_frequency"), ("das_time_offset", "das_time_offset"), ("iq_pipeline", "iq_pipeline"),
               ("das_sparse", None), ("das_voxel_transform", "das_voxel_transform"), ("input_sample_count", "das_samples"))


def is_f16_staged(acq):
    """a stage before DAS goes through binary16: the pipeline's bar is 2e-3 (cases.tolerance)"""
    return cases.tolerance(acq) == 2e-3


def das_twin(acq, das_input, das_samples, das_sampling_frequency, das_time_offset):
    """The acquisition whose plan is the DAS stage alone, with acq's DAS arguments and `das_input` -- (channels, transmits, DAS samples),
    float32 or complex64: oracle.beamform(das_input=...)["data"] or lib.das_input() -- as its RF.  das_sampling_frequency and
    das_time_offset are the plan's float values (OraclePlan / HipPlan), passed through unchanged."""
    das_input = np.ascontiguousarray(das_input)
    channels, transmits = int(acq.bp.channel_count), int(acq.bp.acquisition_count)
    assert das_input.shape == (channels, transmits, int(das_samples)) and das_input.dtype in (np.float32, np.complex64)
    bp = P.SimpleParameters()
    C.memmove(C.byref(bp), C.byref(acq.bp), C.sizeof(bp))
    bp.sample_count = int(das_samples)
    bp.raw_data_dimensions[:] = [transmits * int(das_samples), channels]
    bp.sampling_frequency = das_sampling_frequency
    bp.time_offset = das_time_offset
    bp.decimation_rate = 1
    bp.decode_mode = 0
    bp.contrast_mode = 0
    for i in range(P.MAX_CHANNELS):
        bp.channel_mapping[i] = i
    for i in range(P.MAX_STAGES):
        bp.compute_stages[i] = 0
        bp.compute_stage_parameters[i] = 0
    bp.compute_stages[0], bp.compute_stages[1] = int(P.ShaderKind.Decode), int(P.ShaderKind.DAS)      # decode_mode 0 drops the Decode
    bp.compute_stages_count = 2
    bp.data_kind = int(P.DataKind.Float32Complex if np.iscomplexobj(das_input) else P.DataKind.Float32)
    return cfg.Acquisition(f"{acq.name}_das_twin", bp, [], das_input.reshape(channels, -1), [], acq.seed, "DAS-only twin")


def oracle_twin(oracle, acq):
    """(twin, the oracle's frame of acq, pairs, flags) with the twin built from the ORACLE's DAS-input capture and plan"""
    captured = {}
    flags = {} if acq.bp.interpolation_mode == int(P.InterpolationMode.Nearest) else None
    ref, pairs = oracle.beamform(acq.bp, acq.rf, acq.filters, flags=flags, das_input=captured)
    plan = oracle.plan(acq.bp, acq.filters)
    return das_twin(acq, captured["data"], plan.input_sample_count, plan.das_sampling_frequency, plan.das_time_offset), ref, pairs, flags


def route(description):
    """ROUTE_FIELDS of a HipDasDescription as a dict of plain values"""
    out = {}
    for name in ROUTE_FIELDS:
        v = getattr(description, name)
        out[name] = int(v) if isinstance(v, int) else [int(x) for x in v]
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)
