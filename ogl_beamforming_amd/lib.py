"""ctypes binding of libogl_beamformer_lib.so.

This is the stub a maintainer of the reference would keep: the reference exposes its client
library to Python through cffi over a preprocessed header (build.c:4798-4800); the function
names, argument order and return conventions below are those of
lib/ogl_beamformer_lib_base.h.  The library is the MI355X build in this repository; there
is no CPU fallback -- loading fails loudly when the .so is missing, and compute calls fail
with LibError.SharedMemory when no HIP device is present.
"""
import ctypes as C
import os

import numpy as np

from . import params as P

_HERE = os.path.dirname(os.path.abspath(__file__))
# OGL_BEAMFORMER_LIB points at another build of the same library (kernel experiments)
LIBRARY_PATH = os.environ.get("OGL_BEAMFORMER_LIB") or os.path.join(_HERE, "libogl_beamformer_lib.so")


class BeamformerError(RuntimeError):
    def __init__(self, kind, message):
        super().__init__(f"{P.LibError(kind).name}: {message}")
        self.kind = P.LibError(kind)


def _share_torch_hip_runtime():
    """One HIP runtime per process.  The PyTorch-ROCm wheel ships its own libamdhip64.so.7
    beside libtorch; the dynamic loader keys on the SONAME, so whichever copy is mapped first
    serves both.  The system copy first and torch's HSA runtime second leaves torch without a
    device ("No HIP GPUs are available"), so when torch is installed its copy is mapped before
    the library, without importing torch.  C and MATLAB clients never see this: they link
    the ROCm installation's runtime (csrc/Makefile rpath)."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return                                  # already mapped by torch itself
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    path = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(path):
        try:
            C.CDLL(path, mode=C.RTLD_GLOBAL)
        except OSError:
            pass                                # the ROCm installation's runtime serves alone


def _load():
    if not os.path.exists(LIBRARY_PATH):
        raise ImportError(
            f"{LIBRARY_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU implementation to fall back to.")
    _share_torch_hip_runtime()
    lib = C.CDLL(LIBRARY_PATH)
    u32, i32, u64, vp = C.c_uint32, C.c_int32, C.c_uint64, C.c_void_p
    sig = {
        "beamformer_get_api_version": (u32, []),
        "beamformer_get_last_error": (i32, []),
        "beamformer_get_last_error_string": (C.c_char_p, []),
        "beamformer_error_string": (C.c_char_p, [i32]),
        "beamformer_maximum_frames_for_parameters": (u64, [C.POINTER(P.Parameters)]),
        "beamformer_maximum_frames_for_simple_parameters": (u64, [C.POINTER(P.SimpleParameters)]),
        "beamformer_maximum_rf_data_size": (u64, []),
        "beamformer_beamform_data": (u32, [C.POINTER(P.SimpleParameters), vp, u32, vp, i32]),
        "beamformer_set_global_timeout": (None, [u32]),
        "beamformer_push_data_with_compute": (u32, [vp, u32, u32, u32]),
        "beamformer_get_last_frames": (u32, [vp, u64, u32]),
        "beamformer_reserve_parameter_blocks": (u32, [u32]),
        "beamformer_set_pipeline_stage_parameters": (u32, [u32, i32]),
        "beamformer_set_pipeline_stage_parameters_at": (u32, [u32, i32, u32]),
        "beamformer_push_pipeline": (u32, [C.POINTER(i32), u32, i32]),
        "beamformer_push_pipeline_at": (u32, [C.POINTER(i32), u32, i32, u32]),
        "beamformer_push_simple_parameters": (u32, [C.POINTER(P.SimpleParameters)]),
        "beamformer_push_simple_parameters_at": (u32, [C.POINTER(P.SimpleParameters), u32]),
        "beamformer_push_parameters": (u32, [C.POINTER(P.Parameters)]),
        "beamformer_push_parameters_at": (u32, [C.POINTER(P.Parameters), u32]),
        "beamformer_push_channel_mapping": (u32, [C.POINTER(C.c_int16), u32]),
        "beamformer_push_channel_mapping_at": (u32, [C.POINTER(C.c_int16), u32, u32]),
        "beamformer_push_sparse_elements": (u32, [C.POINTER(C.c_int16), u32]),
        "beamformer_push_sparse_elements_at": (u32, [C.POINTER(C.c_int16), u32, u32]),
        "beamformer_push_focal_vectors": (u32, [C.POINTER(C.c_float), u32]),
        "beamformer_push_focal_vectors_at": (u32, [C.POINTER(C.c_float), u32, u32]),
        "beamformer_push_transmit_receive_orientations": (u32, [C.POINTER(C.c_uint8), u32]),
        "beamformer_push_transmit_receive_orientations_at": (u32, [C.POINTER(C.c_uint8), u32, u32]),
        "beamformer_create_filter": (u32, [C.POINTER(P.FilterParameters), C.c_uint8, C.c_uint8]),
        "beamformer_live_parameters_get_dirty_flag": (i32, []),
        "beamformer_set_live_parameters": (u32, [C.POINTER(P.LiveImagingParameters)]),
        "beamformer_get_live_parameters": (C.POINTER(P.LiveImagingParameters), []),
        "beamformer_compute_timings": (u32, [C.POINTER(P.ComputeStatsTable), i32]),
        # MI355X extensions (include/ogl_beamformer_hip.h)
        "beamformer_hip_set_device": (u32, [i32]),
        "beamformer_hip_get_device": (i32, []),
        "beamformer_hip_set_devices": (u32, [C.POINTER(i32), u32]),
        "beamformer_hip_get_device_count": (u32, []),
        "beamformer_hip_get_device_frame_timings": (u32, [u32, C.POINTER(P.HipFrameTimings)]),
        "beamformer_hip_get_device_info": (u32, [u32, C.POINTER(P.HipDeviceInfo)]),
        "beamformer_hip_set_stream": (u32, [vp]),
        "beamformer_hip_set_output_shard": (u32, [u32, u32, u32]),
        "beamformer_hip_push_device_data_with_compute": (u32, [vp, u32, u32, u32]),
        "beamformer_hip_push_data_burst_with_compute": (u32, [vp, u32, u32, u32, u32]),
        "beamformer_hip_push_device_data_burst_with_compute": (u32, [vp, u32, u32, u32, u32]),
        "beamformer_hip_describe_burst": (u32, [u32, u32, C.POINTER(P.HipBurstDescription)]),
        "beamformer_hip_get_last_burst_info": (u32, [C.POINTER(P.HipBurstInfo)]),
        "beamformer_hip_push_data_readi_sweep_with_compute": (u32, [vp, u32, u32, C.POINTER(u32), u32, u32]),
        "beamformer_hip_push_device_data_readi_sweep_with_compute": (u32, [vp, u32, u32, C.POINTER(u32), u32, u32]),
        "beamformer_hip_describe_readi_sweep": (u32, [u32, C.POINTER(u32), u32, C.POINTER(P.HipBurstDescription)]),
        "beamformer_hip_resolve_readi_groups": (u32, [u32, C.POINTER(u32), u32, C.POINTER(u32)]),
        "beamformer_hip_push_data_readi_image_with_compute": (u32, [vp, u32, u32, C.POINTER(u32), u32, u32]),
        "beamformer_hip_push_device_data_readi_image_with_compute": (u32, [vp, u32, u32, C.POINTER(u32), u32, u32]),
        "beamformer_hip_describe_readi_image": (u32, [u32, C.POINTER(u32), u32, C.POINTER(P.HipReadiImageDescription)]),
        "beamformer_hip_get_last_readi_image_info": (u32, [C.POINTER(P.HipReadiImageInfo)]),
        "beamformer_hip_push_data_views_with_compute": (u32, [vp, u32, C.POINTER(P.HipView), u32, u32]),
        "beamformer_hip_push_device_data_views_with_compute": (u32, [vp, u32, C.POINTER(P.HipView), u32, u32]),
        "beamformer_hip_describe_views": (u32, [u32, C.POINTER(P.HipView), u32, C.POINTER(P.HipViewsDescription)]),
        "beamformer_hip_get_last_views_info": (u32, [C.POINTER(P.HipViewsInfo)]),
        "beamformer_hip_push_data_burst_views_with_compute": (u32, [vp, u32, u32, C.POINTER(P.HipView), u32, u32]),
        "beamformer_hip_push_device_data_burst_views_with_compute": (u32, [vp, u32, u32, C.POINTER(P.HipView), u32, u32]),
        "beamformer_hip_describe_burst_views": (u32, [u32, u32, C.POINTER(P.HipView), u32, C.POINTER(P.HipBurstViewsDescription)]),
        "beamformer_hip_get_last_burst_views_info": (u32, [C.POINTER(P.HipBurstViewsInfo)]),
        "beamformer_hip_push_data_variants_with_compute": (u32, [vp, u32, C.POINTER(P.HipDasVariant), u32, u32, u32]),
        "beamformer_hip_push_device_data_variants_with_compute": (u32, [vp, u32, C.POINTER(P.HipDasVariant), u32, u32, u32]),
        "beamformer_hip_describe_variants": (u32, [u32, C.POINTER(P.HipDasVariant), u32, C.POINTER(P.HipVariantsDescription)]),
        "beamformer_hip_get_last_variants_info": (u32, [C.POINTER(P.HipVariantsInfo)]),
        "beamformer_hip_score_last_frames": (u32, [u32, C.POINTER(P.HipFrameRegion), C.POINTER(P.HipFrameMetrics), C.POINTER(C.c_float)]),
        "beamformer_hip_copy_frame": (u32, [u32, vp, u64]),
        "beamformer_hip_get_frame_info": (u32, [u32, C.POINTER(P.HipFrameInfo)]),
        "beamformer_hip_rank_frames": (u32, [C.POINTER(P.HipFrameMetrics), u32, u32, C.POINTER(C.c_double), C.POINTER(u32)]),
        "beamformer_hip_find_peaks_last_frames": (u32, [u32, C.POINTER(P.HipFrameRegion), C.POINTER(C.c_float), u32, u32, C.POINTER(P.HipFramePeaks),
                                                        C.POINTER(P.HipFramePeak), C.POINTER(u32), C.POINTER(C.c_float)]),
        "beamformer_hip_peaks_to_views": (u32, [C.POINTER(C.c_float), C.POINTER(u32), C.POINTER(P.HipFramePeak), u32, C.POINTER(u32),
                                                C.POINTER(C.c_float), u32, u32, C.POINTER(P.HipView)]),
        "beamformer_hip_quantiles_last_frames": (u32, [u32, C.POINTER(P.HipFrameRegion), C.POINTER(C.c_double), u32, C.POINTER(P.HipFrameQuantiles),
                                                       C.POINTER(P.HipFrameQuantile), C.POINTER(u32), C.POINTER(C.c_float)]),
        "beamformer_hip_peak_threshold_of": (u32, [C.c_float, u32, C.POINTER(C.c_float)]),
        "beamformer_hip_localisation_map_reset": (u32, [C.POINTER(u32)]),
        "beamformer_hip_accumulate_peaks_last_frames": (u32, [u32, C.POINTER(P.HipFrameRegion), C.POINTER(C.c_float), u32, C.POINTER(C.c_double), u32, u32,
                                                              C.POINTER(P.HipMapDeposits), C.POINTER(C.c_float)]),
        "beamformer_hip_localisation_map_copy": (u32, [C.POINTER(u32), u64, C.POINTER(P.HipMapInfo)]),
        "beamformer_hip_queue_localisation_map": (u32, [C.c_float, u32, C.POINTER(u32), C.POINTER(C.c_float)]),
        "beamformer_hip_map_placement": (u32, [C.POINTER(C.c_float), C.POINTER(u32), C.POINTER(C.c_float), C.POINTER(u32), C.POINTER(C.c_double)]),
        "beamformer_hip_track_map_reset": (u32, [C.POINTER(u32)]),
        "beamformer_hip_pair_peaks_last_frames": (u32, [u32, C.POINTER(P.HipFrameRegion), C.POINTER(C.c_float), u32, C.POINTER(C.c_double), u32, u32,
                                                        C.c_float, u32, u32, C.POINTER(P.HipPeakPairs), C.POINTER(P.HipPeakPair), C.POINTER(u32),
                                                        C.POINTER(C.c_float)]),
        "beamformer_hip_track_peaks_last_frames": (u32, [u32, C.POINTER(P.HipFrameRegion), C.POINTER(C.c_float), u32, C.POINTER(C.c_double), u32, u32,
                                                         C.c_float, u32, u32, u32, C.POINTER(P.HipTrackedFrame), C.POINTER(P.HipPeakTrack),
                                                         C.POINTER(P.HipTrackPoint), C.POINTER(u32), C.POINTER(u32), C.POINTER(C.c_float)]),
        "beamformer_hip_draw_tracks_last_frames": (u32, [u32, C.POINTER(P.HipFrameRegion), C.POINTER(C.c_float), u32, C.POINTER(C.c_double), u32, u32,
                                                         C.c_float, u32, u32, u32, u32, C.POINTER(P.HipDrawnFrame), C.POINTER(C.c_float)]),
        "beamformer_hip_track_map_copy": (u32, [C.POINTER(u32), C.POINTER(C.c_int64), u64, C.POINTER(P.HipTrackMapInfo)]),
        "beamformer_hip_queue_track_map": (u32, [u32, C.c_float, u32, u32, C.POINTER(u32), C.POINTER(C.c_float)]),
        "beamformer_hip_gram_last_frames": (u32, [u32, C.POINTER(P.HipFrameRegion), C.POINTER(C.c_double), C.POINTER(P.HipEnsembleInfo), C.POINTER(C.c_float)]),
        "beamformer_hip_clutter_projector": (u32, [C.POINTER(C.c_double), u32, u32, u32, C.POINTER(C.c_float), C.POINTER(C.c_double)]),
        "beamformer_hip_mix_last_frames": (u32, [u32, C.POINTER(C.c_float), u32, u32, C.POINTER(u32), C.POINTER(C.c_float)]),
        "beamformer_hip_gram_boxes_last_frames": (u32, [u32, C.POINTER(P.HipFrameRegion), u32, C.POINTER(C.c_double), C.POINTER(P.HipEnsembleInfo),
                                                        C.POINTER(C.c_float)]),
        "beamformer_hip_lattice_boxes": (u32, [C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), C.POINTER(P.HipFrameRegion)]),
        "beamformer_hip_mix_field_last_frames": (u32, [u32, C.POINTER(C.c_float), C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), u32, u32,
                                                       C.POINTER(u32), C.POINTER(C.c_float)]),
        "beamformer_hip_autocorrelate_last_frames": (u32, [u32, C.POINTER(C.c_float), u32, u32, u32, C.POINTER(u32), C.POINTER(C.c_float)]),
        "beamformer_hip_convolve_last_frames": (u32, [u32, C.POINTER(C.POINTER(C.c_float)), C.POINTER(u32), u32, u32, C.POINTER(u32), C.POINTER(C.c_float)]),
        "beamformer_hip_correlate_last_frames": (u32, [u32, u32, C.POINTER(P.HipFrameRegion), u32, C.POINTER(u32), C.POINTER(P.HipShiftCorrelation),
                                                       C.POINTER(P.HipCorrelationInfo), C.POINTER(C.c_float)]),
        "beamformer_hip_displacements_from_correlation": (u32, [C.POINTER(P.HipShiftCorrelation), u32, C.POINTER(u32), u32, C.POINTER(P.HipDisplacement)]),
        "beamformer_hip_warp_last_frames": (u32, [u32, C.POINTER(C.c_float), C.POINTER(u32), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                                  C.POINTER(C.c_float), u32, u32, u32, C.POINTER(u32), C.POINTER(C.c_float)]),
        "beamformer_hip_synchronize": (u32, []),
        "beamformer_hip_get_last_frame_info": (u32, [C.POINTER(P.HipFrameInfo)]),
        "beamformer_hip_get_last_frame_timings": (u32, [C.POINTER(P.HipFrameTimings)]),
        "beamformer_hip_enable_frame_graphs": (u32, [u32]),
        "beamformer_hip_frame_graph_counts": (u32, [C.POINTER(u64), C.POINTER(u64)]),
        "beamformer_hip_enable_pair_counting": (u32, [u32]),
        "beamformer_hip_frame_min_max": (u32, [C.POINTER(C.c_float)]),
        "beamformer_hip_sum_last_frames": (u32, [u32, vp, u64]),
        "beamformer_hip_copy_das_input": (u32, [vp, u64]),
        "beamformer_hip_copy_das_input_frame": (u32, [u32, vp, u64]),
        "beamformer_hip_display_last_frame": (u32, [C.c_float, C.c_float, C.c_float, C.POINTER(C.c_float), u64]),
        "beamformer_hip_enable_hilbert": (u32, [u32]),
        "beamformer_hip_set_das_path": (u32, [u32]),
        "beamformer_hip_zbp_parameters": (u32, [vp, u64, C.POINTER(P.SimpleParameters), C.POINTER(P.HipZbpPayload)]),
        "beamformer_hip_zbp_load": (u32, [C.c_char_p, u32, C.POINTER(P.SimpleParameters), C.POINTER(vp), C.POINTER(u64)]),
        "beamformer_hip_zbp_free": (None, [vp]),
        "beamformer_hip_zbp_last_error": (C.c_char_p, []),
        "beamformer_hip_host_das_transform": (None, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(i32), C.POINTER(C.c_float)]),
        "beamformer_hip_host_hadamard": (u32, [u32, C.POINTER(C.c_float)]),
        "beamformer_hip_host_filter": (i32, [C.POINTER(P.FilterParameters), C.POINTER(C.c_float), u32,
                                        C.POINTER(C.c_float), C.POINTER(u32)]),
        "beamformer_hip_describe_plan": (u32, [u32, C.POINTER(P.HipPlan)]),
        "beamformer_hip_describe_das": (u32, [u32, C.POINTER(P.HipDasDescription)]),
        "beamformer_hip_describe_upload": (u32, [u32, u32, u32, vp, C.POINTER(P.HipUploadDescription)]),
        "beamformer_hip_set_hook": (u32, [C.c_char_p, C.c_char_p]),
        "beamformer_hip_shutdown": (None, []),
    }
    for name, (restype, argtypes) in sig.items():
        fn = getattr(lib, name)          # AttributeError: the library must export every symbol
        fn.restype = restype
        fn.argtypes = argtypes
    lib._signatures = sig
    return lib


_lib = None


def library():
    global _lib
    if _lib is None:
        _lib = _load()
    return _lib


def exported_symbols():
    """Names the headers under include/ declare (kept in step by tests/test_abi.py)."""
    return sorted(library()._signatures)


def last_error():
    lib = library()
    return P.LibError(lib.beamformer_get_last_error()), lib.beamformer_get_last_error_string().decode()


def _check(result):
    if not result:
        kind, message = last_error()
        raise BeamformerError(kind, message)
    return result


def frame_shape(bp):
    pts = [max(1, int(v)) for v in bp.output_points[:3]]
    return (pts[2], pts[1], pts[0])      # z slowest, x fastest (das.glsl:132-136)


def output_is_complex(bp):
    stages = list(bp.compute_stages[: bp.compute_stages_count])
    return int(P.ShaderKind.Demodulate) in stages or P.DATA_KIND_COMPLEX[int(bp.data_kind)]


def _prepared(bp, filters, timeout_ms):
    """The library with the filters, the parameters (block 0) and the timeout of a beamform*() call in place."""
    lib = library()
    for slot, fp in enumerate(filters):
        if fp is not None:
            _check(lib.beamformer_create_filter(C.byref(fp), slot, 0))
    _check(lib.beamformer_push_simple_parameters(C.byref(bp)))
    lib.beamformer_set_global_timeout(C.c_uint32(timeout_ms & 0xFFFFFFFF).value)
    return lib


def _described(bp, filters, slot):
    """The library with the filters and the parameters (block `slot`) of a describe_*() call in place."""
    L = library()
    for i, fp in enumerate(filters):
        assert L.beamformer_create_filter(C.byref(fp), i, slot), last_error()
    assert L.beamformer_push_simple_parameters_at(C.byref(bp), slot), last_error()
    return L


def _push(kind, rf, on_device_pointer, frame_size, *arguments):
    """beamformer_hip_push_data_<kind>_with_compute on the host array `rf`, or -- `on_device_pointer` given -- its device-resident twin
    on that address; `arguments`: what both take after the frame size."""
    lib = library()
    if on_device_pointer is not None:
        call, data = getattr(lib, f"beamformer_hip_push_device_data_{kind}_with_compute"), C.c_void_p(on_device_pointer)
    else:
        call, data = getattr(lib, f"beamformer_hip_push_data_{kind}_with_compute"), rf.ctypes.data_as(C.c_void_p)
    _check(call(data, frame_size, *arguments))


def beamform(bp, rf, filters=(), timeout_ms=-1):
    """One frame through the C ABI exactly as tests/throughput.c drives the reference:
    create_filter* -> push_simple_parameters -> push_data_with_compute -> get_last_frames.
    `rf` is a C-contiguous numpy array holding raw_data_dimensions[1] rows.  Returns the frame
    as float32 or complex64 with shape (Z, Y, X)."""
    lib = _prepared(bp, filters, timeout_ms)
    rf = np.ascontiguousarray(rf)
    _check(lib.beamformer_push_data_with_compute(rf.ctypes.data_as(C.c_void_p), rf.nbytes, 0, 0))
    return get_last_frame(bp)


def get_last_frames(bp, count, shard_planes=None):
    """The `count` newest frames, oldest first, as one array (count, Z, Y, X); all of this block's size and kind."""
    lib = library()
    shape = list(frame_shape(bp))
    if shard_planes is not None:
        shape[0] = shard_planes
    info = P.HipFrameInfo()
    _check(lib.beamformer_hip_get_last_frame_info(C.byref(info)))
    complex_out = info.data_kind == int(P.DataKind.Float32Complex)
    voxels = int(np.prod(shape))
    each = (voxels * (8 if complex_out else 4) + 63) // 64 * 64          # frames are exported rounded up to 64 bytes
    raw = np.zeros(count * each // 4, dtype=np.float32)
    _check(lib.beamformer_get_last_frames(raw.ctypes.data_as(C.c_void_p), raw.nbytes, count))
    frames = raw.reshape(count, each // 4)
    if complex_out:
        return np.ascontiguousarray(frames[:, : 2 * voxels]).view(np.complex64).reshape([count] + shape)
    return np.ascontiguousarray(frames[:, :voxels]).reshape([count] + shape)


def beamform_burst(bp, rf_frames, filters=(), timeout_ms=-1, on_device_pointer=None):
    """N frames of one geometry in one call (beamformer_hip_push_data_burst_with_compute): `rf_frames` is a C-contiguous array
    whose first axis runs over the frames, each frame laid out as beamform() takes it.  Returns (N, Z, Y, X), oldest first."""
    _prepared(bp, filters, timeout_ms)
    rf_frames = np.ascontiguousarray(rf_frames)
    count = rf_frames.shape[0]
    frame_size = rf_frames.nbytes // count
    _push("burst", rf_frames, on_device_pointer, frame_size, count, 0, 0)
    return get_last_frames(bp, count)


def describe_burst(bp, n, filters=(), slot=0):
    """What a burst of n frames of these parameters would run (beamformer_hip_describe_burst): the description struct; .reason
    says why.  Needs no device."""
    L = _described(bp, filters, slot)
    d = P.HipBurstDescription()
    _check(L.beamformer_hip_describe_burst(slot, n, C.byref(d)))
    return d


def last_burst_info():
    """beamformer_hip_get_last_burst_info: the newest burst's route, ids and whole-burst stage times; waits for it."""
    info = P.HipBurstInfo()
    _check(library().beamformer_hip_get_last_burst_info(C.byref(info)))
    return info


def _group_array(groups):
    """A READI sweep's group list as the C ABI takes it: None -> NULL."""
    if groups is None:
        return None
    groups = [int(g) for g in groups]
    return (C.c_uint32 * len(groups))(*groups)


def beamform_readi_sweep(bp, rf_frames, groups=None, filters=(), timeout_ms=-1, on_device_pointer=None):
    """The group acquisitions of a READI sequence in one call (beamformer_hip_push_data_readi_sweep_with_compute): `rf_frames` as
    beamform_burst() takes it, frame k beamformed with readi_group = groups[k]; groups None: (bp.readi_group + k) % readi_group_count.
    Returns (N, Z, Y, X), oldest first."""
    _prepared(bp, filters, timeout_ms)
    rf_frames = np.ascontiguousarray(rf_frames)
    count = rf_frames.shape[0]
    assert groups is None or len(groups) == count
    frame_size = rf_frames.nbytes // count
    _push("readi_sweep", rf_frames, on_device_pointer, frame_size, count, _group_array(groups), 0, 0)
    return get_last_frames(bp, count)


def describe_readi_sweep(bp, n, groups=None, filters=(), slot=0):
    """What a READI sweep of n frames of these parameters would run (beamformer_hip_describe_readi_sweep): the description struct;
    .reason says why.  Needs no device."""
    L = _described(bp, filters, slot)
    d = P.HipBurstDescription()
    _check(L.beamformer_hip_describe_readi_sweep(slot, _group_array(groups), n, C.byref(d)))
    return d


def resolve_readi_groups(bp, n, groups=None, slot=0):
    """The group of every frame of such a sweep, as the push resolves the list (beamformer_hip_resolve_readi_groups).  Needs no device."""
    L = library()
    assert L.beamformer_push_simple_parameters_at(C.byref(bp), slot), last_error()
    out = (C.c_uint32 * n)()
    _check(L.beamformer_hip_resolve_readi_groups(slot, _group_array(groups), n, out))
    return list(out)


def beamform_readi_image(bp, rf_frames, groups=None, filters=(), timeout_ms=-1, on_device_pointer=None):
    """The group acquisitions of a READI sequence compounded into ONE frame (beamformer_hip_push_data_readi_image_with_compute):
    `rf_frames` and `groups` as beamform_readi_sweep() takes them.  Returns the image, (Z, Y, X): the derived FORCES block's frame of
    the DAS input decoded across the acquisitions -- without coherency weighting the sum of the sweep's frames."""
    _prepared(bp, filters, timeout_ms)
    rf_frames = np.ascontiguousarray(rf_frames)
    count = rf_frames.shape[0]
    assert groups is None or len(groups) == count
    frame_size = rf_frames.nbytes // count
    _push("readi_image", rf_frames, on_device_pointer, frame_size, count, _group_array(groups), 0, 0)
    return get_last_frame(bp)


def describe_readi_image(bp, n, groups=None, filters=(), slot=0):
    """What a READI image push of n RF frames of these parameters would run (beamformer_hip_describe_readi_image): the description
    struct; .reason says what.  Needs no device."""
    L = _described(bp, filters, slot)
    d = P.HipReadiImageDescription()
    _check(L.beamformer_hip_describe_readi_image(slot, _group_array(groups), n, C.byref(d)))
    return d


def last_readi_image_info():
    """beamformer_hip_get_last_readi_image_info: the newest image push's route, id and whole-push stage times; waits for it."""
    info = P.HipReadiImageInfo()
    _check(library().beamformer_hip_get_last_readi_image_info(C.byref(info)))
    return info


def view(points, lo, hi, plane=None, plane_offset=0.0, tag=0):
    """A HipView of `points` voxels spanning lo .. hi: the grid configs' acquisitions are built on (configs._voxel_transform: a volume
    when it has z planes, else a view plane with depth on image y -- plane "yz" for the YZ plane)."""
    from . import configs
    v = P.HipView()
    v.das_voxel_transform[:] = [float(x) for x in configs._voxel_transform(points, lo, hi, plane, plane_offset)]
    v.output_points[:] = [max(1, int(n)) for n in points]
    v.image_plane_tag = int(tag)
    return v


def view_of(bp, tag=0):
    """The HipView of a parameter struct's own grid."""
    v = P.HipView()
    v.das_voxel_transform[:] = list(bp.das_voxel_transform)
    v.output_points[:] = [max(1, int(n)) for n in bp.output_points[:3]]
    v.image_plane_tag = int(tag)
    return v


def _view_array(views):
    views = list(views)
    return (P.HipView * len(views))(*views), len(views)


def get_last_views(views):
    """The frames of the newest views push of these views, oldest first: a list of arrays (Z, Y, X), each of its view's size."""
    lib = library()
    info = P.HipFrameInfo()
    _check(lib.beamformer_hip_get_last_frame_info(C.byref(info)))
    complex_out = info.data_kind == int(P.DataKind.Float32Complex)
    shapes = [(int(v.output_points[2]), int(v.output_points[1]), int(v.output_points[0])) for v in views]
    sizes = [(int(np.prod(sh)) * (8 if complex_out else 4) + 63) // 64 * 64 for sh in shapes]     # each exported rounded up to 64 bytes
    raw = np.zeros(sum(sizes) // 4, dtype=np.float32)
    _check(lib.beamformer_get_last_frames(raw.ctypes.data_as(C.c_void_p), raw.nbytes, len(shapes)))
    out, at = [], 0
    for sh, size in zip(shapes, sizes):
        voxels = int(np.prod(sh))
        if complex_out:
            out.append(raw[at // 4: at // 4 + 2 * voxels].view(np.complex64).reshape(sh).copy())
        else:
            out.append(raw[at // 4: at // 4 + voxels].reshape(sh).copy())
        at += size
    return out


def beamform_views(bp, rf, views, filters=(), timeout_ms=-1, on_device_pointer=None):
    """ONE RF frame on K grids in one call (beamformer_hip_push_data_views_with_compute): everything but the grid from `bp`, view k on
    views[k] (HipView: see view()).  `rf` as beamform() takes it.  Returns a list of K arrays (Z, Y, X), in view order."""
    _prepared(bp, filters, timeout_ms)
    rf = np.ascontiguousarray(rf)
    array, count = _view_array(views)
    _push("views", rf, on_device_pointer, rf.nbytes, array, count, 0)
    return get_last_views(views)


def describe_views(bp, views, filters=(), slot=0):
    """What a views push of these grids would run (beamformer_hip_describe_views): the description struct; .path[k] is view k's own
    single-frame decision, .reason says why this route.  Needs no device."""
    L = _described(bp, filters, slot)
    array, count = _view_array(views)
    d = P.HipViewsDescription()
    _check(L.beamformer_hip_describe_views(slot, array, count, C.byref(d)))
    return d


def last_views_info():
    """beamformer_hip_get_last_views_info: the newest views push's route, ids and whole-push stage times; waits for it."""
    info = P.HipViewsInfo()
    _check(library().beamformer_hip_get_last_views_info(C.byref(info)))
    return info


def variant(speed_of_sound, time_offset, f_number):
    """A HipDasVariant: the three DAS scalars of one candidate of a variants push."""
    return P.HipDasVariant(float(speed_of_sound), float(time_offset), float(f_number))


def variant_of(bp, **changes):
    """The HipDasVariant of a parameter struct's own values, with `changes` (speed_of_sound=, time_offset=, f_number=) applied."""
    values = {"speed_of_sound": bp.speed_of_sound, "time_offset": bp.time_offset, "f_number": bp.f_number}
    values.update(changes)
    return variant(**values)


def with_variant(bp, v):
    """A copy of the parameter struct carrying the variant's three values: the block whose single push frame k of a variants push is."""
    out = type(bp).from_buffer_copy(bp)
    out.speed_of_sound, out.time_offset, out.f_number = v.speed_of_sound, v.time_offset, v.f_number
    return out


def _variant_array(variants):
    variants = list(variants)
    return (P.HipDasVariant * len(variants))(*variants), len(variants)


def beamform_variants(bp, rf, variants, filters=(), timeout_ms=-1, on_device_pointer=None):
    """ONE RF frame under K sets of DAS scalars in one call (beamformer_hip_push_data_variants_with_compute): everything but speed of
    sound, time offset and f-number from `bp`, frame k under variants[k] (HipDasVariant: see variant()).  `rf` as beamform() takes it.
    Returns (K, Z, Y, X), variant 0 first."""
    _prepared(bp, filters, timeout_ms)
    rf = np.ascontiguousarray(rf)
    array, count = _variant_array(variants)
    _push("variants", rf, on_device_pointer, rf.nbytes, array, count, 0, 0)
    return get_last_frames(bp, count)


def describe_variants(bp, variants, filters=(), slot=0):
    """What a variants push of these candidates would run (beamformer_hip_describe_variants): the description struct; .path[k] is
    variant k's own single-frame decision, .taken[k] whether the fused launch takes it, .reason says why this route.  Needs no device."""
    L = _described(bp, filters, slot)
    array, count = _variant_array(variants)
    d = P.HipVariantsDescription()
    _check(L.beamformer_hip_describe_variants(slot, array, count, C.byref(d)))
    return d


def last_variants_info():
    """beamformer_hip_get_last_variants_info: the newest variants push's route, ids and whole-push stage times; waits for it."""
    info = P.HipVariantsInfo()
    _check(library().beamformer_hip_get_last_variants_info(C.byref(info)))
    return info


def frame_region(first, count):
    """A HipFrameRegion: the box of voxels first .. first + count (x, y, z)."""
    return P.HipFrameRegion((C.c_uint32 * 3)(*[int(v) for v in first]), (C.c_uint32 * 3)(*[int(v) for v in count]))


def score_last_frames(count, region=None):
    """beamformer_hip_score_last_frames: the `count` newest frames reduced on the device to one HipFrameMetrics row each, oldest first;
    region (HipFrameRegion: see frame_region()) None: every frame whole.  Returns (rows, device_ms): a ctypes array of `count` rows and
    the device time of the reduction."""
    rows = (P.HipFrameMetrics * max(1, int(count)))()
    ms = C.c_float(0)
    _check(library().beamformer_hip_score_last_frames(count, None if region is None else C.byref(region), rows, C.byref(ms)))
    return rows, float(ms.value)


def rank_frames(rows, criterion):
    """beamformer_hip_rank_frames (host only): (scores, best) -- the criterion (P.FrameScore) of every row as a float64 array, and the
    index of the highest, the lowest index among ties.  Raises when no row has a score."""
    rows = list(rows)
    array = (P.HipFrameMetrics * max(1, len(rows)))(*rows)
    scores = np.zeros(max(1, len(rows)), np.float64)
    best = C.c_uint32(0)
    _check(library().beamformer_hip_rank_frames(array, len(rows), int(criterion), scores.ctypes.data_as(C.POINTER(C.c_double)), C.byref(best)))
    return scores[:len(rows)], int(best.value)


_NO_PLACEMENTS = object()


def _peak_arguments(count, thresholds, region, placements=_NO_PLACEMENTS):
    """What the peak calls take first, as ctypes: [count, region, thresholds, their number] and -- for a call that has placements --
    [placements, their number], ready to be passed on.  Raises ValueError for placements that are not 12 numbers a matrix."""
    values = [float(t) for t in np.atleast_1d(np.asarray(thresholds, np.float32))]
    head = [int(count), None if region is None else C.byref(region), (C.c_float * max(1, len(values)))(*values), len(values)]
    if placements is not _NO_PLACEMENTS:
        matrices = np.ascontiguousarray(np.asarray(placements, np.float64).reshape(-1))
        if matrices.size % 12:
            raise ValueError("placements: 12 numbers (row-major 3 x 4) a matrix")
        head += [matrices.ctypes.data_as(C.POINTER(C.c_double)), matrices.size // 12]
    return head


def _first_records(kind, records, total):
    """the first `total` of the packed records a call wrote into a numpy array of `kind`, as a ctypes array of their own"""
    return (kind * total).from_buffer_copy(records[:total].tobytes())


def find_peaks_last_frames(count, thresholds, max_per_frame, region=None):
    """beamformer_hip_find_peaks_last_frames: the local maxima of the `count` newest frames, found on the device.  thresholds: one number
    for all frames, or `count` of them, oldest first (on the magnitude, in the frame's units); region None: every frame whole.  Returns
    (frames, peaks, device_ms): a ctypes array of `count` HipFramePeaks rows, a ctypes array of the packed HipFramePeak records (frame
    n's are peaks[frames[n].first : frames[n].first + frames[n].stored]) and the device time of the launches."""
    count, max_per_frame = int(count), int(max_per_frame)
    head = _peak_arguments(count, thresholds, region)
    rows = (P.HipFramePeaks * max(1, count))()
    room = count * max_per_frame if 0 < count <= P.HIP_MAX_SCORED_FRAMES and 0 < max_per_frame <= P.HIP_MAX_PEAKS_PER_FRAME else 0
    records = np.zeros(max(1, room), np.dtype(P.HipFramePeak))
    total, ms = C.c_uint32(0), C.c_float(0)
    _check(library().beamformer_hip_find_peaks_last_frames(*head, max_per_frame, rows, records.ctypes.data_as(C.POINTER(P.HipFramePeak)),
                                                           C.byref(total), C.byref(ms)))
    return rows, _first_records(P.HipFramePeak, records, int(total.value)), float(ms.value)


def peaks_to_views(source_transform, source_points, peaks, patch_points, patch_extent_voxels, use_offsets=True, tag=0):
    """beamformer_hip_peaks_to_views (host only): one HipView a peak -- a patch of patch_points voxels spanning patch_extent_voxels voxels
    of the source grid (its das_voxel_transform and points) around the peak, at its sub-voxel offsets when use_offsets.  A list."""
    peaks = list(peaks)
    array = (P.HipFramePeak * max(1, len(peaks)))(*peaks)
    out = (P.HipView * max(1, len(peaks)))()
    _check(library().beamformer_hip_peaks_to_views((C.c_float * 16)(*[float(v) for v in source_transform]),
                                                   (C.c_uint32 * 3)(*[int(v) for v in source_points]), array, len(peaks),
                                                   (C.c_uint32 * 3)(*[int(v) for v in patch_points]),
                                                   (C.c_float * 3)(*[float(v) for v in patch_extent_voxels]), 1 if use_offsets else 0, int(tag), out))
    return list(out[: len(peaks)])


def quantiles_last_frames(count, fractions, region=None, histograms=False):
    """beamformer_hip_quantiles_last_frames: exact order statistics of the `count` newest frames, selected on the device.  fractions: up
    to HIP_MAX_QUANTILES numbers in [0, 1], in any order; region None: every frame whole.  Returns (frames, quantiles, histograms,
    device_ms): a ctypes array of `count` HipFrameQuantiles rows, a ctypes array of count * len(fractions) HipFrameQuantile records
    (frame n's are quantiles[frames[n].first : frames[n].first + frames[n].stored], in the order of `fractions`), the coarse histograms
    as a uint32 array (count, HIP_QUANTILE_BINS) -- None unless asked for -- and the device time of the launches."""
    count = int(count)
    values = np.ascontiguousarray(np.atleast_1d(np.asarray(fractions, np.float64)))
    rows = (P.HipFrameQuantiles * max(1, count))()
    records = (P.HipFrameQuantile * max(1, count * len(values)))()
    tables = np.zeros((max(1, count), P.HIP_QUANTILE_BINS), np.uint32) if histograms else None
    ms = C.c_float(0)
    _check(library().beamformer_hip_quantiles_last_frames(count, None if region is None else C.byref(region),
                                                          values.ctypes.data_as(C.POINTER(C.c_double)), len(values), rows, records,
                                                          None if tables is None else tables.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(ms)))
    return rows, records, tables, float(ms.value)


def peak_threshold_of(decision_value, data_kind):
    """beamformer_hip_peak_threshold_of (host only): the threshold of the peak calls for a quantile's `value` -- the value itself for
    P.DataKind.Float32, the largest float32 T with fl(T * T) <= value for P.DataKind.Float32Complex."""
    out = C.c_float(0)
    _check(library().beamformer_hip_peak_threshold_of(float(decision_value), int(data_kind), C.byref(out)))
    return float(out.value)


_map_points = None      # the grid of the newest localisation_map_reset(): what localisation_map_copy() sizes its array by


def localisation_map_reset(points):
    """beamformer_hip_localisation_map_reset: (re)allocates the library's one localisation map of points = (x, y, z) uint32 counts and
    zeroes it; points None releases it."""
    global _map_points
    _check(library().beamformer_hip_localisation_map_reset(None if points is None else (C.c_uint32 * 3)(*[int(v) & 0xFFFFFFFF for v in points])))
    _map_points = None if points is None else tuple(int(v) for v in points)


def accumulate_peaks_last_frames(count, thresholds, placements, use_offsets=True, region=None):
    """beamformer_hip_accumulate_peaks_last_frames: the peaks of the `count` newest frames (find_peaks_last_frames' peaks, no cap)
    deposited on the device into the localisation map.  thresholds and region as find_peaks_last_frames takes them; placements: one
    3 x 4 float64 matrix for all frames, or `count` of them, oldest first (any shape of 12 or count x 12 numbers; map_placement makes
    one): a peak at index + offset lands on map coordinate A[:, :3] @ p + A[:, 3] and in the bin floor(. + 0.5).  Returns
    (frames, device_ms): a ctypes array of `count` HipMapDeposits rows and the device time of the launches."""
    count = int(count)
    head = _peak_arguments(count, thresholds, region, placements)
    rows = (P.HipMapDeposits * max(1, count))()
    ms = C.c_float(0)
    _check(library().beamformer_hip_accumulate_peaks_last_frames(*head, 1 if use_offsets else 0, rows, C.byref(ms)))
    return rows, float(ms.value)


def localisation_map_copy(points=None):
    """beamformer_hip_localisation_map_copy: (counts, info) -- the map as a uint32 array (Z, Y, X) and its HipMapInfo (the grid, and the
    calls and deposits since the reset).  points: the map's grid (x, y, z), which sizes the array; None: the grid the newest
    localisation_map_reset() of this module asked for."""
    points = _map_points if points is None else tuple(int(v) for v in points)
    if points is None:
        raise ValueError("points: no localisation_map_reset() through this module yet")
    out = np.zeros(max(1, int(np.prod(points))), np.uint32)
    info = P.HipMapInfo()
    _check(library().beamformer_hip_localisation_map_copy(out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size, C.byref(info)))
    shape = (int(info.points[2]), int(info.points[1]), int(info.points[0]))
    return out[: int(np.prod(shape))].reshape(shape), info


def queue_localisation_map(scale=1.0, tag=0, timed=True):
    """beamformer_hip_queue_localisation_map: the map's counts times `scale` queued into the frame ring as one Float32 frame of the
    map's grid; the map itself is left as it is.  Returns (frame_id, device_ms); timed False: the call does not synchronise and
    device_ms is 0."""
    frame, ms = C.c_uint32(0), C.c_float(0)
    _check(library().beamformer_hip_queue_localisation_map(float(scale), int(tag), C.byref(frame), C.byref(ms) if timed else None))
    return int(frame.value), float(ms.value)


def map_placement(frame_transform, frame_points, map_transform, map_points):
    """beamformer_hip_map_placement (host only): the float64 (3, 4) placement that takes a voxel position of the frame's grid (its
    das_voxel_transform and points) to the map coordinate of the same point in space, for accumulate_peaks_last_frames."""
    out = np.zeros(12, np.float64)
    _check(library().beamformer_hip_map_placement((C.c_float * 16)(*[float(v) for v in frame_transform]),
                                                  (C.c_uint32 * 3)(*[int(v) for v in frame_points]),
                                                  (C.c_float * 16)(*[float(v) for v in map_transform]),
                                                  (C.c_uint32 * 3)(*[int(v) for v in map_points]), out.ctypes.data_as(C.POINTER(C.c_double))))
    return out.reshape(3, 4)


_track_points = None    # the grid of the newest track_map_reset(): what track_map_copy() sizes its arrays by


def track_map_reset(points):
    """beamformer_hip_track_map_reset: (re)allocates the library's one track map of points = (x, y, z) voxels -- a uint32 count and three
    int64 displacement sums each -- and zeroes it; points None releases it."""
    global _track_points
    _check(library().beamformer_hip_track_map_reset(None if points is None else (C.c_uint32 * 3)(*[int(v) & 0xFFFFFFFF for v in points])))
    _track_points = None if points is None else tuple(int(v) for v in points)


def pair_peaks_last_frames(count, thresholds, placements, max_distance, max_per_frame, use_offsets=True, deposit=False, region=None,
                           records=True):
    """beamformer_hip_pair_peaks_last_frames: the peaks of the `count` newest frames (find_peaks_last_frames' records at the same
    thresholds, region and max_per_frame) linked frame to frame on the device: a peak a of frame n and a peak b of frame n + 1 are a
    pair when each is the other's nearest within max_distance (in map coordinates, under the frames' placements: one 3 x 4 float64
    matrix for all frames or `count` of them, as accumulate_peaks_last_frames takes them).  deposit: the pairs' midpoints and
    displacements go into the track map (track_map_reset).  Returns (rows, pairs, device_ms): a ctypes array of count - 1 HipPeakPairs
    rows, a ctypes array of the packed HipPeakPair records (frame pair n's are pairs[rows[n].first : rows[n].first + rows[n].pairs];
    empty with records False: the call makes none) and the device time of the launches."""
    count, max_per_frame = int(count), int(max_per_frame)
    head = _peak_arguments(count, thresholds, region, placements)
    rows = (P.HipPeakPairs * max(1, count - 1))()
    room = (count - 1) * max_per_frame if records and 2 <= count <= P.HIP_MAX_SCORED_FRAMES and 0 < max_per_frame <= P.HIP_MAX_PEAKS_PER_FRAME else 0
    out = np.zeros(max(1, room), np.dtype(P.HipPeakPair))
    total, ms = C.c_uint32(0), C.c_float(0)
    _check(library().beamformer_hip_pair_peaks_last_frames(*head, 1 if use_offsets else 0, float(max_distance), max_per_frame, 1 if deposit else 0,
                                                           rows, out.ctypes.data_as(C.POINTER(P.HipPeakPair)) if records else None, C.byref(total),
                                                           C.byref(ms)))
    return rows, _first_records(P.HipPeakPair, out, int(total.value) if records else 0), float(ms.value)


def track_peaks_last_frames(count, thresholds, placements, max_distance, max_per_frame, min_length, use_offsets=True, deposit=0, region=None,
                            records=True):
    """beamformer_hip_track_peaks_last_frames: the pairs of pair_peaks_last_frames (same arguments up to max_per_frame) chained over the
    `count` newest frames into tracks -- a head, its links toward newer frames, no gap closing --, of which those of at least
    min_length peaks are kept, listed in ascending (start frame, head's rank) and deposited: deposit is 0 or any of
    P.HIP_TRACK_DEPOSIT_POINTS (the kept tracks' peaks into the localisation map) and P.HIP_TRACK_DEPOSIT_LINKS (their pairs into the
    track map).  Returns (rows, tracks, points, device_ms): a ctypes array of `count` HipTrackedFrame rows, ctypes arrays of the
    HipPeakTrack and the HipTrackPoint records (track t's points are points[tracks[t].first : tracks[t].first + tracks[t].length];
    both empty with records False: the call downloads none) and the device time of the launches."""
    count, max_per_frame = int(count), int(max_per_frame)
    head = _peak_arguments(count, thresholds, region, placements)
    rows = (P.HipTrackedFrame * max(1, count))()
    room = count * max_per_frame if records and 2 <= count <= P.HIP_MAX_SCORED_FRAMES and 0 < max_per_frame <= P.HIP_MAX_PEAKS_PER_FRAME else 0
    out_tracks, out_points = np.zeros(max(1, room), np.dtype(P.HipPeakTrack)), np.zeros(max(1, room), np.dtype(P.HipTrackPoint))
    track_total, point_total, ms = C.c_uint32(0), C.c_uint32(0), C.c_float(0)
    _check(library().beamformer_hip_track_peaks_last_frames(*head, 1 if use_offsets else 0, float(max_distance), max_per_frame, int(min_length),
                                                            int(deposit), rows,
                                                            out_tracks.ctypes.data_as(C.POINTER(P.HipPeakTrack)) if records else None,
                                                            out_points.ctypes.data_as(C.POINTER(P.HipTrackPoint)) if records else None,
                                                            C.byref(track_total), C.byref(point_total), C.byref(ms)))
    kept_tracks, kept_points = (int(track_total.value), int(point_total.value)) if records else (0, 0)
    return rows, _first_records(P.HipPeakTrack, out_tracks, kept_tracks), _first_records(P.HipTrackPoint, out_points, kept_points), float(ms.value)


def draw_tracks_last_frames(count, thresholds, placements, max_distance, max_per_frame, min_length, smooth=0, use_offsets=True, deposit=0,
                            region=None):
    """beamformer_hip_draw_tracks_last_frames: the kept tracks of track_peaks_last_frames (same arguments up to min_length) smoothed by
    a moving average of half-width `smooth` (0 .. P.HIP_MAX_TRACK_SMOOTH, clipped at each track's ends) and drawn at map resolution:
    every link is sampled once a map cell of its extent, and each drawn sample goes into the localisation map
    (P.HIP_TRACK_DEPOSIT_POINTS) and, with the link's displacement, into the track map (P.HIP_TRACK_DEPOSIT_LINKS).  No record list
    comes back.  Returns (rows, device_ms): a ctypes array of `count` HipDrawnFrame rows and the device time of the launches."""
    count, max_per_frame = int(count), int(max_per_frame)
    head = _peak_arguments(count, thresholds, region, placements)
    rows = (P.HipDrawnFrame * max(1, count))()
    ms = C.c_float(0)
    _check(library().beamformer_hip_draw_tracks_last_frames(*head, 1 if use_offsets else 0, float(max_distance), max_per_frame, int(min_length),
                                                            int(smooth), int(deposit), rows, C.byref(ms)))
    return rows, float(ms.value)


def track_map_copy(points=None):
    """beamformer_hip_track_map_copy: (counts, sums, info) -- the track map's counts as a uint32 array (Z, Y, X), its displacement sums
    as an int64 array (3, Z, Y, X) in units of 2^-20 map voxels (component r along map axis r) and its HipTrackMapInfo.  points: the
    map's grid (x, y, z), which sizes the arrays; None: the grid the newest track_map_reset() of this module asked for."""
    points = _track_points if points is None else tuple(int(v) for v in points)
    if points is None:
        raise ValueError("points: no track_map_reset() through this module yet")
    voxels = max(1, int(np.prod(points)))
    counts, sums = np.zeros(voxels, np.uint32), np.zeros(3 * voxels, np.int64)
    info = P.HipTrackMapInfo()
    _check(library().beamformer_hip_track_map_copy(counts.ctypes.data_as(C.POINTER(C.c_uint32)), sums.ctypes.data_as(C.POINTER(C.c_int64)),
                                                   counts.size, C.byref(info)))
    shape = (int(info.points[2]), int(info.points[1]), int(info.points[0]))
    n = int(np.prod(shape))
    return counts[:n].reshape(shape), sums[:3 * n].reshape((3,) + shape), info


def queue_track_map(component, scale=1.0, min_pairs=1, tag=0, timed=True):
    """beamformer_hip_queue_track_map: one component of the track map queued into the frame ring as one Float32 frame of the map's grid
    -- 0..2: the mean displacement along map axis x, y, z per frame interval; 3: the pair count; 4: the squared mean speed --, times
    `scale`, 0 where fewer than max(1, min_pairs) pairs were deposited.  Returns (frame_id, device_ms); timed False: the call does not
    synchronise and device_ms is 0."""
    frame, ms = C.c_uint32(0), C.c_float(0)
    _check(library().beamformer_hip_queue_track_map(int(component), float(scale), int(min_pairs), int(tag), C.byref(frame),
                                                    C.byref(ms) if timed else None))
    return int(frame.value), float(ms.value)


def gram_last_frames(count, region=None):
    """beamformer_hip_gram_last_frames: the slow-time Gram matrix of the `count` newest frames (one grid, one kind), reduced on the
    device over the voxels of the box that are finite in every frame; region None: the frames whole.  Returns (gram, info, device_ms):
    a complex128 (count, count) array -- gram[j, k] = sum of conj(f_j) f_k, index 0 the oldest frame --, the HipEnsembleInfo and the
    device time of the launches."""
    count = int(count)
    room = count if 0 < count <= P.HIP_MAX_ENSEMBLE_FRAMES else 1
    gram = np.zeros((room, room), np.complex128)
    info, ms = P.HipEnsembleInfo(), C.c_float(0)
    _check(library().beamformer_hip_gram_last_frames(count, None if region is None else C.byref(region), gram.ctypes.data_as(C.POINTER(C.c_double)),
                                                     C.byref(info), C.byref(ms)))
    return gram, info, float(ms.value)


def clutter_projector(gram, remove_high, remove_low=0):
    """beamformer_hip_clutter_projector (host only): the projector that drops the remove_high strongest and the remove_low weakest
    slow-time components of the Hermitian `gram` (its upper triangle is read).  Returns (weights, eigenvalues): a complex64 (K, K)
    array for mix_last_frames and the K eigenvalues in descending order."""
    gram = np.ascontiguousarray(gram, np.complex128)
    count = int(gram.shape[0]) if gram.ndim == 2 and gram.shape[0] == gram.shape[1] else 0
    room = max(1, count)
    weights, values = np.zeros((room, room), np.complex64), np.zeros(room, np.float64)
    _check(library().beamformer_hip_clutter_projector(gram.ctypes.data_as(C.POINTER(C.c_double)), count, int(remove_high), int(remove_low),
                                                      weights.ctypes.data_as(C.POINTER(C.c_float)), values.ctypes.data_as(C.POINTER(C.c_double))))
    return weights, values


def mix_last_frames(count, weights, tag=0, timed=True):
    """beamformer_hip_mix_last_frames: weights.shape[0] new frames of the frame ring, frame j = sum over k of weights[j, k] times the
    k-th oldest of the `count` newest frames; weights: (out_count, count), complex (real frames: real, or complex with zero imaginary
    parts).  Returns (first_frame_id, device_ms); timed False: the call does not synchronise and device_ms is 0."""
    count = int(count)
    weights = np.ascontiguousarray(np.atleast_2d(np.asarray(weights)), np.complex64)
    out_count = int(weights.shape[0])
    if weights.shape[1] != count:
        raise ValueError(f"weights {weights.shape}: the second dimension is not count = {count}")
    first, ms = C.c_uint32(0), C.c_float(0)
    _check(library().beamformer_hip_mix_last_frames(count, weights.ctypes.data_as(C.POINTER(C.c_float)), out_count, int(tag), C.byref(first),
                                                    C.byref(ms) if timed else None))
    return int(first.value), float(ms.value)


def gram_boxes_last_frames(count, regions):
    """beamformer_hip_gram_boxes_last_frames: the slow-time Gram matrix of the `count` newest frames over each box of `regions` (a
    sequence of HipFrameRegion: see frame_region() and lattice_boxes()), each byte for byte what gram_last_frames gives for that box, in
    one call that synchronises once.  Returns (grams, infos, device_ms): a complex128 (B, count, count) array, the B HipEnsembleInfo
    and the device time of the launches."""
    count = int(count)
    boxes = list(regions)
    B = len(boxes)
    room = (B, count, count) if 0 < B <= P.HIP_MAX_GRAM_BOXES and 0 < count <= P.HIP_MAX_ENSEMBLE_FRAMES and \
        B * count * count <= P.HIP_MAX_GRAM_BOX_ENTRIES else (1, 1, 1)       # the call refuses before it writes: room for nothing
    grams = np.zeros(room, np.complex128)
    array = (P.HipFrameRegion * max(1, B))(*boxes)
    infos, ms = (P.HipEnsembleInfo * room[0])(), C.c_float(0)
    _check(library().beamformer_hip_gram_boxes_last_frames(count, array, B, grams.ctypes.data_as(C.POINTER(C.c_double)), infos, C.byref(ms)))
    return grams, list(infos), float(ms.value)


def _three(values, what):
    values = [int(v) for v in values]
    if len(values) != 3:
        raise ValueError(what + ": one number per axis, x, y, z")
    return (C.c_uint32 * 3)(*[v & 0xFFFFFFFF for v in values]), values


def lattice_boxes(points, nodes, node_first, node_step, half):
    """beamformer_hip_lattice_boxes (host only): the boxes of a lattice of nodes = (x, y, z) nodes an axis on a grid of `points`, node j
    of axis a at voxel node_first[a] + j * node_step[a], each box reaching `half[a]` voxels to either side of its node and clipped to the
    frame.  Returns a list of HipFrameRegion in flat node order, (jz * Ny + jy) * Nx + jx: what gram_boxes_last_frames takes, and the
    order of the nodes of mix_field_last_frames' weights."""
    arrays = [_three(v, what) for v, what in ((points, "points"), (nodes, "nodes"), (node_first, "node_first"), (node_step, "node_step"), (half, "half"))]
    N = arrays[1][1]
    product = N[0] * N[1] * N[2]
    regions = (P.HipFrameRegion * (product if 0 < product <= P.HIP_MAX_MIX_NODES else 1))()
    _check(library().beamformer_hip_lattice_boxes(*[a for a, _ in arrays], regions))
    return list(regions)


def mix_field_last_frames(count, weights, node_first, node_step, tag=0, timed=True):
    """beamformer_hip_mix_field_last_frames: weights.shape[3] new frames of the frame ring, a mix of the `count` newest frames whose
    weight table varies over the frame.  weights: complex (Nz, Ny, Nx, M, count) -- the table mix_last_frames would take, one at each
    node of a lattice, node j of axis a at voxel node_first[a] + j * node_step[a] (x, y, z).  Between two nodes the nodes' outputs are
    blended linearly, outside the lattice the nearest node's table holds; a lattice of one node is mix_last_frames.  Returns
    (first_frame_id, device_ms); timed False: the call does not synchronise and device_ms is 0."""
    count = int(count)
    weights = np.ascontiguousarray(np.asarray(weights), np.complex64)
    if weights.ndim != 5 or weights.shape[4] != count:
        raise ValueError(f"weights {weights.shape}: not (Nz, Ny, Nx, M, count = {count})")
    nodes, _ = _three(weights.shape[2::-1], "nodes")
    first, ms = C.c_uint32(0), C.c_float(0)
    _check(library().beamformer_hip_mix_field_last_frames(count, weights.ctypes.data_as(C.POINTER(C.c_float)), nodes, _three(node_first, "node_first")[0],
                                                          _three(node_step, "node_step")[0], int(weights.shape[3]), int(tag), C.byref(first),
                                                          C.byref(ms) if timed else None))
    return int(first.value), float(ms.value)


def autocorrelate_last_frames(count, weights=None, lags=2, tag=0, timed=True):
    """beamformer_hip_autocorrelate_last_frames: `lags` new frames of the frame ring, frame L = sum over n of conj(y_n) y_(n+L) per
    voxel, y_n = sum over k of weights[n, k] times the k-th oldest of the `count` newest frames -- bit for bit the frames
    mix_last_frames would store, which are never written; weights: (rows, count) as for mix_last_frames, or None: y_n is the n-th
    frame itself.  Returns (first_frame_id, device_ms): the id of lag 0; timed False: the call does not synchronise and device_ms is 0."""
    count = int(count)
    pointer, rows = None, count
    if weights is not None:
        weights = np.ascontiguousarray(np.atleast_2d(np.asarray(weights)), np.complex64)
        if weights.shape[1] != count:
            raise ValueError(f"weights {weights.shape}: the second dimension is not count = {count}")
        pointer, rows = weights.ctypes.data_as(C.POINTER(C.c_float)), int(weights.shape[0])
    first, ms = C.c_uint32(0), C.c_float(0)
    _check(library().beamformer_hip_autocorrelate_last_frames(count, pointer, rows, int(lags), int(tag), C.byref(first),
                                                              C.byref(ms) if timed else None))
    return int(first.value), float(ms.value)


def convolve_last_frames(count, taps, mode=0, tag=0, timed=True):
    """beamformer_hip_convolve_last_frames: `count` new frames of the frame ring, the `count` newest ones filtered along x, y and z in
    that order -- taps: three sequences of an odd number of real taps, (x, y, z), or None for an axis that is left alone; a true
    convolution (taps (0, 0, 1) move the frame by +1 voxel), terms outside the frame skipped.  mode: P.HipSpatialMode -- Zero: plain
    IEEE; Normalised: the weights renormalised over the finite in-frame voxels under the taps (taps >= 0): no darkening at the edges, NaN
    holes filled.  Returns (first_frame_id, device_ms): the id of the oldest output; timed False: the call does not synchronise and
    device_ms is 0."""
    if len(taps) != 3:
        raise ValueError("taps: one sequence (or None) per axis, x, y, z")
    arrays = [None if h is None else np.ascontiguousarray(np.asarray(h, np.float32).reshape(-1)) for h in taps]
    pointers = (C.POINTER(C.c_float) * 3)(*[None if h is None or not h.size else h.ctypes.data_as(C.POINTER(C.c_float)) for h in arrays])
    counts = (C.c_uint32 * 3)(*[0 if h is None else int(h.size) for h in arrays])
    first, ms = C.c_uint32(0), C.c_float(0)
    _check(library().beamformer_hip_convolve_last_frames(int(count), pointers, counts, int(mode), int(tag), C.byref(first),
                                                         C.byref(ms) if timed else None))
    return int(first.value), float(ms.value)


def correlate_last_frames(count, reference, max_shift, regions=None):
    """beamformer_hip_correlate_last_frames: each of the `count` newest frames (one grid, one kind) correlated on the device with frame
    `reference` of them (0: the oldest) at every integer shift |s_a| <= max_shift[a] (x, y, z), over each box of `regions` (a sequence
    of HipFrameRegion: see frame_region()); regions None: one box, the frames whole.  Returns (table, info, device_ms): a structured
    array (P.HipShiftCorrelation's fields) of shape (R, count, 2 Sz + 1, 2 Sy + 1, 2 Sx + 1) -- table[r, k, sz + Sz, sy + Sy, sx + Sx];
    if frame k is the reference moved by d voxels, |re + i im| peaks at s = d --, the HipCorrelationInfo and the device time of the
    launches."""
    count, reference = int(count), int(reference)
    S = [int(v) for v in max_shift]
    if len(S) != 3:
        raise ValueError("max_shift: one number per axis, x, y, z")
    boxes = None if regions is None else list(regions)
    R = 1 if boxes is None else len(boxes)
    window = [2 * v + 1 if 0 <= v <= P.HIP_MAX_SHIFT else 1 for v in S]
    shape = (max(1, R), max(1, count), window[2], window[1], window[0])
    if int(np.prod(shape)) > P.HIP_MAX_CORRELATION_ENTRIES:
        shape = (1, 1, 1, 1, 1)         # the call refuses before it writes: room for nothing
    table = np.zeros(shape, np.dtype(P.HipShiftCorrelation))
    array = None if boxes is None else (P.HipFrameRegion * max(1, R))(*boxes)
    info, ms = P.HipCorrelationInfo(), C.c_float(0)
    _check(library().beamformer_hip_correlate_last_frames(count, reference, array, R, (C.c_uint32 * 3)(*[v & 0xFFFFFFFF for v in S]),
                                                          table.ctypes.data_as(C.POINTER(P.HipShiftCorrelation)), C.byref(info), C.byref(ms)))
    return table, info, float(ms.value)


def displacements_from_correlation(tables, max_shift, normalised=True):
    """beamformer_hip_displacements_from_correlation (host only): one displacement a table.  tables: what correlate_last_frames returns,
    or any array of P.HipShiftCorrelation entries whose last axes hold whole tables of T = prod(2 max_shift + 1) entries.  Returns a
    structured array (P.HipDisplacement's fields) with the leading shape of `tables` -- (R, K) for correlate_last_frames' table; an
    empty table's row is zero.  Raises when no table has a candidate."""
    tables = np.ascontiguousarray(tables, np.dtype(P.HipShiftCorrelation))
    S = [int(v) for v in max_shift]
    T = int(np.prod([2 * v + 1 for v in S]))
    n = tables.size // T if T > 0 and tables.size % T == 0 else 0
    lead = tables.shape[:-3] if tables.ndim >= 3 and tables.shape[-3:] == (2 * S[2] + 1, 2 * S[1] + 1, 2 * S[0] + 1) else (n,)
    out = np.zeros(max(1, n), np.dtype(P.HipDisplacement))
    _check(library().beamformer_hip_displacements_from_correlation(tables.ctypes.data_as(C.POINTER(P.HipShiftCorrelation)), n,
                                                                   (C.c_uint32 * 3)(*[v & 0xFFFFFFFF for v in S]), 1 if normalised else 0,
                                                                   out.ctypes.data_as(C.POINTER(P.HipDisplacement))))
    return out[:n].reshape(lead)


def warp_last_frames(count, displacements, nodes=(1, 1, 1), node_first=(0, 0, 0), node_step=(1, 1, 1), rotations=None,
                     interpolation=P.HipWarpInterpolation.Linear, edge=P.HipWarpEdge.Zero, tag=0, timed=True):
    """beamformer_hip_warp_last_frames: `count` new frames of the frame ring, output n the n-th of the `count` newest ones sampled at
    v + d_n(v).  displacements: count x nodes z x nodes y x nodes x x 3 floats (any shape of that size), voxels (x, y, z) at the nodes
    of a lattice of nodes = (x, y, z) nodes an axis, node j of axis a at voxel coordinate node_first[a] + j * node_step[a]; nodes
    (1, 1, 1): one rigid shift a frame, a HipDisplacement's `displacement` as it is.  The field is trilinear between the nodes and
    constant outside them.  rotations: None, or `count` complex factors applied to the outputs (exp(-1j * phase) of a displacement).
    interpolation: P.HipWarpInterpolation (Linear, Cubic: Catmull-Rom); edge: P.HipWarpEdge (Zero: terms outside the frame are
    skipped; Clamp: the edge voxel repeats).  Returns (first_frame_id, device_ms): the id of the oldest output; timed False: the
    call does not synchronise and device_ms is 0."""
    count = int(count)
    N = [int(v) for v in nodes]
    if len(N) != 3 or len(node_first) != 3 or len(node_step) != 3:
        raise ValueError("nodes, node_first, node_step: one number per axis, x, y, z")
    field = np.ascontiguousarray(np.asarray(displacements, np.float32).reshape(-1))
    product = N[0] * N[1] * N[2]
    if 0 < product <= P.HIP_MAX_WARP_NODES and 0 < count <= P.HIP_MAX_ENSEMBLE_FRAMES and field.size != 3 * count * product:
        raise ValueError("displacements: count x nodes z x nodes y x nodes x x 3 floats")
    rot = None
    if rotations is not None:
        rot = np.ascontiguousarray(np.asarray(rotations, np.complex64).reshape(-1))
        if rot.size != count:
            raise ValueError("rotations: one complex factor a frame")
    floats = C.POINTER(C.c_float)
    first, ms = C.c_uint32(0), C.c_float(0)
    _check(library().beamformer_hip_warp_last_frames(count, field.ctypes.data_as(floats), (C.c_uint32 * 3)(*[v & 0xFFFFFFFF for v in N]),
                                                     (C.c_float * 3)(*[float(v) for v in node_first]), (C.c_float * 3)(*[float(v) for v in node_step]),
                                                     None if rot is None else rot.ctypes.data_as(floats), int(interpolation), int(edge), int(tag),
                                                     C.byref(first), C.byref(ms) if timed else None))
    return int(first.value), float(ms.value)


def frame_info(frame_id):
    """beamformer_hip_get_frame_info: the HipFrameInfo of the frame with this id, while it is still in the frame ring."""
    info = P.HipFrameInfo()
    _check(library().beamformer_hip_get_frame_info(int(frame_id), C.byref(info)))
    return info


def copy_frame(frame_id):
    """beamformer_hip_copy_frame: the frame with this id, as float32 or complex64 of shape (Z, Y, X) -- its own points and kind."""
    info = frame_info(frame_id)
    raw = np.zeros(int(info.size_bytes) // 4, dtype=np.float32)
    _check(library().beamformer_hip_copy_frame(int(frame_id), raw.ctypes.data_as(C.c_void_p), raw.nbytes))
    shape = (int(info.points[2]), int(info.points[1]), int(info.points[0]))
    voxels = int(np.prod(shape))
    if info.data_kind == int(P.DataKind.Float32Complex):
        return raw[: 2 * voxels].view(np.complex64).reshape(shape)
    return raw[:voxels].reshape(shape)


def beamform_burst_views(bp, rf_frames, views, filters=(), timeout_ms=-1, on_device_pointer=None):
    """N RF frames on K grids in one call (beamformer_hip_push_data_burst_views_with_compute): `rf_frames` as beamform_burst() takes it,
    `views` as beamform_views() does.  Returns a list of K lists of N arrays (Z, Y, X): [v][k] is (view v, RF frame k) -- the order the
    frames are queued in, view-major."""
    _prepared(bp, filters, timeout_ms)
    rf_frames = np.ascontiguousarray(rf_frames)
    n = rf_frames.shape[0]
    frame_size = rf_frames.nbytes // n
    views = list(views)
    array, count = _view_array(views)
    _push("burst_views", rf_frames, on_device_pointer, frame_size, n, array, count, 0)
    flat = get_last_views([v for v in views for _ in range(n)])
    return [flat[v * n:(v + 1) * n] for v in range(count)]


def describe_burst_views(bp, n, views, filters=(), slot=0):
    """What a burst views push of n RF frames on these grids would run (beamformer_hip_describe_burst_views): the description struct;
    .rung is the ladder's rung, .path[k] view k's own single-frame decision, .reason says why.  Needs no device."""
    L = _described(bp, filters, slot)
    array, count = _view_array(views)
    d = P.HipBurstViewsDescription()
    _check(L.beamformer_hip_describe_burst_views(slot, n, array, count, C.byref(d)))
    return d


def last_burst_views_info():
    """beamformer_hip_get_last_burst_views_info: the newest burst views push's route, ids and whole-push stage times; waits for it."""
    info = P.HipBurstViewsInfo()
    _check(library().beamformer_hip_get_last_burst_views_info(C.byref(info)))
    return info


def get_last_frame(bp, shard_planes=None):
    lib = library()
    shape = list(frame_shape(bp))
    if shard_planes is not None:
        shape[0] = shard_planes
    info = P.HipFrameInfo()
    _check(lib.beamformer_hip_get_last_frame_info(C.byref(info)))
    complex_out = info.data_kind == int(P.DataKind.Float32Complex)
    voxels = int(np.prod(shape))
    # with several devices the info describes the ingest device's slab; the export is the whole frame
    whole = (voxels * (8 if complex_out else 4) + 63) // 64 * 64
    raw = np.empty((max(int(info.size_bytes), whole) + 3) // 4, dtype=np.float32)
    _check(lib.beamformer_get_last_frames(raw.ctypes.data_as(C.c_void_p), raw.nbytes, 1))
    if complex_out:
        return raw[: 2 * voxels].view(np.complex64).reshape(shape)
    return raw[:voxels].reshape(shape)


def das_input(bp, frame=None, transmits=None):
    """beamformer_hip_copy_das_input: what the newest frame's DAS stage read, as float32 or complex64 of shape
    (channels, transmits, DAS samples); frame = k: RF frame k of the newest push (beamformer_hip_copy_das_input_frame: a burst's
    frame k).  transmits: the transmit count where it is not the block's (a READI image push's decoded input: G x A).  Valid until the
    next push; one device only."""
    lib = library()
    plan = P.HipPlan()
    _check(lib.beamformer_hip_describe_plan(0, C.byref(plan)))
    shape = (int(bp.channel_count), int(bp.acquisition_count if transmits is None else transmits), int(plan.das_samples))
    out = np.empty(int(np.prod(shape)), np.complex64 if plan.iq_pipeline else np.float32)
    if frame is None:
        _check(lib.beamformer_hip_copy_das_input(out.ctypes.data_as(C.c_void_p), out.nbytes))
    else:
        _check(lib.beamformer_hip_copy_das_input_frame(frame, out.ctypes.data_as(C.c_void_p), out.nbytes))
    return out.reshape(shape)


def load_zbp(path, frame_number=0):
    """(SimpleParameters, raw RF bytes as a numpy uint8 array) from a ZBP .bp file, through the
    library's loader (tests/throughput.c:150-374 of the reference)."""
    lib = library()
    bp = P.SimpleParameters()
    rf, size = C.c_void_p(), C.c_uint64()
    if not lib.beamformer_hip_zbp_load(os.fsencode(path), frame_number, C.byref(bp), C.byref(rf), C.byref(size)):
        raise ValueError(f"{path}: {lib.beamformer_hip_zbp_last_error().decode()}")
    try:
        data = np.ctypeslib.as_array(C.cast(rf, C.POINTER(C.c_uint8)), shape=(size.value,)).copy()
    finally:
        lib.beamformer_hip_zbp_free(rf)
    return bp, data


def set_hook(name, value=None):
    """beamformer_hip_set_hook: a test / measurement hook of the library (name without the BEAMFORMER_HIP_ prefix; None = off)"""
    ok = library().beamformer_hip_set_hook(name.encode(), None if value is None else str(value).encode())
    assert ok, f"unknown hook {name}"


def describe_das(bp, filters=(), slot=0):
    """The DAS kernel the library would run for these parameters under the current das path mode, and why the others
    were declined (beamformer_hip_describe_das): (path, kernel, name, {path number: reason}, description struct).  Needs no device."""
    L = _described(bp, filters, slot)
    d = P.HipDasDescription()
    assert L.beamformer_hip_describe_das(slot, C.byref(d)), last_error()
    reasons = {k: bytes(d.declined[k]).split(b"\0")[0].decode() for k in range(8)}
    return int(d.path), d.kernel.decode(), d.name.decode(), reasons, d


def describe_upload(bp, data_size, frame_count=1, device_pointer=None, filters=(), slot=0):
    """How the RF of a push of these parameters would reach the RF ring (beamformer_hip_describe_upload): the description struct;
    .route is a P.UploadRoute, .name says it in words.  data_size: the bytes of one raw frame; device_pointer: the address a
    device-resident push would be given, None for host data.  Needs no device."""
    L = _described(bp, filters, slot)
    d = P.HipUploadDescription()
    _check(L.beamformer_hip_describe_upload(slot, data_size, frame_count, C.c_void_p(device_pointer), C.byref(d)))
    return d
